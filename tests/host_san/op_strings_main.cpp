// The plan side of the strings of single-site operators (csrc/qk_local_plan.h: operator_supports) on two hand-made states over 7
// sites: supports with codes up to 255, the index of the first code above n_ops, that string_supports is the n_ops = 3 case, and
// that the chains, their weights, the cut and the task lists of an operator string equal those of the Pauli string with the same
// zeros.  Every expected support is restated here from the definition.  Built with g++ -fsanitize=address,undefined and run by
// tests/test_op_strings_plan.py; prints one line per section, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <cstdio>
#include <numeric>
#include <vector>

using namespace qkl;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr int NS = 2, N = 7, N1 = N + 1;
const int32_t TRU[NS * N1] = {
    1, 2, 4,  8,  4,  2,  1, 1,  // pads to 16 everywhere
    1, 2, 17, 70, 150, 33, 2, 1,  // pads to 16, 16, 32, 80, 160, 48, 16, 16: two 64-blocks with a ragged second one at bond 3
};
constexpr int MAX_PAD = 160;

constexpr int NSTR = 8;
// codes 0 .. 255; the Pauli twin of a row has 1 + (code % 3) wherever the code is not 0
const uint8_t CODES[NSTR][N] = {
    {0, 0, 0, 0, 0, 0, 0},          // all identity: no chain
    {255, 0, 0, 0, 0, 0, 0},        // a single site, the first
    {0, 0, 0, 0, 0, 0, 200},        // a single site, the last
    {0, 5, 0, 0, 17, 0, 0},         // an identity gap
    {1, 2, 3, 4, 5, 6, 7},          // the whole chain
    {0, 0, 129, 255, 0, 0, 0},      // two neighbours inside
    {9, 0, 0, 0, 0, 0, 9},          // the two ends
    {0, 0, 0, 64, 0, 0, 0},         // a single site inside
};
const int SUPP[NSTR][2] = {{-1, -1}, {0, 0}, {6, 6}, {1, 4}, {0, 6}, {2, 3}, {0, 6}, {3, 3}};

void test_supports() {
  std::vector<uint8_t> codes(&CODES[0][0], &CODES[0][0] + NSTR * N);
  std::vector<int32_t> supp;
  CHECK(operator_supports(codes.data(), NSTR, N, 255, supp) == -1 && supp.size() == 2 * NSTR);
  for (int m = 0; m < NSTR; ++m) CHECK(supp[2 * m] == SUPP[m][0] && supp[2 * m + 1] == SUPP[m][1]);
  // the first code above n_ops, in row-major order: codes[1][0] = 255 for every n_ops below 255 that admits row 0
  for (const int n_ops : {1, 3, 8, 199, 254}) CHECK(operator_supports(codes.data(), NSTR, N, n_ops, supp) == 1 * N + 0);
  {
    std::vector<uint8_t> low = codes;  // without row 1 and the 255 of row 5, the first offender depends on n_ops
    low[1 * N + 0] = 1, low[5 * N + 3] = 2;
    CHECK(operator_supports(low.data(), NSTR, N, 199, supp) == 2 * N + 6);    // 200
    CHECK(operator_supports(low.data(), NSTR, N, 200, supp) == -1);
    CHECK(operator_supports(low.data(), NSTR, N, 128, supp) == 2 * N + 6);
    low[2 * N + 6] = 3;
    CHECK(operator_supports(low.data(), NSTR, N, 16, supp) == 3 * N + 4);     // 17
    CHECK(operator_supports(low.data(), NSTR, N, 4, supp) == 3 * N + 1);      // 5
    CHECK(operator_supports(low.data(), NSTR, N, 128, supp) == 5 * N + 2);    // 129
    CHECK(operator_supports(low.data(), NSTR, N, 129, supp) == -1);
  }
  // string_supports is the n_ops = 3 case: same supports on Pauli codes, same offender
  std::vector<uint8_t> pauli(codes.size());
  for (size_t e = 0; e < codes.size(); ++e) pauli[e] = codes[e] ? (uint8_t)(1 + codes[e] % 3) : 0;
  std::vector<int32_t> s3, sp;
  CHECK(operator_supports(pauli.data(), NSTR, N, 3, s3) == -1 && string_supports(pauli.data(), NSTR, N, sp) == -1 && s3 == sp);
  for (int m = 0; m < NSTR; ++m) CHECK(sp[2 * m] == SUPP[m][0] && sp[2 * m + 1] == SUPP[m][1]);
  pauli[4 * N + 2] = 4, pauli[6 * N + 0] = 9;
  CHECK(string_supports(pauli.data(), NSTR, N, sp) == 4 * N + 2 && operator_supports(pauli.data(), NSTR, N, 3, s3) == 4 * N + 2);
  CHECK(OPSTR_MAX_OPS == 255);
  std::printf("ok  supports\n");
}

bool same_tasks(const std::vector<Task2>& a, const std::vector<Task2>& b) {
  if (a.size() != b.size()) return false;
  for (size_t e = 0; e < a.size(); ++e)
    if (a[e].x != b[e].x || a[e].y != b[e].y) return false;
  return true;
}

void test_chains_equal_the_pauli_plan() {
  std::vector<uint8_t> codes(&CODES[0][0], &CODES[0][0] + NSTR * N), pauli(NSTR * N);
  for (size_t e = 0; e < codes.size(); ++e) pauli[e] = codes[e] ? (uint8_t)(1 + codes[e] % 3) : 0;
  std::vector<int32_t> so, sp;
  CHECK(operator_supports(codes.data(), NSTR, N, 255, so) == -1 && string_supports(pauli.data(), NSTR, N, sp) == -1 && so == sp);
  EnvSizes z;
  env_sizes(TRU, NS, N, MAX_PAD, LOC_RMUL, true, z);
  for (int s0 = 0; s0 < NS; ++s0) {
    const int nb = NS - s0;
    const Chains co = list_chains(z, s0, nb, NSTR, codes.data(), so), cp = list_chains(z, s0, nb, NSTR, pauli.data(), sp);
    const size_t nch = (size_t)nb * (NSTR - 1);
    CHECK(co.cent.size() == nch && co.cent == cp.cent && co.cstr == cp.cstr && co.ntasks == cp.ntasks && co.weight == cp.weight);
    // a chain has an elementwise task at a site exactly where its code is not 0: p[k] / 16 chunks
    for (size_t e = 0; e < nch; ++e) {
      const int m = co.cstr[e];
      const int32_t* p = &z.pad[(size_t)(s0 + co.cent[e]) * N1];
      for (int k = 0; k < N; ++k)
        CHECK(chain_task_count(STR_PAULI, k, p, &codes[(size_t)m * N], so[2 * m], so[2 * m + 1], N) == (CODES[m][k] ? p[k] / 16 : 0));
    }
    const long long all = std::accumulate(co.weight.begin(), co.weight.end(), 0ll);
    std::vector<Task2> to, tp;
    std::vector<long long> fo, fp;
    for (const long long cap : {0ll, 1ll, 3ll})
      for (const long long room : {all, all / 3, 0ll}) {
        const std::vector<size_t> cs = chain_cut(co.weight, room, cap);
        CHECK(cs == chain_cut(cp.weight, room, cap) && cs.front() == 0 && cs.back() == nch);
        for (size_t cb = 0; cb + 1 < cs.size(); ++cb) {
          const size_t c0 = cs[cb], nc = cs[cb + 1] - c0;
          CHECK(nc >= 1 && (cap == 0 || (long long)nc <= cap));
          chain_lists(z, s0, co, c0, nc, codes.data(), so, to, fo);
          chain_lists(z, s0, cp, c0, nc, pauli.data(), sp, tp, fp);
          CHECK(fo == fp && same_tasks(to, tp) && fo.size() == 4 * N + 1 && fo.back() == (long long)to.size());
          for (const Task2& t : to) CHECK(t.x >= 0 && t.x < (int)nc && t.y >= 0);
        }
      }
  }
  std::printf("ok  chains\n");
}

}  // namespace

int main() {
  test_supports();
  test_chains_equal_the_pauli_plan();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
