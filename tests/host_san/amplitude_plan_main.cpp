// The host-side plan of the amplitude chains (csrc/qk_local_plan.h: the AMP_* kinds) on a hand-made set over 6 sites: the string
// tiles of a state (every string once, ragged tails), the regions of a chain's slot against what the launches index, the task
// counts and the launch count, the per-site launch lists of a chain batch that does not start at chain 0, the same work whatever the
// cut into chain batches, the state batch with and without the environment pass, the check of the outcome bytes and the log
// likelihood of a mantissa and an exponent.  Every expected value is restated here from the definitions, not taken from the header.
// Built with g++ -fsanitize=address,undefined and run by tests/test_amplitude_plan.py; prints one line per section, exits 1 on a
// mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

using namespace qkl;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr int N = 6, N1 = N + 1, NS = 3;
const int32_t TRU[NS * N1] = {
    1, 2, 4,  8,  4,  2, 1,
    1, 2, 17, 70, 33, 2, 1,
    1, 2, 4,  50, 64, 4, 1,
};
const int PAD[NS * N1] = {
    16, 16, 16, 16, 16, 16, 16,
    16, 16, 32, 80, 48, 16, 16,
    16, 16, 16, 64, 64, 16, 16,
};
const int PMAX[NS] = {16, 80, 64};
constexpr int MAXPAD = 80;

long long b64(const long long m, const long long n) { return ((m + 63) / 64) * ((n + 63) / 64); }

EnvSizes sizes(const bool keep_l = false) {
  EnvSizes z;
  env_sizes(TRU, NS, N, MAXPAD, LOC_RMUL, keep_l, z);
  return z;
}

void test_tiles() {
  const EnvSizes z = sizes();
  CHECK(AMP_TILE == 64);
  const int cases[][2] = {{140, 64}, {1, 64}, {64, 64}, {65, 64}, {100, 32}, {17, 16}, {128, 64}};
  for (const auto& cs : cases) {
    const int strings = cs[0], tile = cs[1];
    const SmpChains c = list_amp_chains(z, 1, 2, strings, tile);  // states 1 and 2
    const int tiles = (strings + tile - 1) / tile;
    CHECK((int)c.cent.size() == 2 * tiles);
    for (int i = 0; i < 2; ++i) {
      std::vector<int> seen(strings, 0);
      for (int t = 0; t < tiles; ++t) {
        const size_t e = (size_t)i * tiles + t;
        CHECK(c.cent[e] == i && c.shot0[e] == t * tile);
        CHECK(c.rows[e] >= 1 && c.rows[e] <= tile && (t + 1 < tiles ? c.rows[e] == tile : c.rows[e] == strings - t * tile));
        for (int r = 0; r < c.rows[e]; ++r) ++seen[c.shot0[e] + r];
        const int R = smp_rows_pad(c.rows[e]);
        CHECK(R % 16 == 0 && R >= c.rows[e] && R < c.rows[e] + 16);
        CHECK(c.slot[e] == 6ll * PMAX[1 + i] * R);  // V: 2 P R, W: 4 P R -- the sampler's slot is 14 P R
      }
      for (int s = 0; s < strings; ++s) CHECK(seen[s] == 1);
    }
  }
  std::printf("ok  tiles\n");
}

// the regions of a slot, in doubles, for P and R: V [P][R], W [R][2P], each twice (re, im)
void test_slot() {
  CHECK(amp_V() == 0 && amp_W() - amp_V() == 2 && amp_size() - amp_W() == 4);
  // the largest element every launch touches, for state 1 (P = 80) and a ragged tile of 12 strings (R = 16), lies inside its region
  const int P = PMAX[1], R = smp_rows_pad(12);
  const long long PR = (long long)P * R;
  CHECK(16ll * R <= PR);  // the init kernel: the first 16 bond rows of V
  for (int k = 0; k < N; ++k) {
    const long long l = PAD[N1 + k], r = PAD[N1 + k + 1];
    CHECK((l - 1) * R + (R - 1) < PR);            // V[b][row], ld R, plane P R: the A operand of AMP_W
    CHECK((r - 1) * R + (R - 1) < PR);            // the next V the pick kernel writes
    CHECK((R - 1) * 2 * r + 2 * r - 1 < 2 * PR);  // W[row][(t, b')], ld 2 r, plane 2 P R
  }
  std::printf("ok  slot\n");
}

long long expected_tasks(const int kind, const int k, const int* p, const int R) {
  if (kind == AMP_W) return b64(R, 2 * p[k + 1]);  // W [R][2 pad_{k+1}]
  return R / 16;                                   // 16-row chunks of the strings
}

void test_counts() {
  const EnvSizes z = sizes();
  CHECK(AMP_KINDS[0] == AMP_W && AMP_KINDS[1] == AMP_PICK && AMP_W >= 0 && AMP_PICK < 0 && !conj_b(AMP_W));
  const int every[] = {LOC_REV_T, LOC_REV_X, LOC_FWD_T, LOC_FWD_W, LOC_PAIR_T, LOC_PAIR_V, LOC_DIST_T, LOC_DIST_X, LOC_BOND_M, STR_T, STR_X, BLK_T, BLK_X, BLK_V, BLK_W,
                       LOC_RHO, LOC_PAIR_RHO, LOC_DIST_RHO, LOC_ADMIT, LOC_BOND_TR, STR_LNEXT, STR_PAULI, STR_CLOSE, BLK_RED, SMP_W, SMP_Q, SMP_ROT, SMP_DRAW, WIN_G,
                       WIN_H, WIN_CLOSE};
  for (const int other : every) CHECK(other != AMP_W && other != AMP_PICK);  // the new kinds take no number that is in use
  for (const int n : {1, 2, N, 40}) CHECK(amp_launches(n) == 2 * n + 1);      // half the sampler's 4 n, plus the init kernel
  for (int s = 0; s < NS; ++s)
    for (const int R : {16, 48, 64, 128})
      for (int k = 0; k < N; ++k) {
        for (const int kind : AMP_KINDS) CHECK(amp_task_count(kind, k, &z.pad[(size_t)s * N1], R) == expected_tasks(kind, k, PAD + s * N1, R));
        CHECK(amp_task_count(AMP_W, k, &z.pad[(size_t)s * N1], R) == smp_task_count(SMP_W, k, &z.pad[(size_t)s * N1], R));  // the sampler's shape
      }
  // a chain's tasks and weight: 140 strings of state 1 are tiles of 64, 64 and 12 rows
  const SmpChains c = list_amp_chains(z, 1, 1, 140, 64);
  CHECK(c.cent.size() == 3);
  for (size_t e = 0; e < c.cent.size(); ++e) {
    const int R = e < 2 ? 64 : 16;
    long long nt = 0;
    for (int k = 0; k < N; ++k)
      for (const int kind : AMP_KINDS) nt += expected_tasks(kind, k, PAD + N1, R);
    CHECK(c.ntasks[e] == nt && c.weight[e] >= c.slot[e] + nt);
  }
  std::printf("ok  counts\n");
}

void test_lists() {
  const EnvSizes z = sizes();
  const SmpChains c = list_amp_chains(z, 0, NS, 70, 64);  // 6 chains: (state, tile) = (0,0) (0,1) (1,0) (1,1) (2,0) (2,1)
  CHECK(c.cent.size() == 6);
  std::vector<Task2> tasks;
  std::vector<long long> first;
  const size_t c0 = 1, nc = 4;  // a batch that starts inside state 0 and ends inside state 2
  amp_lists(z, 0, c, c0, nc, tasks, first);
  CHECK(first.size() == 2 * N + 1 && first[0] == 0 && first.back() == (long long)tasks.size());
  long long total = 0;
  for (int k = 0; k < N; ++k)
    for (int j = 0; j < 2; ++j) {
      const size_t li = 2 * k + j;
      long long at = first[li];
      for (size_t e = 0; e < nc; ++e) {  // chain-major, blocks ascending
        const int s = c.cent[c0 + e], R = smp_rows_pad(c.rows[c0 + e]);
        const long long want = expected_tasks(AMP_KINDS[j], k, PAD + s * N1, R);
        for (long long b = 0; b < want; ++b, ++at) CHECK(at < first[li + 1] && tasks[at].x == (int)e && tasks[at].y == (int)b);
      }
      CHECK(at == first[li + 1]);
      total += first[li + 1] - first[li];
    }
  long long nt = 0;
  for (size_t e = 0; e < nc; ++e) nt += c.ntasks[c0 + e];
  CHECK(total == nt);
  std::printf("ok  lists\n");
}

// the work of a call is the same whatever the cut: per launch, the (global chain, block) pairs of all batches together
void test_cuts() {
  const EnvSizes z = sizes();
  const SmpChains c = list_amp_chains(z, 0, NS, 150, 64);  // 9 chains
  const size_t nch = c.cent.size();
  CHECK(nch == 9);
  std::map<std::pair<int, long long>, int> ref;
  bool have_ref = false;
  long long all = 0;
  for (size_t e = 0; e < nch; ++e) all += c.weight[e];
  const long long rooms[] = {all, all / 2, c.weight[2] + c.weight[3], 1};
  for (const long long cap : {0ll, 1ll, 3ll, 100ll})
    for (const long long room : rooms) {
      const std::vector<size_t> cstart = chain_cut(c.weight, room, cap);
      CHECK(cstart.front() == 0 && cstart.back() == nch);
      std::map<std::pair<int, long long>, int> got;  // (launch, chain * 2^20 + block) -> times
      for (size_t cb = 0; cb + 1 < cstart.size(); ++cb) {
        const size_t c0 = cstart[cb], nc = cstart[cb + 1] - c0;
        CHECK(nc >= 1 && (cap == 0 || (long long)nc <= cap));
        long long w = 0;
        for (size_t e = c0; e < c0 + nc; ++e) w += c.weight[e];
        CHECK(nc == 1 || w <= room);
        std::vector<Task2> tasks;
        std::vector<long long> first;
        amp_lists(z, 0, c, c0, nc, tasks, first);
        for (size_t li = 0; li + 1 < first.size(); ++li)
          for (long long t = first[li]; t < first[li + 1]; ++t) ++got[{(int)li, ((long long)(c0 + tasks[t].x) << 20) + tasks[t].y}];
      }
      for (const auto& kv : got) CHECK(kv.second == 1);
      if (!have_ref) ref = got, have_ref = true;
      CHECK(got == ref);
    }
  std::printf("ok  cuts\n");
}

// a state batch without <psi|psi> is its tables alone (an empty plan: no tasks, no L offsets); with it, the environment pass of the
// Pauli strings, every L_k kept
void test_env() {
  const EnvSizes z = sizes();
  EnvTables eb;
  env_tables(z, Plan{}, 1, 2, 0, eb);
  CHECK(eb.tasks.empty() && eb.first.size() == 1 && eb.first[0] == 0 && eb.b_tasks == 0 && eb.h_loff.empty());
  CHECK(eb.h_states[0] == 1 && eb.h_states[1] == 2 && eb.h_pmax[0] == PMAX[1] && eb.tot == z.need[1] + z.need[2]);
  const EnvSizes zl = sizes(true);
  EnvTables el;
  env_tables(zl, env_plan(N), 0, NS, 0, el);
  CHECK(zl.keep_l && el.h_loff.size() == (size_t)NS * N1 && el.first.size() == 2 * (N - 1) + 3 * N + 1);
  for (int s = 0; s < NS; ++s) {
    long long need = 14ll * PMAX[s] * PMAX[s];
    for (int k = 1; k <= N; ++k) need += 2ll * PAD[s * N1 + k] * PAD[s * N1 + k];
    CHECK(z.need[s] == need);
    for (int k = 0; k < N; ++k) need += 2ll * PAD[s * N1 + k] * PAD[s * N1 + k];
    CHECK(zl.need[s] == need);
  }
  // a one-site chain: one GEMM block and one chunk
  const int32_t one[2] = {1, 1};
  EnvSizes z1;
  env_sizes(one, 1, 1, 16, LOC_RMUL, false, z1);
  const SmpChains c1 = list_amp_chains(z1, 0, 1, 5, 64);
  CHECK(c1.cent.size() == 1 && c1.rows[0] == 5 && c1.ntasks[0] == 1 + 1 && c1.slot[0] == 6 * 16 * 16);
  std::printf("ok  env\n");
}

void test_bits_and_logp() {
  std::vector<uint8_t> b(140 * N, 0);
  CHECK(amp_bad_bit(b.data(), (long long)b.size()) == -1);
  b[5] = 1, b[6] = 1;
  CHECK(amp_bad_bit(b.data(), (long long)b.size()) == -1);
  b[200] = 2;
  CHECK(amp_bad_bit(b.data(), (long long)b.size()) == 200);
  b[100] = 255;
  CHECK(amp_bad_bit(b.data(), (long long)b.size()) == 100);
  CHECK(amp_bad_bit(b.data(), 100) == -1);
  // log(|v 2^E|^2 / norm): amplitude 1/2 of a state of norm 2 is probability 1/8; a zero amplitude is -inf; 2^-2000 survives
  CHECK(std::fabs(amp_logp(0.5, 0.0, 0, std::log(2.0)) - std::log(0.125)) < 1e-15);
  CHECK(std::fabs(amp_logp(0.0, -0.5, 1, 0.0)) < 1e-15);
  CHECK(std::fabs(amp_logp(0.6, 0.8, 3, 0.0) - 6.0 * std::log(2.0)) < 1e-14);
  CHECK(std::isinf(amp_logp(0.0, 0.0, 0, 0.0)) && amp_logp(0.0, 0.0, 0, 0.0) < 0);
  CHECK(std::fabs(amp_logp(0.5, 0.5, -2000, 0.0) - (2.0 * (-2000.0 - 0.5) * std::log(2.0))) < 1e-11);
  std::printf("ok  bits\n");
}

}  // namespace

int main() {
  test_tiles();
  test_slot();
  test_counts();
  test_lists();
  test_cuts();
  test_env();
  test_bits_and_logp();
  if (failures) std::printf("FAIL: %d check(s)\n", failures);
  return failures ? 1 : 0;
}
