// The plan side of the MPO observables (csrc/qk_local_plan.h: mpo_plan, mpo_task_count, list_mpo_chains, mpo_lists) on two hand-made
// states over 7 sites and four hand-made MPOs: supports, block lists (sorted by v then u, zero blocks dropped, a v without a block),
// the slot regions, the task counts of the four launch kinds, the chains and that every cut covers every chain once with task lists
// that hold the chains' tasks.  Every expected number is restated here from the definitions.  Built with
// g++ -fsanitize=address,undefined and run by tests/test_mpo_plan.py; prints one line per section, exits 1 on a mismatch.
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
    1, 2, 4,  8,  4,   2,  1, 1,  // pads to 16 everywhere
    1, 2, 17, 70, 150, 33, 2, 1,  // pads to 16, 16, 32, 80, 160, 48, 16, 16
};
const int PAD1[N1] = {16, 16, 32, 80, 160, 48, 16, 16};
constexpr int MAX_PAD = 160;

constexpr int NM = 4;
const int32_t BONDS[NM * N1] = {
    1, 1, 1, 1, 1, 1, 1, 1,  // MPO 0: all identity, no chain
    1, 1, 2, 3, 3, 1, 1, 1,  // MPO 1: support [1, 4], bonds up to 3
    1, 1, 1, 1, 1, 1, 1, 1,  // MPO 2: bond 1, operators on sites 2 and 5, identities between: support [2, 5]
    1, 2, 2, 2, 2, 2, 2, 1,  // MPO 3: the whole chain, bond 2
};

void put(std::vector<double>& t, const double re, const double im) { t.push_back(re), t.push_back(im); }
void block(std::vector<double>& t, const double a, const double b, const double c, const double d) { put(t, a, 0.5 * a), put(t, b, -b), put(t, c, 0), put(t, 0, d); }
void zero(std::vector<double>& t) { block(t, 0, 0, 0, 0); }
void ident(std::vector<double>& t) { put(t, 1, 0), put(t, 0, 0), put(t, 0, 0), put(t, 1, 0); }

// the packed tensors; `zeros` = the (MPO, site, u, v) blocks left exactly zero
std::vector<double> tensors() {
  std::vector<double> t;
  for (int k = 0; k < N; ++k) ident(t);  // MPO 0
  // MPO 1
  ident(t);                                               // site 0
  block(t, 1, 2, 3, 4), block(t, 5, 6, 7, 8);             // site 1: [1][2], both blocks
  // site 2: [2][3] = (0,0) (0,1) (0,2) (1,0) (1,1) (1,2); (0,1) and (1,1) are zero: plane v = 1 has no block
  block(t, 1, 0, 0, 0), zero(t), block(t, 0, 0, 0, 2), block(t, 0, 3, 0, 0), zero(t), zero(t);
  // site 3: [3][3], the diagonal and (2, 0): row-major (u, v)
  for (int u = 0; u < 3; ++u)
    for (int v = 0; v < 3; ++v) (u == v || (u == 2 && v == 0)) ? block(t, u + 1, v, 0, 1) : zero(t);
  block(t, 1, 1, 1, 1), zero(t), block(t, 2, 2, 2, 2);    // site 4: [3][1], u = 1 zero
  ident(t), ident(t);                                     // sites 5, 6
  // MPO 2
  ident(t), ident(t), block(t, 0, 1, 1, 0), ident(t), ident(t), block(t, 1, 0, 0, -1), ident(t);
  // MPO 3: every block present; a -0.0 block at site 3, (1, 0), counts as zero
  block(t, 1, 2, 3, 4), block(t, 4, 3, 2, 1);
  for (int k = 1; k < N - 1; ++k)
    for (int e = 0; e < 4; ++e) {
      if (k == 3 && e == 2) {
        for (int q = 0; q < 8; ++q) t.push_back(-0.0);
      } else {
        block(t, e + 1, k, 1, 1);
      }
    }
  block(t, 1, 2, 3, 4), block(t, 4, 3, 2, 1);
  return t;
}

void test_supports_and_blocks() {
  const std::vector<double> t = tensors();
  CHECK(mpo_bad_bond(BONDS, NM, N) == -1 && mpo_doubles(BONDS, NM, N) == (long long)t.size());
  {
    std::vector<int32_t> bad(BONDS, BONDS + NM * N1);
    bad[1 * N1 + 3] = 33;
    CHECK(mpo_bad_bond(bad.data(), NM, N) == 1 * N1 + 3);
    bad[0 * N1 + 7] = 0;
    CHECK(mpo_bad_bond(bad.data(), NM, N) == 7);
    CHECK(MPO_MAX_BOND == 32);
  }
  const MpoPlan mp = mpo_plan(BONDS, t.data(), NM, N);
  const int SUPP[NM][2] = {{-1, -1}, {1, 4}, {2, 5}, {0, 6}};
  const int WMAX[NM] = {1, 3, 1, 2};
  for (int m = 0; m < NM; ++m) CHECK(mp.supp[2 * m] == SUPP[m][0] && mp.supp[2 * m + 1] == SUPP[m][1] && mp.wmax[m] == WMAX[m]);
  // the tensors lie one behind the other
  long long at = 0;
  for (int m = 0; m < NM; ++m)
    for (int k = 0; k < N; ++k) {
      CHECK(mp.toff[m * N + k] == at);
      at += 8ll * BONDS[m * N1 + k] * BONDS[m * N1 + k + 1];
    }
  // a site has a mix launch unless its tensor is the exact 1 x 1 identity
  for (int k = 0; k < N; ++k) CHECK(mp.vat[0 * N + k] == -1 && (mp.vat[1 * N + k] >= 0) == (k >= 1 && k <= 4) && (mp.vat[2 * N + k] >= 0) == (k == 2 || k == 5) && mp.vat[3 * N + k] >= 0);
  auto blocks_of = [&](const int m, const int k, const int v) {
    std::vector<int> us;
    const int a = mp.vat[m * N + k];
    for (int b = mp.vfirst[a + v]; b < mp.vfirst[a + v + 1]; ++b) {
      us.push_back(mp.blk_u[b]);
      CHECK(mp.blk_v[b] == v);
    }
    return us;
  };
  using V = std::vector<int>;
  CHECK(blocks_of(1, 1, 0) == V{0} && blocks_of(1, 1, 1) == V{0});
  CHECK(blocks_of(1, 2, 0) == (V{0, 1}) && blocks_of(1, 2, 1).empty() && blocks_of(1, 2, 2) == V{0});  // zero blocks dropped, an empty v
  CHECK(blocks_of(1, 3, 0) == (V{0, 2}) && blocks_of(1, 3, 1) == V{1} && blocks_of(1, 3, 2) == V{2});   // ascending u inside a v
  CHECK(blocks_of(1, 4, 0) == (V{0, 2}));
  CHECK(blocks_of(2, 2, 0) == V{0} && blocks_of(2, 5, 0) == V{0});
  CHECK(blocks_of(3, 3, 0) == V{0} && blocks_of(3, 3, 1) == (V{0, 1}));  // the -0.0 block (u, v) = (1, 0) is dropped
  CHECK(blocks_of(3, 2, 0) == (V{0, 1}) && blocks_of(3, 0, 1) == V{0} && blocks_of(3, 6, 0) == (V{0, 1}));
  // the whole list is sorted by (MPO, site, v, u) and holds the coefficients of its blocks
  CHECK(mp.blk_w.size() == 8 * mp.blk_u.size() && mp.blk_v.size() == mp.blk_u.size());
  {
    const int a = mp.vat[1 * N + 3], b = mp.vfirst[a + 0] + 1;  // MPO 1, site 3, v = 0, second block: u = 2
    const double* w = t.data() + mp.toff[1 * N + 3] + 8 * (2 * 3 + 0);
    for (int e = 0; e < 8; ++e) CHECK(mp.blk_w[8 * b + e] == w[e]);
  }
  std::printf("ok  supports and blocks\n");
}

void test_slot_regions() {
  // E: 2 planes of U; T and T': 2 planes of 2 U each (w pad_k rows of 2 pad_{k+1} <= 2 w P^2)
  CHECK(mpo_E() == 0 && mpo_T() == mpo_E() + 2 && mpo_Tp() == mpo_T() + 4 && mpo_size() == mpo_Tp() + 4);
  CHECK(mpo_unit(160, 3) == 3ll * 160 * 160 && mpo_unit(304, 32) == 32ll * 304 * 304);
  for (int w = 1; w <= 3; ++w)
    for (int k = 0; k < N; ++k) {
      const long long U = mpo_unit(MAX_PAD, 3);
      CHECK((long long)PAD1[k] * w * PAD1[k] <= U);                // a plane of E at the cut k
      CHECK((long long)w * PAD1[k] * 2 * PAD1[k + 1] <= 2 * U);    // a plane of T or T'
    }
  std::printf("ok  slot regions\n");
}

void test_tasks_chains_and_cuts() {
  const std::vector<double> t = tensors();
  const MpoPlan mp = mpo_plan(BONDS, t.data(), NM, N);
  EnvSizes z;
  env_sizes(TRU, NS, N, MAX_PAD, LOC_RMUL, true, z);
  const int32_t* p = &z.pad[N1];
  for (int k = 0; k <= N; ++k) CHECK(p[k] == PAD1[k]);
  // MPO 1 on state 1: site 2 (bonds 2 -> 3, pads 32 -> 80), site 3 (3 -> 3, 80 -> 160), site 4 (3 -> 1, 160 -> 48)
  CHECK(mpo_task_count(MPO_T, 2, p, mp, 1) == 1 * 3 && mpo_task_count(MPO_MIX, 2, p, mp, 1) == 3 * 2 && mpo_task_count(MPO_X, 2, p, mp, 1) == 3 * 4 && mpo_task_count(MPO_CLOSE, 2, p, mp, 1) == 0);
  CHECK(mpo_task_count(MPO_T, 3, p, mp, 1) == 4 * 5 && mpo_task_count(MPO_MIX, 3, p, mp, 1) == 3 * 5 && mpo_task_count(MPO_X, 3, p, mp, 1) == 3 * 9);
  CHECK(mpo_task_count(MPO_T, 4, p, mp, 1) == 8 * 2 && mpo_task_count(MPO_MIX, 4, p, mp, 1) == 1 * 10 && mpo_task_count(MPO_X, 4, p, mp, 1) == 1 && mpo_task_count(MPO_CLOSE, 4, p, mp, 1) == 3);
  for (const int kind : MPO_KINDS) CHECK(mpo_task_count(kind, 0, p, mp, 1) == 0 && mpo_task_count(kind, 5, p, mp, 1) == 0);  // outside the support
  // MPO 2: an identity site inside the support has the two GEMMs and no mix
  CHECK(mpo_task_count(MPO_T, 3, p, mp, 2) == 2 * 5 && mpo_task_count(MPO_MIX, 3, p, mp, 2) == 0 && mpo_task_count(MPO_X, 3, p, mp, 2) == 9);
  CHECK(mpo_task_count(MPO_MIX, 2, p, mp, 2) == 2 && mpo_task_count(MPO_CLOSE, 5, p, mp, 2) == 1);
  for (int k = 0; k < N; ++k)
    for (const int kind : MPO_KINDS) CHECK(mpo_task_count(kind, k, p, mp, 0) == 0);
  for (int s0 = 0; s0 < NS; ++s0) {
    const int nb = NS - s0;
    const Chains c = list_mpo_chains(z, s0, nb, mp);
    const size_t nch = (size_t)nb * (NM - 1);
    CHECK(c.cent.size() == nch && c.cstr.size() == nch && c.slot.size() == nch && c.ntasks.size() == nch && c.weight.size() == nch);
    for (size_t e = 0; e < nch; ++e) {  // state-major in MPO order, the all-identity MPO left out
      CHECK(c.cent[e] == (int)(e / (NM - 1)) && c.cstr[e] == 1 + (int)(e % (NM - 1)));
      const long long P = z.pmax[s0 + c.cent[e]];
      CHECK(c.slot[e] == 10ll * mp.wmax[c.cstr[e]] * P * P && c.weight[e] == c.slot[e] + 2ll * z.max_chunks + c.ntasks[e] + 2);
      long long nt = 0;
      for (int k = 0; k < N; ++k)
        for (const int kind : MPO_KINDS) nt += mpo_task_count(kind, k, &z.pad[(size_t)(s0 + c.cent[e]) * N1], mp, c.cstr[e]);
      CHECK(nt == c.ntasks[e] && nt > 0);
    }
    const long long all = std::accumulate(c.weight.begin(), c.weight.end(), 0ll);
    std::vector<Task2> tasks;
    std::vector<long long> first;
    const std::vector<ChainCol> cols{{c.cent.data(), sizeof(int32_t), 1}, {c.cstr.data(), sizeof(int32_t), 1}};
    for (const long long cap : {0ll, 1ll, 2ll, 4ll})
      for (const long long room : {all, all / 2, all / 5, 0ll}) {
        const std::vector<size_t> cs = chain_cut(c.weight, room, cap);
        CHECK(cs.front() == 0 && cs.back() == nch);
        std::vector<int> seen(nch, 0);
        for (size_t cb = 0; cb + 1 < cs.size(); ++cb) {
          const size_t c0 = cs[cb], nc = cs[cb + 1] - c0;
          CHECK(nc >= 1 && (cap == 0 || (long long)nc <= cap));
          for (size_t e = c0; e < c0 + nc; ++e) ++seen[e];
          mpo_lists(z, s0, c, c0, nc, mp, tasks, first);
          CHECK(first.size() == 4 * N + 1 && first.back() == (long long)tasks.size());
          std::vector<long long> per(nc, 0);
          for (size_t li = 0; li + 1 < first.size(); ++li)
            for (long long q = first[li]; q < first[li + 1]; ++q) {
              const Task2& tk = tasks[q];
              CHECK(tk.x >= 0 && tk.x < (int)nc);
              const int cnt = mpo_task_count(MPO_KINDS[li % 4], (int)(li / 4), &z.pad[(size_t)(s0 + c.cent[c0 + tk.x]) * N1], mp, c.cstr[c0 + tk.x]);
              CHECK(tk.y >= 0 && tk.y < cnt);
              ++per[tk.x];
            }
          for (size_t e = 0; e < nc; ++e) CHECK(per[e] == c.ntasks[c0 + e]);
          ChainStage st;
          chain_stage(cols, c, c0, c0 + nc, 2ll * z.max_chunks, tasks, st);  // the image holds the tables and the tasks, the slots follow
          CHECK(st.tasks + al256(tasks.size() * sizeof(Task2)) == st.part && st.total > st.slots && st.cbase.size() == nc && st.cbase[0] == 0);
          for (size_t e = 1; e < nc; ++e) CHECK(st.cbase[e] == st.cbase[e - 1] + c.slot[c0 + e - 1]);
        }
        for (size_t e = 0; e < nch; ++e) CHECK(seen[e] == 1);  // every chain in exactly one batch
      }
  }
  std::printf("ok  tasks, chains and cuts\n");
}

}  // namespace

int main() {
  test_supports_and_blocks();
  test_slot_regions();
  test_tasks_chains_and_cuts();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
