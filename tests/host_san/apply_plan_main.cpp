// The plan side of applying an MPO to a set (csrc/qk_local_plan.h: apply_plan on top of mpo_plan) on two hand-made ragged states over
// 7 sites and one hand-made MPO: the new true and padded bonds, the 64-bit offsets and the total, the row lists of the blocks (by u
// then v, zero blocks absent, a v without a block, a u without a block), identity sites marked as copies, tasks that cover every
// (state, site, u, chunk) exactly once and -- with the ranges the kernel writes restated here -- every double of the new image exactly
// once, the 512 limit (512 passes, 513 names its state and bond), and offsets beyond 2^31 doubles on a synthetic bond table (tables
// only, nothing is allocated).  Every expected number is restated here from the definitions.  Built with
// g++ -fsanitize=address,undefined and run by tests/test_apply_plan.py; prints one line per section, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <cstdio>
#include <map>
#include <set>
#include <tuple>
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
    1, 2, 4,  8,  4,   2,  1, 1,
    1, 2, 17, 70, 150, 33, 2, 1,
};
const int32_t BONDS[N1] = {1, 1, 2, 3, 3, 1, 1, 1};  // support [1, 4]; sites 0, 5, 6 are the exact identity
// the new true bonds w_k chi_k and their pads, restated
const int NEW_TRU[NS * N1] = {
    1, 2, 8,  24,  12,  2,  1, 1,
    1, 2, 34, 210, 450, 33, 2, 1,
};
const int NEW_PAD[NS * N1] = {
    16, 16, 16, 32,  16,  16, 16, 16,
    16, 16, 48, 224, 464, 48, 16, 16,
};

void put(std::vector<double>& t, const double re, const double im) { t.push_back(re), t.push_back(im); }
void block(std::vector<double>& t, const double a, const double b, const double c, const double d) { put(t, a, 0.5 * a), put(t, b, -b), put(t, c, 0), put(t, 0, d); }
void zero(std::vector<double>& t) { block(t, 0, 0, 0, 0); }
void ident(std::vector<double>& t) { put(t, 1, 0), put(t, 0, 0), put(t, 0, 0), put(t, 1, 0); }

std::vector<double> tensors() {
  std::vector<double> t;
  ident(t);                                    // site 0
  block(t, 1, 2, 3, 4), block(t, 5, 6, 7, 8);  // site 1: [1][2], both blocks
  // site 2: [2][3] = (0,0) (0,1) (0,2) (1,0) (1,1) (1,2); (0,1), (1,1) and (1,2) are zero: plane v = 1 has no block
  block(t, 1, 0, 0, 0), zero(t), block(t, 0, 0, 0, 2), block(t, 0, 3, 0, 0), zero(t), zero(t);
  // site 3: [3][3], the diagonal and (2, 0), with row u = 1 all zero (as -0.0): a u without a block
  for (int u = 0; u < 3; ++u)
    for (int v = 0; v < 3; ++v) {
      if (u == 1) {
        for (int q = 0; q < 8; ++q) t.push_back(-0.0);
      } else {
        (u == v || (u == 2 && v == 0)) ? block(t, u + 1, v, 0, 1) : zero(t);
      }
    }
  block(t, 1, 1, 1, 1), zero(t), block(t, 2, 2, 2, 2);  // site 4: [3][1], u = 1 zero
  ident(t), ident(t);                                   // sites 5, 6
  return t;
}

// the doubles a task writes in the re plane of its site, as the kernel's loops do (the im plane has the same pattern): count[e] += 1
void task_writes(const ApplyPlan& ap, const Task2 t, const int32_t* tru, const int32_t* w, std::vector<int>& count, const long long site_doubles) {
  const int n = ap.n_sites, st = t.x / n, k = t.x % n, u = apply_task_u(t.y), c = apply_task_chunk(t.y);
  const int l = tru[st * (n + 1) + k], r = tru[st * (n + 1) + k + 1], wl = w[k], wr = w[k + 1];
  const long long PL = ap.pad[(size_t)st * (n + 1) + k], PR = ap.pad[(size_t)st * (n + 1) + k + 1];
  CHECK(site_doubles == 2 * PL * 2 * PR);
  const int a0 = LOC_CHUNK * c, rows = std::min(LOC_CHUNK, l - a0);
  CHECK(rows >= 1 && u < wl);
  for (int a = a0; a < a0 + rows; ++a)
    for (int sp = 0; sp < 2; ++sp)
      for (long long col = 0; col < PR; ++col)  // the column blocks v r + b of every v < wr, then the padding columns from wr r on
        ++count[(size_t)((((long long)u * l + a) * 2 + sp) * PR + col)];
  CHECK((long long)wr * r <= PR);
  if (u == wl - 1 && a0 + LOC_CHUNK >= l)
    for (long long e = (long long)wl * l * 2 * PR; e < PL * 2 * PR; ++e) ++count[(size_t)e];
}

void test_tables() {
  const std::vector<double> t = tensors();
  const MpoPlan mp = mpo_plan(BONDS, t.data(), 1, N);
  const ApplyPlan ap = apply_plan(TRU, NS, N, mp);
  CHECK(ap.bad_state == -1 && ap.bad_bond == -1 && ap.n_states == NS && ap.n_sites == N);
  long long total = 0, read = 0;
  for (int s = 0; s < NS; ++s) {
    for (int k = 0; k <= N; ++k) CHECK(ap.tru[s * N1 + k] == NEW_TRU[s * N1 + k] && ap.pad[s * N1 + k] == NEW_PAD[s * N1 + k]);
    for (int k = 0; k < N; ++k) {
      CHECK(ap.offs[s * N + k] == total);
      CHECK(ap.offs[s * N + k] % 2 == 0);
      total += 2ll * NEW_PAD[s * N1 + k] * 2 * NEW_PAD[s * N1 + k + 1];
      read += 4ll * BONDS[k] * TRU[s * N1 + k] * TRU[s * N1 + k + 1];
    }
  }
  CHECK(ap.total == total && ap.read == read && ap.max_pad == 464);
  // copies
  const int want_copy[N] = {1, 0, 0, 0, 0, 1, 1};
  for (int k = 0; k < N; ++k) CHECK(ap.copy[k] == want_copy[k]);
  // row lists: per site the (u, v) of the listed blocks, by u then v
  const std::vector<std::vector<std::pair<int, int>>> want{{{0, 0}}, {{0, 0}, {0, 1}}, {{0, 0}, {0, 2}, {1, 0}}, {{0, 0}, {2, 0}, {2, 2}}, {{0, 0}, {2, 0}}, {{0, 0}}, {{0, 0}}};
  size_t at = 0;
  for (int k = 0; k < N; ++k) {
    CHECK(ap.uat[k] + BONDS[k] + 1 <= (int)ap.ufirst.size());
    CHECK(ap.ufirst[ap.uat[k]] == (int)at);
    for (const auto& uv : want[k]) {
      CHECK(at < ap.blk_u.size() && ap.blk_u[at] == uv.first && ap.blk_v[at] == uv.second);
      CHECK(ap.ufirst[ap.uat[k] + uv.first] <= (int)at && (int)at < ap.ufirst[ap.uat[k] + uv.first + 1]);
      // the coefficients are the tensor's own
      const int wr = BONDS[k + 1];
      long long toff = 0;
      for (int q = 0; q < k; ++q) toff += 8ll * BONDS[q] * BONDS[q + 1];
      for (int e = 0; e < 8; ++e) CHECK(ap.blk_w[8 * at + e] == t[(size_t)toff + 8 * ((size_t)uv.first * wr + uv.second) + e]);
      ++at;
    }
    CHECK(ap.ufirst[ap.uat[k] + BONDS[k]] == (int)at);
  }
  CHECK(at == ap.blk_u.size() && ap.blk_w.size() == 8 * at);
  // site 3, u = 1 has no block; site 2 has no block with v = 1
  CHECK(ap.ufirst[ap.uat[3] + 1] == ap.ufirst[ap.uat[3] + 2]);
  for (int j = ap.ufirst[ap.uat[2]]; j < ap.ufirst[ap.uat[2] + 2]; ++j) CHECK(ap.blk_v[j] != 1);
  std::printf("ok  tables: %lld doubles, %zu blocks\n", ap.total, at);
}

void test_tasks() {
  const std::vector<double> t = tensors();
  const MpoPlan mp = mpo_plan(BONDS, t.data(), 1, N);
  const ApplyPlan ap = apply_plan(TRU, NS, N, mp);
  std::set<std::tuple<int, int, int, int>> seen;
  for (const Task2 q : ap.tasks) {
    const int st = q.x / N, k = q.x % N, u = apply_task_u(q.y), c = apply_task_chunk(q.y);
    CHECK(st >= 0 && st < NS && u >= 0 && u < BONDS[k] && c >= 0 && c * LOC_CHUNK < TRU[st * N1 + k]);
    CHECK(seen.insert({st, k, u, c}).second);
  }
  size_t want = 0;
  for (int s = 0; s < NS; ++s)
    for (int k = 0; k < N; ++k) want += (size_t)BONDS[k] * ((TRU[s * N1 + k] + 15) / 16);
  CHECK(seen.size() == want && ap.tasks.size() == want);
  // every double of every site's re plane is written exactly once
  for (int s = 0; s < NS; ++s)
    for (int k = 0; k < N; ++k) {
      const long long plane = (long long)ap.pad[s * N1 + k] * 2 * ap.pad[s * N1 + k + 1];
      std::vector<int> count((size_t)plane, 0);
      for (const Task2 q : ap.tasks)
        if (q.x == s * N + k) task_writes(ap, q, TRU, BONDS, count, 2 * plane);
      bool once = true;
      for (const int c : count) once = once && c == 1;
      CHECK(once);
    }
  std::printf("ok  tasks: %zu\n", ap.tasks.size());
}

void test_limit_and_big() {
  // 512 exactly passes, 513 is named
  const int32_t w[4] = {1, 32, 27, 1};
  std::vector<double> t;
  for (int k = 0; k < 3; ++k)
    for (int e = 0; e < w[k] * w[k + 1]; ++e) block(t, 1, 2, 3, 4);
  const MpoPlan mp = mpo_plan(w, t.data(), 1, 3);
  const int32_t ok[2 * 4] = {1, 16, 18, 1, 1, 2, 2, 1}, bad[2 * 4] = {1, 16, 18, 1, 1, 2, 19, 1};
  const ApplyPlan a = apply_plan(ok, 2, 3, mp);
  CHECK(a.bad_state == -1 && a.tru[1] == 512 && a.pad[1] == 512 && a.tru[2] == 486 && a.pad[2] == 496 && a.max_pad == 512);
  const ApplyPlan b = apply_plan(bad, 2, 3, mp);
  CHECK(b.bad_state == 1 && b.bad_bond == 2 && b.tasks.empty() && b.offs.empty() && b.total == 0);
  const int32_t bad0[4] = {1, 17, 2, 1};
  const ApplyPlan c = apply_plan(bad0, 1, 3, mp);
  CHECK(c.bad_state == 0 && c.bad_bond == 1);
  // offsets beyond 2^31 doubles: 50 states x 60 sites of bond 256 under an MPO of bond 2 (tables only)
  constexpr int BN = 60, BS = 50;
  std::vector<int32_t> tru((size_t)BS * (BN + 1)), wb(BN + 1, 2);
  wb[0] = wb[BN] = 1;
  for (int s = 0; s < BS; ++s)
    for (int k = 0; k <= BN; ++k) tru[(size_t)s * (BN + 1) + k] = std::min({1 << std::min(k, 20), 1 << std::min(BN - k, 20), 256});
  std::vector<double> bt;
  for (int k = 0; k < BN; ++k)
    for (int e = 0; e < wb[k] * wb[k + 1]; ++e) block(bt, 1, 2, 3, 4);
  const MpoPlan bmp = mpo_plan(wb.data(), bt.data(), 1, BN);
  const ApplyPlan big = apply_plan(tru.data(), BS, BN, bmp);
  long long per_state = 0;
  for (int k = 0; k < BN; ++k) {
    const long long pl = qk_pad16(wb[k] * tru[k]), pr = qk_pad16(wb[k + 1] * tru[k + 1]);
    per_state += 2 * pl * 2 * pr;
  }
  CHECK(big.bad_state == -1 && big.max_pad == 512);
  CHECK(big.total == BS * per_state && big.total > (1ll << 31));
  for (int s = 0; s < BS; ++s) CHECK(big.offs[(size_t)s * BN] == s * per_state);
  CHECK(big.offs.back() > (1ll << 31) && big.offs.back() + 2ll * 16 * 2 * 16 == big.total);
  for (size_t e = 1; e < big.offs.size(); ++e) CHECK(big.offs[e] > big.offs[e - 1]);
  std::printf("ok  limit and 64-bit offsets: %lld doubles, %zu tasks\n", big.total, big.tasks.size());
}

}  // namespace

int main() {
  test_tables();
  test_tasks();
  test_limit_and_big();
  if (failures) std::printf("%d check(s) FAILED\n", failures);
  return failures ? 1 : 0;
}
