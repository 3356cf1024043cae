// The host-side plan of the block kernels (csrc/qk_local_plan.h: the BLK_* kinds) on hand-made x and y sets over 7 sites whose
// bonds differ: the geometry of a step for both sides, the pair-chain task counts over rectangular (pad_x, pad_y) blocks, the slot
// regions (V and W inside T), the launches of a width list that skips cuts, the offsets of the kept-cut buffer, and the cut into
// several pair batches with the task lists of a batch that does not start at pair 0.  Every expected value is restated here from
// the definitions, not taken from the header.  Built with g++ -fsanitize=address,undefined and run by tests/test_block_plan.py;
// prints one line per section, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <cstdio>
#include <vector>

using namespace qkl;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr int N = 7, N1 = N + 1, NX = 3, NY = 2;
const int32_t XTRU[NX * N1] = {
    1, 2, 4,  8,  4,   2,  1, 1,
    1, 2, 17, 80, 150, 33, 2, 1,
    1, 2, 4,  65, 64,  4,  2, 1,
};
const int XPAD[NX * N1] = {
    16, 16, 16, 16, 16,  16, 16, 16,
    16, 16, 32, 80, 160, 48, 16, 16,
    16, 16, 16, 80, 64,  16, 16, 16,
};
const int32_t YTRU[NY * N1] = {
    1, 2, 3, 5,  70, 9,  2, 1,
    1, 2, 4, 33, 16, 20, 2, 1,
};
const int YPAD[NY * N1] = {
    16, 16, 16, 16, 80, 16, 16, 16,
    16, 16, 16, 48, 16, 32, 16, 16,
};
const int XPMAX[NX] = {16, 160, 80}, YPMAX[NY] = {80, 48};
constexpr int XMAXPAD = 160, YMAXPAD = 80;

long long b64(const long long m, const long long n) { return ((m + 63) / 64) * ((n + 63) / 64); }

EnvSizes sizes(const int32_t* tru, const int ns, const int max_pad) {
  EnvSizes z;
  env_sizes(tru, ns, N, max_pad, LOC_RMUL, true, z);
  return z;
}

// the bonds a step enters and leaves by, and its site, restated: the left chain walks sites 0, 1, ..; the right chain walks the
// reversed image, sites n-1, n-2, ..
void geometry(const int side, const int j, int& site, int& in, int& out) {
  if (side == 0) site = j, in = j, out = j + 1;
  else site = N - 1 - j, in = N - j, out = N - 1 - j;
}

long long expected_tasks(const int kind, const int side, const int j, const int* px, const int* py) {
  int site, in, out;
  geometry(side, j, site, in, out);
  if (kind == BLK_T) return b64(px[in], 2 * py[out]);   // T [pad x_in][2 pad y_out]
  if (kind == BLK_X) return b64(py[out], px[out]);      // E' [pad y_out][pad x_out]
  if (kind == BLK_V) return b64(py[out], px[out]);      // V  [pad y_out][pad x_out]
  if (kind == BLK_W) return b64(px[out], px[out]);      // W  [pad x_out][pad x_out]
  return px[out] / 16;                                  // 16-row chunks of W
}

void test_geometry() {
  for (int side = 0; side < 2; ++side)
    for (int j = 0; j < N; ++j) {
      int site, in, out;
      geometry(side, j, site, in, out);
      CHECK(blk_site(side, j, N) == site && blk_in(side, j, N) == in && blk_out(side, j, N) == out);
      CHECK(blk_cut_bond(side, j + 1, N) == out);  // after step j the chain stands at the cut of width j + 1
      if (j) CHECK(blk_in(side, j, N) == blk_out(side, j - 1, N));
    }
  CHECK(blk_cut_bond(0, 1, N) == 1 && blk_cut_bond(0, N, N) == N && blk_cut_bond(1, 1, N) == N - 1 && blk_cut_bond(1, N, N) == 0);
  CHECK(conj_b(BLK_X) && conj_b(BLK_W) && !conj_b(BLK_T) && !conj_b(BLK_V));
  CHECK(BLK_T >= 0 && BLK_X >= 0 && BLK_V >= 0 && BLK_W >= 0 && BLK_RED < 0);
  const int kinds[] = {LOC_REV_T, LOC_REV_X, LOC_FWD_T, LOC_FWD_W, LOC_PAIR_T, LOC_PAIR_V, LOC_DIST_T, LOC_DIST_X, LOC_BOND_M, STR_T, STR_X, LOC_RHO, LOC_PAIR_RHO,
                       LOC_DIST_RHO, LOC_ADMIT, LOC_BOND_TR, STR_LNEXT, STR_PAULI, STR_CLOSE};
  for (const int k : kinds) CHECK(k != BLK_T && k != BLK_X && k != BLK_V && k != BLK_W && k != BLK_RED);
  std::printf("ok  geometry\n");
}

void test_task_counts() {
  const int kinds[] = {BLK_T, BLK_X, BLK_V, BLK_W, BLK_RED};
  long long rect = 0;
  for (int side = 0; side < 2; ++side)
    for (int i = 0; i < NX; ++i)
      for (int jy = 0; jy < NY; ++jy)
        for (int j = 0; j < N; ++j)
          for (const int kind : kinds) {
            const long long want = expected_tasks(kind, side, j, XPAD + i * N1, YPAD + jy * N1);
            CHECK(blk_task_count(kind, side, j, XPAD + i * N1, YPAD + jy * N1, N) == want);
            CHECK(want >= 1);
            int site, in, out;
            geometry(side, j, site, in, out);
            rect += XPAD[i * N1 + out] != YPAD[jy * N1 + out];
          }
  CHECK(rect > 0);  // the cases do have unequal pad_x and pad_y
  // spelled out: x state 1 against y state 0, left, step 3 (bond 3 -> 4): x 80 -> 160, y 16 -> 80
  CHECK(blk_task_count(BLK_T, 0, 3, XPAD + N1, YPAD, N) == 2 * 3);   // 80 x 160
  CHECK(blk_task_count(BLK_X, 0, 3, XPAD + N1, YPAD, N) == 2 * 3);   // 80 x 160
  CHECK(blk_task_count(BLK_V, 0, 3, XPAD + N1, YPAD, N) == 2 * 3);
  CHECK(blk_task_count(BLK_W, 0, 3, XPAD + N1, YPAD, N) == 3 * 3);   // 160 x 160
  CHECK(blk_task_count(BLK_RED, 0, 3, XPAD + N1, YPAD, N) == 10);
  // the same pair from the right, step 2 (bond 5 -> 4): x 48 -> 160, y 16 -> 80
  CHECK(blk_task_count(BLK_T, 1, 2, XPAD + N1, YPAD, N) == 1 * 3);   // 48 x 160
  CHECK(blk_task_count(BLK_W, 1, 2, XPAD + N1, YPAD, N) == 9);
  std::printf("ok  task counts\n");
}

void test_slot() {
  // a slot is 6 P^2 doubles: E = planes [0, 1), [1, 2); T = planes of 2 P^2 at [2, 4), [4, 6).  V and W are re | im planes of
  // P^2 inside T and apart from each other and from E.
  CHECK(chain_E() == 0 && chain_T() == 2 && chain_size() == 6);
  CHECK(blk_V() >= chain_T() && blk_V() + 2 <= chain_size());
  CHECK(blk_W() >= chain_T() && blk_W() + 2 <= chain_size());
  CHECK(blk_V() + 2 <= blk_W() || blk_W() + 2 <= blk_V());
  CHECK(blk_V() >= chain_E() + 2 && blk_W() >= chain_E() + 2);
  // every matrix of a pair fits its region for P = max(P_x, P_y)
  for (int i = 0; i < NX; ++i)
    for (int jy = 0; jy < NY; ++jy) {
      const long long P = std::max(XPMAX[i], YPMAX[jy]), P2 = P * P;
      for (int k = 0; k <= N; ++k) {
        const long long ax = XPAD[i * N1 + k], by = YPAD[jy * N1 + k];
        CHECK(by * ax <= P2 && ax * ax <= P2);           // E, V; W
        if (k < N) CHECK(ax * 2 * YPAD[jy * N1 + k + 1] <= 2 * P2 && XPAD[i * N1 + k + 1] * 2 * by <= 2 * P2);  // T of either side
      }
    }
  std::printf("ok  slot regions\n");
}

void test_plan_of_widths() {
  const int32_t widths[3] = {2, 3, 6};  // skips 1, 4, 5 and stops before 7
  const std::vector<BlkLaunch> plan = blk_plan(3, widths);
  CHECK(plan.size() == 2 * 6 + 3 * 3);
  size_t at = 0;
  int ci = 0;
  for (int j = 0; j < 6; ++j) {
    CHECK(plan[at].kind == BLK_T && plan[at].step == j && plan[at].cut == -1);
    ++at;
    CHECK(plan[at].kind == BLK_X && plan[at].step == j && plan[at].cut == -1);
    ++at;
    if (j + 1 == 2 || j + 1 == 3 || j + 1 == 6) {
      for (const int kind : {BLK_V, BLK_W, BLK_RED}) {
        CHECK(plan[at].kind == kind && plan[at].step == j && plan[at].cut == ci);
        ++at;
      }
      ++ci;
    }
  }
  CHECK(at == plan.size() && ci == 3);
  const int32_t all[N] = {1, 2, 3, 4, 5, 6, 7};
  CHECK(blk_plan(N, all).size() == 2 * N + 3 * N);
  const int32_t one[1] = {1};
  CHECK(blk_plan(1, one).size() == 5);
  CHECK(blk_bad_width(3, widths, N) == -1 && blk_bad_width(N, all, N) == -1);
  const int32_t b0[2] = {0, 2}, b1[2] = {2, 2}, b2[2] = {3, 1}, b3[2] = {1, 8};
  CHECK(blk_bad_width(2, b0, N) == 0 && blk_bad_width(2, b1, N) == 1 && blk_bad_width(2, b2, N) == 1 && blk_bad_width(2, b3, N) == 1);
  std::printf("ok  launches of a width list\n");
}

void test_kept_offsets() {
  const EnvSizes zx = sizes(XTRU, NX, XMAXPAD), zy = sizes(YTRU, NY, YMAXPAD);
  const int32_t widths[3] = {2, 3, 6};
  for (int side = 0; side < 2; ++side) {
    std::vector<int64_t> kx, ky;
    CHECK(blk_kept_unit() == 512);
    const long long mid = blk_kept_offsets(zx, side, 3, widths, blk_kept_unit(), kx);
    const long long end = blk_kept_offsets(zy, side, 3, widths, mid, ky);
    CHECK(kx.size() == 3 * NX && ky.size() == 3 * NY);
    long long at = 512;  // behind the unit matrix: state-major, in width order, both planes of pad x pad
    for (int s = 0; s < NX; ++s)
      for (int ci = 0; ci < 3; ++ci) {
        const int bond = side ? N - widths[ci] : widths[ci];
        CHECK(kx[s * 3 + ci] == at);
        at += 2ll * XPAD[s * N1 + bond] * XPAD[s * N1 + bond];
      }
    CHECK(at == mid);
    for (int s = 0; s < NY; ++s)
      for (int ci = 0; ci < 3; ++ci) {
        const int bond = side ? N - widths[ci] : widths[ci];
        CHECK(ky[s * 3 + ci] == at);
        at += 2ll * YPAD[s * N1 + bond] * YPAD[s * N1 + bond];
      }
    CHECK(at == end);
  }
  // left, x state 1: bonds 2, 3, 6 pad to 32, 80, 16
  std::vector<int64_t> kx;
  blk_kept_offsets(zx, 0, 3, widths, blk_kept_unit(), kx);
  CHECK(kx[3] == 512 + 3 * 512 && kx[4] == kx[3] + 2 * 32 * 32 && kx[5] == kx[4] + 2 * 80 * 80 && kx[6] == kx[5] + 512);
  std::printf("ok  kept-cut buffer\n");
}

void test_pair_batches() {
  const EnvSizes zx = sizes(XTRU, NX, XMAXPAD), zy = sizes(YTRU, NY, YMAXPAD);
  const int32_t widths[3] = {2, 3, 6};
  const std::vector<BlkLaunch> plan = blk_plan(3, widths);
  // every pair, y-major, and one of them twice
  std::vector<int32_t> pairs;
  for (int jy = 0; jy < NY; ++jy)
    for (int i = 0; i < NX; ++i) pairs.push_back(i), pairs.push_back(jy);
  pairs.push_back(1), pairs.push_back(0);
  const long long np = (long long)pairs.size() / 2;
  for (int side = 0; side < 2; ++side) {
    const BlkChains c = list_blk_chains(zx, zy, np, pairs.data(), side, plan, 3);
    CHECK((long long)c.slot.size() == np && (long long)c.weight.size() == np);
    const int max_chunks = XMAXPAD / 16;
    for (long long e = 0; e < np; ++e) {
      const int i = pairs[2 * e], jy = pairs[2 * e + 1];
      const long long P = std::max(XPMAX[i], YPMAX[jy]);
      long long nt = 0;
      for (const BlkLaunch& l : plan) nt += expected_tasks(l.kind, side, l.step, XPAD + i * N1, YPAD + jy * N1);
      CHECK(c.slot[e] == 6 * P * P && c.ntasks[e] == nt);
      CHECK(c.weight[e] == 6 * P * P + 3 * max_chunks + nt + 4);
    }
    CHECK(c.weight[1] == c.weight[np - 1] && c.ntasks[1] == c.ntasks[np - 1]);  // the pair listed twice
    // a cap of 3 chains: batches [0,3) [3,6) [6,7)
    const std::vector<size_t> cap3 = chain_cut(c.weight, 1ll << 60, 3);
    CHECK(cap3 == (std::vector<size_t>{0, 3, 6, 7}));
    // room for the two largest neighbours only: every batch holds what fits, at least one chain, in order, nothing lost
    const long long room = c.weight[1] + c.weight[2];
    const std::vector<size_t> cut = chain_cut(c.weight, room, 0);
    CHECK(cut.front() == 0 && cut.back() == (size_t)np && cut.size() > 3);
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
      CHECK(cut[b] < cut[b + 1]);
      long long acc = 0;
      for (size_t e = cut[b]; e < cut[b + 1]; ++e) acc += c.weight[e];
      CHECK(acc <= room || cut[b + 1] - cut[b] == 1);
      if (cut[b + 1] < (size_t)np) CHECK(acc + c.weight[cut[b + 1]] > room);
    }
    // the task lists of the batch [3, 6): chains are numbered from 0 inside the batch, launch by launch in plan order
    std::vector<Task2> tasks;
    std::vector<long long> first;
    blk_lists(zx, zy, pairs.data(), 3, 3, side, plan, tasks, first);
    CHECK(first.size() == plan.size() + 1 && first.front() == 0 && first.back() == (long long)tasks.size());
    long long total = 0;
    for (size_t li = 0; li < plan.size(); ++li) {
      long long at = first[li];
      for (int e = 0; e < 3; ++e) {
        const int i = pairs[2 * (3 + e)], jy = pairs[2 * (3 + e) + 1];
        const long long cnt = expected_tasks(plan[li].kind, side, plan[li].step, XPAD + i * N1, YPAD + jy * N1);
        for (long long b = 0; b < cnt; ++b, ++at) CHECK(at < first[li + 1] && tasks[at].x == e && tasks[at].y == b);
      }
      CHECK(at == first[li + 1]);
      total += first[li + 1] - first[li];
    }
    CHECK(total == c.ntasks[3] + c.ntasks[4] + c.ntasks[5]);
  }
  std::printf("ok  pair batches\n");
}

}  // namespace

int main() {
  test_geometry();
  test_task_counts();
  test_slot();
  test_plan_of_widths();
  test_kept_offsets();
  test_pair_batches();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
