// The host-side plan of the k-qubit windows (csrc/qk_local_plan.h: the WIN_* kinds) on a hand-made set over 8 sites with ragged
// bonds: the regions of a chain's slot against what the launches of every step read and write (no block of a launch reads what
// another block of it writes, nothing leaves the slot), the pair index of the closing sums, the task counts against the
// definitions, every output block of every launch listed exactly once -- also for a chain batch that does not start at chain 0 and
// for stacked widths that are no multiple of 64 -- the same work whatever the cut into chain batches, and the checks of width and
// starts.  Every expected value is restated here from the definitions, not taken from the header.  Built with
// g++ -fsanitize=address,undefined and run by tests/test_window_plan.py; prints one line per section, exits 1 on a mismatch.
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

constexpr int N = 8, N1 = N + 1, NS = 3;
const int32_t TRU[NS * N1] = {
    1, 2, 4,  8,  16, 8,  4,  2, 1,
    1, 2, 4,  17, 70, 33, 20, 2, 1,
    1, 2, 3,  50, 64, 65, 4,  2, 1,
};
const int PAD[NS * N1] = {
    16, 16, 16, 16, 16, 16, 16, 16, 16,
    16, 16, 16, 32, 80, 48, 32, 16, 16,
    16, 16, 16, 64, 64, 80, 16, 16, 16,
};
const int PMAX[NS] = {16, 80, 80};
constexpr int MAXPAD = 80;

long long b64(const long long m, const long long n) { return ((m + 63) / 64) * ((n + 63) / 64); }

EnvSizes sizes() {
  EnvSizes z;
  env_sizes(TRU, NS, N, MAXPAD, LOC_RMUL, true, z);
  return z;
}

// the buffers of a slot: G_j in buffer j & 1, Gr_j in buffer 2 + (j & 1), H in the G buffer that G_w does not lie in; two planes of
// U = 2^w P^2 each, eight planes in all
void test_slot() {
  CHECK(win_size() == 8);
  for (int w = 1; w <= WIN_MAX_WIDTH; ++w) {
    CHECK(win_dim(w) == (1 << w));
    for (int j = 0; j <= w; ++j) {
      CHECK(win_G(j) == 2 * (j % 2) && win_Gr(j) == 4 + 2 * (j % 2));
      CHECK(win_G(j) + 2 <= 4 && win_Gr(j) >= 4 && win_Gr(j) + 2 <= win_size());
      if (j < w) CHECK(win_G(j) != win_G(j + 1) && win_Gr(j) != win_Gr(j + 1));  // a step reads one parity and writes the other
    }
    CHECK(win_H(w) != win_G(w) && win_H(w) == win_G(w - 1) && win_H(w) + 2 <= 4);  // H takes the place of the dead G_{w-1}
    CHECK(win_H(w) != win_Gr(w));
    CHECK(win_unit(80, w) == 80ll * 80 * (1 << w));
    // the largest element every launch touches lies inside a plane, for every state and window of the set
    for (int s = 0; s < NS; ++s)
      for (int a = 0; a + w <= N; ++a) {
        const int* p = PAD + s * N1;
        const long long U = win_unit(PMAX[s], w), pb = p[a + w];
        for (int j = 0; j < w; ++j) {
          const long long rows = p[a + w - 1 - j], ld = 2 * (pb << j);  // G_{j+1}: pad_c rows of 2^(j+1) pad_b
          CHECK((rows - 1) * ld + ld - 1 < U);
        }
        CHECK((long long)(p[a] - 1) * (pb << w) + (pb << w) - 1 < U);  // H and the operands of the closing sum
      }
  }
  std::printf("ok  slot\n");
}

void test_pairs() {
  for (int w = 1; w <= WIN_MAX_WIDTH; ++w) {
    const int D = 1 << w;
    CHECK(win_pairs(w) == D * (D + 1) / 2 && win_vals(w) == D * (D + 1));
    int p = 0;
    for (int s = 0; s < D; ++s)
      for (int sp = s; sp < D; ++sp, ++p) {
        CHECK(win_pair(s, sp, w) == p);
        int s2 = -1, sp2 = -1;
        win_pair_of(p, w, s2, sp2);
        CHECK(s2 == s && sp2 == sp);
      }
    CHECK(p == win_pairs(w));
  }
  CHECK(WIN_CLOSE_GROUP == 16);
  std::printf("ok  pairs\n");
}

void test_plan_and_counts() {
  for (int w = 1; w <= WIN_MAX_WIDTH; ++w) {
    const Plan plan = win_plan(w);
    CHECK((int)plan.size() == w + 2);
    for (int j = 0; j < w; ++j) CHECK(plan[j].first == WIN_G && plan[j].second == j);
    CHECK(plan[w].first == WIN_H && plan[w + 1].first == WIN_CLOSE);
    for (int s = 0; s < NS; ++s)
      for (int a = 0; a + w <= N; ++a) {
        const int32_t* p = PAD + s * N1;
        const int b = a + w;
        for (int j = 0; j < w; ++j) {
          const long long per = b64(p[b - 1 - j], (long long)p[b] << j);
          CHECK(win_step_blocks(j, p, a, w) == per);
          CHECK(win_task_count(WIN_G, j, p, a, w) == (j == 0 ? 2 : 4) * per);  // step 0 grows Gr alone: G_1 is the site itself
        }
        CHECK(win_task_count(WIN_H, 0, p, a, w) == b64(p[a], (long long)p[b] << w));
        CHECK(win_task_count(WIN_CLOSE, 0, p, a, w) == p[a] / 16);
      }
  }
  CHECK(!conj_b(WIN_G) && !conj_b(WIN_H) && WIN_G >= 0 && WIN_H >= 0 && WIN_CLOSE < 0);
  std::printf("ok  plan and counts\n");
}

// every output block of every launch exactly once: decode (chain, block) of a WIN_G task into (seed, t, row block, column block)
void check_lists(const EnvSizes& z, const int s0, const WinChains& c, const size_t c0, const size_t nc, const int w, const int32_t* starts,
                 std::map<std::tuple<int, int, int, int>, int>& seen /* (global chain, launch, block, 0) -> count */) {
  std::vector<Task2> tasks;
  std::vector<long long> first;
  win_lists(z, s0, c, c0, nc, w, starts, tasks, first);
  const Plan plan = win_plan(w);
  CHECK(first.size() == plan.size() + 1 && first.front() == 0 && first.back() == (long long)tasks.size());
  for (size_t li = 0; li < plan.size(); ++li) {
    CHECK(first[li] <= first[li + 1]);
    std::set<std::tuple<int, int, int, int, int>> outputs;  // (chain, seed, t, m block, n block): no two tasks write the same block
    for (long long t = first[li]; t < first[li + 1]; ++t) {
      const Task2 tk = tasks[t];
      CHECK(tk.x >= 0 && tk.x < (int)nc);
      const size_t e = c0 + tk.x;
      const int32_t* p = PAD + (s0 + c.cent[e]) * N1;
      const int a = starts[c.cwin[e]], b = a + w;
      ++seen[{(int)e, (int)li, tk.y, 0}];
      if (plan[li].first == WIN_G) {
        const int j = plan[li].second, M = p[b - 1 - j];
        const long long Nn = (long long)p[b] << j;
        const int npm = (M + 63) / 64, npn = (int)((Nn + 63) / 64), per = npm * npn;
        const int q = tk.y / per, blk = tk.y % per;
        CHECK(q < (j == 0 ? 2 : 4));
        CHECK(64 * (blk % npm) < M && 64ll * (blk / npm) < Nn);
        CHECK(outputs.insert({tk.x, q >> 1, q & 1, blk % npm, blk / npm}).second);
      } else if (plan[li].first == WIN_H) {
        const int M = p[a];
        const long long Nn = (long long)p[b] << w;
        const int npm = (M + 63) / 64;
        CHECK(64 * (tk.y % npm) < M && 64ll * (tk.y / npm) < Nn);
        CHECK(outputs.insert({tk.x, 0, 0, tk.y % npm, tk.y / npm}).second);
      } else {
        CHECK(tk.y < p[a] / 16);
        CHECK(outputs.insert({tk.x, 0, 0, tk.y, 0}).second);
      }
    }
  }
}

void test_lists_and_cuts() {
  const EnvSizes z = sizes();
  const int32_t some[] = {0, 2, 3, 5};
  for (int w = 1; w <= WIN_MAX_WIDTH; ++w) {
    std::vector<int32_t> all;
    for (int a = 0; a + w <= N; ++a) all.push_back(a);
    std::vector<int32_t> sub;
    for (const int32_t a : some)
      if (a + w <= N) sub.push_back(a);
    for (const std::vector<int32_t>& starts : {all, sub}) {
      const int nw = (int)starts.size(), s0 = 1, nb = 2;  // the state batch of states 1 and 2: a batch other than the first
      const WinChains c = list_win_chains(z, s0, nb, w, nw, starts.data());
      CHECK((int)c.cent.size() == nb * nw);
      long long want_total = 0;
      for (int i = 0; i < nb; ++i)
        for (int m = 0; m < nw; ++m) {
          const size_t e = (size_t)i * nw + m;
          CHECK(c.cent[e] == i && c.cwin[e] == m);
          CHECK(c.slot[e] == 8ll * PMAX[s0 + i] * PMAX[s0 + i] * (1 << w));
          long long nt = 0;
          const int32_t* p = PAD + (s0 + i) * N1;
          const int a = starts[m], b = a + w;
          for (int j = 0; j < w; ++j) nt += (j == 0 ? 2 : 4) * b64(p[b - 1 - j], (long long)p[b] << j);
          nt += b64(p[a], (long long)p[b] << w) + p[a] / 16;
          CHECK(c.ntasks[e] == nt);
          CHECK(c.weight[e] >= c.slot[e] + (long long)(MAXPAD / 16) * (1 << w) * ((1 << w) + 1) + nt);  // slot, partial sums, tasks
          want_total += nt;
        }
      // the same work whatever the cut: every (chain, launch, block) exactly once, for several caps and a room that forces cuts
      for (const long long cap : {0ll, 1ll, 3ll, 5ll, 1000ll}) {
        for (const long long room : {1ll << 60, 3 * c.weight[0] + 1}) {
          const std::vector<size_t> cut = chain_cut(c.weight, room, cap);
          CHECK(cut.front() == 0 && cut.back() == c.weight.size());
          std::map<std::tuple<int, int, int, int>, int> seen;
          for (size_t cb = 0; cb + 1 < cut.size(); ++cb) {
            CHECK(cut[cb] < cut[cb + 1]);
            if (cap > 0) CHECK((long long)(cut[cb + 1] - cut[cb]) <= cap);
            long long acc = 0;
            for (size_t e = cut[cb]; e < cut[cb + 1]; ++e) acc += c.weight[e];
            CHECK(cut[cb + 1] - cut[cb] == 1 || acc <= room);
            check_lists(z, s0, c, cut[cb], cut[cb + 1] - cut[cb], w, starts.data(), seen);
          }
          CHECK((long long)seen.size() == want_total);
          for (const auto& kv : seen) CHECK(kv.second == 1);
        }
      }
    }
  }
  std::printf("ok  lists and cuts\n");
}

void test_arguments() {
  for (int n = 1; n <= 9; ++n)
    for (int w = -1; w <= 8; ++w) CHECK(win_bad_width(w, n) == !(w >= 1 && w <= n && w <= 6));
  const int32_t ok[] = {0, 1, 4, 6};
  CHECK(win_bad_start(4, ok, 8, 2) == -1);
  CHECK(win_bad_start(4, ok, 8, 3) == 3);           // 6 > n - w = 5
  const int32_t neg[] = {-1, 2};
  CHECK(win_bad_start(2, neg, 8, 2) == 0);
  const int32_t rep[] = {0, 3, 3};
  CHECK(win_bad_start(3, rep, 8, 2) == 2);          // not strictly increasing
  const int32_t down[] = {4, 2};
  CHECK(win_bad_start(2, down, 8, 2) == 1);
  const int32_t last[] = {6};
  CHECK(win_bad_start(1, last, 8, 2) == -1 && win_bad_start(1, last, 7, 2) == 0);
  const int32_t zero[] = {0};
  CHECK(win_bad_start(1, zero, 6, 6) == -1);
  std::printf("ok  arguments\n");
}

}  // namespace

int main() {
  test_slot();
  test_pairs();
  test_plan_and_counts();
  test_lists_and_cuts();
  test_arguments();
  if (failures) std::printf("%d FAILED\n", failures);
  return failures ? 1 : 0;
}
