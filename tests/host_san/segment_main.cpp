// The segmentation of a pair's chain into plain and merged steps (qk_segment_chain, csrc/qk_plan.h) on the CPU.  Built with
// g++ -fsanitize=address,undefined and run by tests/test_segment_host.py; prints one line per check, exits 1 on a failure.
//   dp        chains of 1 .. 12 middle sites (edge_k 0 and 4, so n - 2 k odd and even), bond rows of x and y drawn from
//             {16, 20, 32, 40, 48, 70, 96}, both shape rules of the 12-wave launches and the 8-wave one, every mask of allowed parities: the
//             objective of the dynamic programme equals the minimum over ALL admissible segmentations (brute force), and the mask is
//             well-formed.  Chains of up to 4 sites with x = y are enumerated exhaustively, the rest is drawn at random (7^13 rows per state
//             cannot be enumerated).
//   anchor    odd starts disallowed, every admissible merge taken: the mask equals the rule the step table applied before the mask existed
//             (restated below from that table), for every pair of a random set of 40 states.
//   never_worse  the programme's objective against that rule's on the same inputs.
#include "../../qml-cutensornet_amd/csrc/qk_plan.h"

#include <cstdlib>
#include <random>
#include <vector>

namespace {

const int VALUES[7] = {16, 20, 32, 40, 48, 70, 96};
const QkSegRule RULES[3] = {{QKF_XCAP_ONE, 12, true}, {QKF_XCAP_ONE, 24, false}, {QKF_XCAP_TWO, 8, false}};  // dual, 12-wave one-tile (two slots), 8-wave

struct Row {  // a state's true and padded bonds
  std::vector<int32_t> t, d;
  void set(const std::vector<int32_t>& tr) {
    t = tr, d.resize(tr.size());
    for (size_t i = 0; i < tr.size(); ++i) d[i] = qk_pad16(tr[i]);
  }
};

long long cost_of(const Row& x, const Row& y, const int e, const bool merged) {
  return (merged ? qk_step_instr(4, x.d[e], x.d[e + 2], y.d[e], y.d[e + 2], x.t[e], y.t[e]) : qk_step_instr(2, x.d[e], x.d[e + 1], y.d[e], y.d[e + 1], x.t[e], y.t[e])) + QK_STEP_PRICE;
}

// minimum of the objective over every admissible segmentation of the sites [i, m)
long long brute(const Row& x, const Row& y, const int ek, const int m, const QkSegRule& r, const int par, const int i) {
  if (i >= m) return 0;
  long long best = cost_of(x, y, ek + i, false) + brute(x, y, ek, m, r, par, i + 1);
  if (i + 1 < m && ((par >> (i & 1)) & 1) && qk_merge_admissible(r, x.d.data(), y.d.data(), ek + i)) best = std::min(best, cost_of(x, y, ek + i, true) + brute(x, y, ek, m, r, par, i + 2));
  return best;
}

// the mask walks the chain: every site once, merges only where admissible and allowed, none past the chain; returns the objective or -1
long long walk(const Row& x, const Row& y, const int ek, const int m, const QkSegRule& r, const int par, const QkSegMask& k, int* n_steps) {
  long long obj = 0;
  std::vector<int> covered(m, 0);
  int steps = 0;
  for (int i = 0; i < m; ++steps) {
    const bool mg = qk_seg_bit(k.w[0], k.w[1], i);
    if (mg && (i + 1 >= m || !((par >> (i & 1)) & 1) || !qk_merge_admissible(r, x.d.data(), y.d.data(), ek + i))) return -1;
    obj += cost_of(x, y, ek + i, mg);
    for (int s = i; s < i + (mg ? 2 : 1); ++s) ++covered[s];
    i += mg ? 2 : 1;
  }
  for (int i = 0; i < m; ++i)
    if (covered[i] != 1) return -1;
  for (int i = 0; i < QK_SEG_BITS; ++i)  // a set bit is a merged step that is walked: not the second site of one, not beyond the chain
    if (qk_seg_bit(k.w[0], k.w[1], i) && (i + 1 >= m || (i > 0 && qk_seg_bit(k.w[0], k.w[1], i - 1)))) return -1;
  if (n_steps) *n_steps = steps;
  return obj;
}

// the rule of the step table before the mask: the fixed pairs (ek + 2 t, ek + 2 t + 1), each merged when admissible
QkSegMask old_rule(const Row& x, const Row& y, const int n, const int ek, const QkSegRule& r) {
  QkSegMask k{{0, 0}};
  const int k_hi = n - ek;
  auto one_round = [&](const int pmt, const int nt) { return r.dual ? pmt * ((nt + 1) / 2) <= r.cap : pmt * nt <= r.cap; };
  auto is_small = [&](const int a, const int a2, const int b, const int b2, const int pd) {
    return a * b <= r.xcap && a2 * b2 <= r.xcap && (one_round(pd * (a / 16), b2 / 16) || a * b + a2 * b2 <= r.xcap);
  };
  for (int t = 0; 2 * t < k_hi - ek; ++t) {
    const int e = ek + 2 * t;
    if (e + 1 >= k_hi) continue;
    const int a = x.d[e], am = x.d[e + 1], a2 = x.d[e + 2], b = y.d[e], bm = y.d[e + 1], b2 = y.d[e + 2];
    const bool sm = is_small(a, a2, b, b2, 4);
    const long long work_m = 4ll * a * b2 * (b + a2), work_p = 2ll * a * bm * (b + am) + 2ll * am * b2 * (bm + a2);
    if ((sm || (!is_small(a, am, b, bm, 2) && !is_small(am, a2, bm, b2, 2))) && work_m <= work_p && 2 * t < QK_SEG_BITS) k.w[(2 * t) >> 6] |= 1ull << ((2 * t) & 63);
  }
  return k;
}

struct Tally {
  long long checked = 0, bad = 0;
};

void check_dp(const Row& x, const Row& y, const int n, const int ek, Tally& dp, Tally& nw) {
  const int m = n - 2 * ek;
  for (const QkSegRule& r : RULES) {
    long long obj_old = 0;
    for (int par = 0; par < 4; ++par) {
      long long obj = -1;
      int steps = -1, steps_w = -2;
      const QkSegMask k = qk_segment_chain(x.d.data(), x.t.data(), y.d.data(), y.t.data(), n, ek, r, par, false, &obj, &steps);
      const long long w = walk(x, y, ek, m, r, par, k, &steps_w);
      ++dp.checked, dp.bad += !(w >= 0 && w == obj && steps == steps_w && obj == brute(x, y, ek, m, r, par, 0));
      if (par == 1) (void)qk_segment_chain(x.d.data(), x.t.data(), y.d.data(), y.t.data(), n, ek, r, 1, true, &obj_old);
      if (par == 3) ++nw.checked, nw.bad += !(obj <= obj_old);
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(12);
  auto draw = [&](const int n) {
    std::vector<int32_t> t(n + 1);
    for (auto& v : t) v = VALUES[rng() % 7];
    return t;
  };
  Tally dp, nw, anchor;
  Row x, y;
  // (1) exhaustive: x = y, chains of 1 .. 4 sites, edge_k = 0
  for (int m = 1; m <= 4; ++m) {
    std::vector<int32_t> t(m + 1);
    long long combos = 1;
    for (int i = 0; i <= m; ++i) combos *= 7;
    for (long long c = 0; c < combos; ++c) {
      long long v = c;
      for (int i = 0; i <= m; ++i) t[i] = VALUES[v % 7], v /= 7;
      x.set(t), y.set(t);
      check_dp(x, y, m, 0, dp, nw);
    }
  }
  // ... and drawn at random: 1 .. 12 middle sites, edge_k 0 and 4 (the sites of the edges carry bonds too: the function must not read them as chain)
  for (int m = 1; m <= 12; ++m)
    for (const int ek : {0, 4})
      for (int rep = 0; rep < 1500; ++rep) {
        const int n = m + 2 * ek;
        x.set(draw(n)), y.set(draw(n));
        if (rep % 3 == 0) y = x;
        check_dp(x, y, n, ek, dp, nw);
      }
  std::printf("%s  dp: %lld checked, %lld bad\n", dp.bad ? "FAIL" : "ok  ", dp.checked, dp.bad);
  std::printf("%s  never_worse: %lld checked, %lld bad\n", nw.bad ? "FAIL" : "ok  ", nw.checked, nw.bad);
  // (2) the anchor of QK_MERGE=1: every pair of 40 random states, chains with n - 2 k odd and even, k = 0 and 4, a chain of 2 middle sites
  for (const int n : {20, 21, 10, 2}) {
    std::vector<Row> set(40);
    for (Row& s : set) {  // bonds that wander: a walk over the values, so that level stretches (merges) and dips both occur
      std::vector<int32_t> t(n + 1);
      int v = (int)(rng() % 7);
      for (auto& b : t) v = std::min(6, std::max(0, v + (int)(rng() % 3) - 1)), b = VALUES[v];
      s.set(t);
    }
    for (const int ek : {0, 4}) {
      if (n - 2 * ek < 2) continue;
      for (const QkSegRule& r : RULES)
        for (const Row& a : set)
          for (const Row& b : set) {
            const QkSegMask k = qk_segment_chain(a.d.data(), a.t.data(), b.d.data(), b.t.data(), n, ek, r, 1, true), o = old_rule(a, b, n, ek, r);
            ++anchor.checked, anchor.bad += !(k.w[0] == o.w[0] && k.w[1] == o.w[1]);
          }
    }
  }
  std::printf("%s  anchor: %lld checked, %lld bad\n", anchor.bad ? "FAIL" : "ok  ", anchor.checked, anchor.bad);
  return dp.bad || nw.bad || anchor.bad ? 1 : 0;
}
