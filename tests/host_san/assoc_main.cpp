// The association of the steps of a pair's chain (qk_segment_chain with assoc, csrc/qk_plan.h) on the CPU.  Built with
// g++ -fsanitize=address,undefined and run by tests/test_assoc_host.py; prints one line per check, exits 1 on a failure.
//   dp        chains of 1 .. 10 middle sites (edge_k 0 and 3), bond rows of x and y drawn from {16, 20, 32, 40, 48, 70, 96, 128}, the shape
//             rules of the 12-wave dual launch, the 12-wave one-tile launch and the 8-wave one, switch prices 0, 40 and 150: the masks walk
//             the chain (every site once, merges admissible in the orientation at hand, a switch only behind an LDS-resident step, the
//             second site of a merged step repeats its bit, nothing beyond bit m), the objective, the steps and the switches the function
//             reports are those of the walk, and (objective, switches, steps in orientation 1, steps) is the lexicographic minimum over
//             ALL segmentations with orientations (brute force) -- the ties as specified: fewer switches, then orientation 0.
//   assoc0    assoc = 0 gives the masks of the segmentation as it was before the orientations existed (restated below), bit for bit, an
//             empty orientation mask and the same objective, for every mask of allowed parities.
//   symmetric x = y: both orientations cost the same, so the chain stays in orientation 0 with no switch.
//   pattern   assoc = 2 and 3: the walk is well-formed, starts in orientation 0 / 1 and switches behind EVERY step that may switch.
//   long      a chain that leaves no room for bit m keeps orientation 0.
//   record    the step-table record of an orientation-1 step is the orientation-0 record of the exchanged pair (but for its flag).
//   3m        the two 3M forms of phase 2 on random complex numbers: the switch step's (conj(t) a) and the one-sum form of the ordinary
//             step (t conj(a)).
#include "../../qml-cutensornet_amd/csrc/qk_plan.h"

#include <cmath>
#include <complex>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

const int VALUES[8] = {16, 20, 32, 40, 48, 70, 96, 128};
const QkSegRule RULES[3] = {{QKF_XCAP_ONE, 12, true}, {QKF_XCAP_ONE, 24, false}, {QKF_XCAP_TWO, 8, false}};  // dual, 12-wave one-tile (two slots), 8-wave

struct Row {  // a state's true and padded bonds
  std::vector<int32_t> t, d;
  void set(const std::vector<int32_t>& tr) {
    t = tr, d.resize(tr.size());
    for (size_t i = 0; i < tr.size(); ++i) d[i] = qk_pad16(tr[i]);
  }
};

struct Tup {  // what the programme minimises, in this order
  long long c;
  int sw, n1, st;
};
bool less(const Tup& a, const Tup& b) { return a.c != b.c ? a.c < b.c : a.sw != b.sw ? a.sw < b.sw : a.n1 != b.n1 ? a.n1 < b.n1 : a.st < b.st; }
bool same(const Tup& a, const Tup& b) { return a.c == b.c && a.sw == b.sw && a.n1 == b.n1 && a.st == b.st; }

// the step of `len` sites at site e in orientation o: the states exchanged in orientation 1
long long cost_of(const Row& x, const Row& y, const int e, const int len, const int o) {
  const Row &p = o ? y : x, &r = o ? x : y;
  return qk_step_instr(2 * len, p.d[e], p.d[e + len], r.d[e], r.d[e + len], p.t[e], r.t[e]) + QK_STEP_PRICE;
}
bool small_of(const Row& x, const Row& y, const int e, const int len, const int o, const QkSegRule& r) {
  const Row &p = o ? y : x, &s = o ? x : y;
  return qk_seg_small(r, p.d[e], p.d[e + len], s.d[e], s.d[e + len], 2 * len);
}
bool may_merge(const Row& x, const Row& y, const int ek, const int m, const int i, const int o, const QkSegRule& r, const int par) {
  return i + 1 < m && ((par >> (i & 1)) & 1) && qk_merge_admissible(r, (o ? y : x).d.data(), (o ? x : y).d.data(), ek + i);
}

// the lexicographic minimum over every segmentation with orientations of the sites [i, m), the step at i in orientation o
Tup brute(const Row& x, const Row& y, const int ek, const int m, const QkSegRule& r, const int par, const int price, const int i, const int o) {
  if (i >= m) return Tup{0, 0, 0, 0};
  Tup best{-1, 0, 0, 0};
  for (int len = 1; len <= 2; ++len) {
    if (len == 2 && !may_merge(x, y, ek, m, i, o, r, par)) continue;
    const long long c = cost_of(x, y, ek + i, len, o);
    for (int sw = 0; sw < 2; ++sw) {
      if (sw && !small_of(x, y, ek + i, len, o, r)) continue;
      const Tup rest = brute(x, y, ek, m, r, par, price, i + len, o ^ sw);
      const Tup t{c + (sw ? price : 0) + rest.c, rest.sw + sw, rest.n1 + o, rest.st + 1};
      if (best.c < 0 || less(t, best)) best = t;
    }
  }
  return best;
}

// the two masks walk the chain; returns false on a malformed pair of masks
bool walk(const Row& x, const Row& y, const int ek, const int m, const QkSegRule& r, const int par, const int price, const QkSegMask& k, const QkSegMask& ori, Tup* out, bool* every_switch) {
  Tup t{0, 0, 0, 0};
  bool every = true;
  auto bit = [](const QkSegMask& q, const int i) { return qk_seg_bit(q.w[0], q.w[1], i); };
  for (int i = 0; i < m;) {
    const bool mg = bit(k, i);
    const int o = bit(ori, i) ? 1 : 0, len = mg ? 2 : 1;
    if (mg && !may_merge(x, y, ek, m, i, o, r, par)) return false;
    if (mg && (bit(k, i + 1) || bit(ori, i + 1) != bit(ori, i))) return false;  // the second site: no step of its own, its step's orientation
    const bool sw = bit(ori, i + len) != bit(ori, i), can = small_of(x, y, ek + i, len, o, r);
    if (sw && !can) return false;  // a switch only behind an LDS-resident step
    if (can && !sw) every = false;
    t.c += cost_of(x, y, ek + i, len, o) + (sw ? price : 0), t.sw += sw, t.n1 += o, t.st += 1;
    i += len;
  }
  for (int i = m; i < QK_SEG_BITS; ++i)
    if (bit(k, i) || (i > m && bit(ori, i))) return false;
  if (m > 0 && bit(k, m - 1)) return false;
  *out = t;
  if (every_switch) *every_switch = every;
  return true;
}

// the segmentation as it was before the orientations existed (the dynamic programme and the greedy rule of the parent, restated)
QkSegMask old_chain(const Row& x, const Row& y, const int n_sites, const int ek, const QkSegRule& rule, const int parities, const bool greedy, long long* objective) {
  const int m = n_sites - 2 * ek;
  const int32_t *xd = x.d.data(), *yd = y.d.data(), *xt = x.t.data(), *yt = y.t.data();
  auto may = [&](const int i) { return i + 1 < m && i < QK_SEG_BITS && ((parities >> (i & 1)) & 1) != 0 && qk_merge_admissible(rule, xd, yd, ek + i); };
  auto plain_cost = [&](const int i) { return qk_step_instr(2, xd[ek + i], xd[ek + i + 1], yd[ek + i], yd[ek + i + 1], xt[ek + i], yt[ek + i]) + QK_STEP_PRICE; };
  auto merged_cost = [&](const int i) { return qk_step_instr(4, xd[ek + i], xd[ek + i + 2], yd[ek + i], yd[ek + i + 2], xt[ek + i], yt[ek + i]) + QK_STEP_PRICE; };
  QkSegMask take{{0ull, 0ull}};
  if (greedy) {
    for (int i = 0; i < m && i < QK_SEG_BITS; ++i)
      if (may(i)) take.w[i >> 6] |= 1ull << (i & 63);
  } else {
    long long c1 = 0, c2 = 0;
    int s1 = 0, s2 = 0;
    for (int i = m - 1; i >= 0; --i) {
      long long c = plain_cost(i) + c1;
      int s = s1 + 1;
      if (may(i)) {
        const long long cm = merged_cost(i) + c2;
        const int sm = s2 + 1;
        if (cm < c || (cm == c && (sm < s || (sm == s && (i & 1) == 0)))) c = cm, s = sm, take.w[i >> 6] |= 1ull << (i & 63);
      }
      c2 = c1, s2 = s1, c1 = c, s1 = s;
    }
  }
  QkSegMask out{{0ull, 0ull}};
  long long obj = 0;
  for (int i = 0; i < m;) {
    if (qk_seg_bit(take.w[0], take.w[1], i)) out.w[i >> 6] |= 1ull << (i & 63), obj += merged_cost(i), i += 2;
    else obj += plain_cost(i), i += 1;
  }
  *objective = obj;
  return out;
}

std::vector<int32_t> draw(std::mt19937& g, const int n1) {
  std::vector<int32_t> r(n1);
  for (int i = 0; i < n1; ++i) r[i] = VALUES[g() % 8];
  return r;
}

}  // namespace

int main() {
  std::mt19937 gen(20260919);
  int bad_total = 0;
  {  // dp, pattern, assoc0
    long long n_dp = 0, bad_dp = 0, n_pat = 0, bad_pat = 0, n_a0 = 0, bad_a0 = 0, with_switch = 0, start1 = 0;
    for (int ek : {0, 3}) {
      for (int m = 1; m <= 10; ++m) {
        const int n = m + 2 * ek;
        for (int rep = 0; rep < 60; ++rep) {
          Row x, y;
          x.set(draw(gen, n + 1)), y.set(draw(gen, n + 1));
          for (const QkSegRule& r : RULES) {
            for (int price : {0, 40, 150}) {
              long long obj = -1;
              int st = -1, sw = -1;
              QkSegMask ori{{~0ull, ~0ull}};
              const QkSegMask k = qk_segment_chain(x.d.data(), x.t.data(), y.d.data(), y.t.data(), n, ek, r, 3, false, &obj, &st, 1, price, &ori, &sw);
              Tup w{};
              const bool ok = walk(x, y, ek, m, r, 3, price, k, ori, &w, nullptr);
              const Tup b0 = brute(x, y, ek, m, r, 3, price, 0, 0), b1 = brute(x, y, ek, m, r, 3, price, 0, 1), b = less(b1, b0) ? b1 : b0;
              ++n_dp;
              if (!ok || w.c != obj || w.st != st || w.sw != sw || !same(w, b)) {
                if (++bad_dp <= 5) std::printf("FAIL dp: m %d ek %d price %d: walk ok %d, objective %lld / walk %lld / brute %lld, switches %d / %d / %d\n", m, ek, price, (int)ok, obj, w.c, b.c, sw, w.sw, b.sw);
              }
              with_switch += sw > 0, start1 += (int)qk_seg_bit(ori.w[0], ori.w[1], 0);
            }
            for (int mode : {2, 3}) {
              long long obj = -1;
              int st = -1, sw = -1;
              QkSegMask ori{{~0ull, ~0ull}};
              const QkSegMask k = qk_segment_chain(x.d.data(), x.t.data(), y.d.data(), y.t.data(), n, ek, r, 3, false, &obj, &st, mode, 40, &ori, &sw);
              Tup w{};
              bool every = false;
              const bool ok = walk(x, y, ek, m, r, 3, 40, k, ori, &w, &every);
              ++n_pat;
              if (!ok || !every || w.c != obj || w.st != st || w.sw != sw || qk_seg_bit(ori.w[0], ori.w[1], 0) != (mode == 3)) {
                if (++bad_pat <= 5) std::printf("FAIL pattern: m %d ek %d mode %d: walk ok %d, every %d\n", m, ek, mode, (int)ok, (int)every);
              }
            }
            for (int par = 0; par < 4; ++par)
              for (int greedy = 0; greedy < 2; ++greedy) {
                long long obj = -1, obj_old = -2;
                QkSegMask ori{{~0ull, ~0ull}};
                int sw = -1;
                const QkSegMask k = qk_segment_chain(x.d.data(), x.t.data(), y.d.data(), y.t.data(), n, ek, r, par, greedy != 0, &obj, nullptr, greedy ? 1 : 0, 40, &ori, &sw);  // (the greedy rule ignores assoc)
                const QkSegMask o = old_chain(x, y, n, ek, r, par, greedy != 0, &obj_old);
                ++n_a0;
                if (k.w[0] != o.w[0] || k.w[1] != o.w[1] || ori.w[0] != 0 || ori.w[1] != 0 || sw != 0 || obj != obj_old) {
                  if (++bad_a0 <= 5) std::printf("FAIL assoc0: m %d ek %d par %d greedy %d\n", m, ek, par, greedy);
                }
              }
          }
        }
      }
    }
    std::printf("%s dp: %lld checked, %lld bad (%lld chains switch, %lld start in orientation 1)\n", bad_dp ? "FAIL" : "ok  ", n_dp, bad_dp, with_switch, start1);
    std::printf("%s pattern: %lld checked, %lld bad\n", bad_pat ? "FAIL" : "ok  ", n_pat, bad_pat);
    std::printf("%s assoc0: %lld checked, %lld bad\n", bad_a0 ? "FAIL" : "ok  ", n_a0, bad_a0);
    if (with_switch == 0 || start1 == 0) std::printf("FAIL dp: the drawn rows never switch or never start in orientation 1\n"), ++bad_total;
    bad_total += (int)(bad_dp + bad_pat + bad_a0);
  }
  {  // symmetric: x = y
    long long n_sym = 0, bad_sym = 0;
    for (int m = 1; m <= 10; ++m)
      for (int rep = 0; rep < 40; ++rep) {
        Row x;
        x.set(draw(gen, m + 1));
        for (const QkSegRule& r : RULES)
          for (int price : {0, 40}) {
            QkSegMask ori{{~0ull, ~0ull}};
            int sw = -1;
            long long obj = 0, obj0 = 0;
            const QkSegMask k = qk_segment_chain(x.d.data(), x.t.data(), x.d.data(), x.t.data(), m, 0, r, 3, false, &obj, nullptr, 1, price, &ori, &sw);
            const QkSegMask k0 = qk_segment_chain(x.d.data(), x.t.data(), x.d.data(), x.t.data(), m, 0, r, 3, false, &obj0);
            ++n_sym;
            if (sw != 0 || ori.w[0] != 0 || ori.w[1] != 0 || k.w[0] != k0.w[0] || k.w[1] != k0.w[1] || obj != obj0) ++bad_sym;
          }
      }
    std::printf("%s symmetric: %lld checked, %lld bad\n", bad_sym ? "FAIL" : "ok  ", n_sym, bad_sym);
    bad_total += (int)bad_sym;
  }
  {  // long: m + 1 > QK_SEG_BITS
    long long n_long = 0, bad_long = 0;
    for (int m : {QK_SEG_BITS - 1, QK_SEG_BITS, QK_SEG_BITS + 5}) {
      Row x, y;
      x.set(draw(gen, m + 1)), y.set(draw(gen, m + 1));
      for (int mode = 1; mode <= 3; ++mode) {
        QkSegMask ori{{~0ull, ~0ull}};
        int sw = -1;
        long long obj = 0, obj0 = 0;
        const QkSegMask k = qk_segment_chain(x.d.data(), x.t.data(), y.d.data(), y.t.data(), m, 0, RULES[0], 3, false, &obj, nullptr, mode, 40, &ori, &sw);
        const QkSegMask k0 = qk_segment_chain(x.d.data(), x.t.data(), y.d.data(), y.t.data(), m, 0, RULES[0], 3, false, &obj0);
        ++n_long;
        const bool room = m + 1 <= QK_SEG_BITS;
        if (!room && (sw != 0 || ori.w[0] != 0 || ori.w[1] != 0 || k.w[0] != k0.w[0] || k.w[1] != k0.w[1] || obj != obj0)) ++bad_long;
        if (room && mode == 1 && obj > obj0) ++bad_long;
      }
    }
    std::printf("%s long: %lld checked, %lld bad\n", bad_long ? "FAIL" : "ok  ", n_long, bad_long);
    bad_total += (int)bad_long;
  }
  {  // record
    long long n_rec = 0, bad_rec = 0;
    for (int rep = 0; rep < 400; ++rep) {
      Row x, y;
      x.set(draw(gen, 4)), y.set(draw(gen, 4));
      for (const QkSegRule& r : RULES)
        for (int len = 1; len <= 2; ++len)
          for (int sw = 0; sw < 2; ++sw)
            for (int recips = 0; recips < 2; ++recips) {
              const QkStepRec a = qk_step_record(x.d.data(), x.t.data(), y.d.data(), y.t.data(), 1, len, 1, sw != 0, r, recips != 0);
              const QkStepRec b = qk_step_record(y.d.data(), y.t.data(), x.d.data(), x.t.data(), 1, len, 0, sw != 0, r, recips != 0);
              ++n_rec;
              bool eq = true;
              for (int w = 0; w < 12; ++w) eq = eq && a.w[w] == (w == 7 ? (b.w[w] | QK_REC_ORIENT) : b.w[w]);
              // and the record against its definition
              const int A = y.d[1], A2 = y.d[1 + len], B = x.d[1], B2 = x.d[1 + len];
              eq = eq && a.w[0] == A && a.w[1] == A2 && a.w[2] == B && a.w[3] == B2 && a.w[4] == y.t[1] && a.w[5] == (x.t[1] + 3) / 4 && a.w[9] == len && a.w[10] == 1 + len;
              eq = eq && ((a.w[7] & QK_REC_SMALL) != 0) == qk_seg_small(r, A, A2, B, B2, 2 * len) && ((a.w[7] & QK_REC_SWITCH) != 0) == (sw != 0);
              if (!eq) ++bad_rec;
            }
    }
    std::printf("%s record: %lld checked, %lld bad\n", bad_rec ? "FAIL" : "ok  ", n_rec, bad_rec);
    bad_total += (int)bad_rec;
  }
  {  // 3m: sums over four k-steps, as a block of phase 2 forms them
    long long n_3m = 0, bad_3m = 0;
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int rep = 0; rep < 20000; ++rep) {
      double tr[4], ti[4], ar[4], ai[4];
      std::complex<double> sw_ref = 0, or_ref = 0;
      double scale = 0;
      for (int i = 0; i < 4; ++i) {
        tr[i] = u(gen), ti[i] = u(gen), ar[i] = u(gen), ai[i] = u(gen);
        const std::complex<double> t(tr[i], ti[i]), a(ar[i], ai[i]);
        sw_ref += std::conj(t) * a, or_ref += t * std::conj(a), scale += std::abs(t) * std::abs(a);
      }
      // the switch step: k1 = sum tr (Ar + Ai), re = k1 + sum (ti - tr) Ai, im = k1 + sum (-tr - ti) Ar
      double k1 = 0, re = 0, im = 0;
      for (int i = 0; i < 4; ++i) k1 += tr[i] * (ar[i] + ai[i]);
      re = im = k1;
      for (int i = 0; i < 4; ++i) re += (ti[i] - tr[i]) * ai[i], im += (-tr[i] - ti[i]) * ar[i];
      // the ordinary step with one operand sum: k1 = sum tr (Ar - Ai), re = k1 + sum (tr + ti) Ai, im = k1 + sum (ti - tr) Ar
      double k2 = 0, re2 = 0, im2 = 0;
      for (int i = 0; i < 4; ++i) k2 += tr[i] * (ar[i] - ai[i]);
      re2 = im2 = k2;
      for (int i = 0; i < 4; ++i) re2 += (tr[i] + ti[i]) * ai[i], im2 += (ti[i] - tr[i]) * ar[i];
      ++n_3m;
      const double tol = 16 * 2.3e-16 * scale;  // a dozen roundings of terms of this size
      if (std::abs(std::complex<double>(re, im) - sw_ref) > tol || std::abs(std::complex<double>(re2, im2) - or_ref) > tol) ++bad_3m;
    }
    std::printf("%s 3m: %lld checked, %lld bad\n", bad_3m ? "FAIL" : "ok  ", n_3m, bad_3m);
    bad_total += (int)bad_3m;
  }
  return bad_total ? 1 : 0;
}
