// The order of a step's units in the site-fused sweep (qk_unit_decode, csrc/qk_plan.h), on the CPU.  For every shape pd in {2, 4}, mt and w in
// 1..32, NW in {8, 12}, in the dual form (a column unit = a pair of column blocks) and the one-tile form:
//   * the decode over v = 0 .. units - 1 hits every unit (ta, tc, p) exactly once, for the order of the plain kernels and for the ordered one;
//   * the reciprocals of the step record equal the divisions for every argument they can meet (v / mt for v < pd mt wc, c / wc for c < pd wc),
//     and the packed word of the record (qk_unit_recips) gives every strip of a step -- the full ones and a shorter last one -- its own;
//   * the block model: units are dealt to the waves in rounds of NW consecutive indices; unit (ta, tc, p) reads the A block (ta, p) and the B
//     blocks (p, its column blocks); the distinct blocks of a round, summed over the rounds of a step, of the new order are at most those of
//     the present order (p fastest, tc slowest -- kept here as the reference formula) and strictly fewer whenever the step has more than one round;
//   * six named steps: distinct blocks, present order, new order (the last as an upper bound).
// Built with g++ and run by tests/test_unit_order.py; prints one line per check, exits 1 on a failure.
#include "../../qml-cutensornet_amd/csrc/qk_plan.h"

#include <set>
#include <tuple>
#include <vector>

namespace {

struct Shape {
  int pd, mt, w, NW;
  bool dual;
  int wc() const { return qk_unit_cols(w, dual); }
  int units() const { return pd * mt * wc(); }
};

// the present order, written out with divisions: v = pd (tc mt + ta) + p
QkUnit reference_order(const int v, const Shape& s) {
  const int u = v / s.pd;
  return QkUnit{u % s.mt, u / s.mt, v % s.pd};
}
// the new order with divisions: v = (p wc + tc) mt + ta
QkUnit new_order_by_division(const int v, const Shape& s) {
  const int c = v / s.mt;
  return QkUnit{v % s.mt, c % s.wc(), c / s.wc()};
}
bool same(const QkUnit& a, const QkUnit& b) { return a.ta == b.ta && a.tc == b.tc && a.p == b.p; }

template <typename Decode>
long blocks_over_rounds(const Shape& s, const Decode dec, int* rounds = nullptr) {
  long total = 0;
  int nr = 0;
  for (int r0 = 0; r0 < s.units(); r0 += s.NW, ++nr) {
    std::set<std::tuple<int, int, int>> blk;  // (0, ta, p) = an A block, (1, p, tb) = a B block
    for (int v = r0; v < std::min(s.units(), r0 + s.NW); ++v) {
      const QkUnit u = dec(v);
      blk.insert({0, u.ta, u.p});
      if (s.dual) {
        blk.insert({1, u.p, 2 * u.tc});
        if (2 * u.tc + 1 < s.w) blk.insert({1, u.p, 2 * u.tc + 1});  // (the last pair of an odd strip has one tile)
      } else {
        blk.insert({1, u.p, u.tc});
      }
    }
    total += (long)blk.size();
  }
  if (rounds) *rounds = nr;
  return total;
}

int report(const char* what, const long checked, const long bad) {
  std::printf("%s  %s: %ld checked, %ld bad\n", bad ? "FAIL" : "ok  ", what, checked, bad);
  return bad ? 1 : 0;
}

}  // namespace

int main() {
  int failed = 0;
  long n_dec = 0, bad_dec = 0, n_rec = 0, bad_rec = 0, n_mod = 0, bad_mod = 0, n_multi = 0;
  for (const bool dual : {true, false})
    for (const int NW : {8, 12})
      for (const int pd : {2, 4})
        for (int mt = 1; mt <= 32; ++mt)
          for (int w = 1; w <= 32; ++w) {
            const Shape s{pd, mt, w, NW, dual};
            const int ps = pd == 2 ? 1 : 2, wc = s.wc(), units = s.units();
            const int inv_mt = qk_recip20(mt), inv_wc = qk_recip15(wc);
            // every unit exactly once, both orders; the decode equals its definition by division
            std::vector<int> seen(units, 0), seen_o(units, 0);
            bool ok = true;
            for (int v = 0; v < units; ++v) {
              const QkUnit u = qk_unit_decode(v, mt, wc, inv_mt, inv_wc), o = qk_unit_decode_ordered(v, ps, mt, inv_mt);
              ok = ok && same(u, new_order_by_division(v, s)) && same(o, reference_order(v, s));
              for (const QkUnit& x : {u, o}) ok = ok && x.ta >= 0 && x.ta < mt && x.tc >= 0 && x.tc < wc && x.p >= 0 && x.p < pd;
              if (!ok) break;
              ++seen[(u.p * wc + u.tc) * mt + u.ta], ++seen_o[(o.p * wc + o.tc) * mt + o.ta];
            }
            for (int e = 0; ok && e < units; ++e) ok = seen[e] == 1 && seen_o[e] == 1;
            ++n_dec, bad_dec += !ok;
            // the reciprocals against the divisions, for every argument (and one round beyond: the look-ahead decodes v + NW)
            bool rok = true;
            for (int v = 0; v < units + NW; ++v) rok = rok && ((v * inv_mt) >> 20) == v / mt;
            for (int c = 0; c < pd * wc + NW; ++c) rok = rok && ((c * inv_wc) >> 15) == c / wc;
            ++n_rec, bad_rec += !rok;
            // the block model
            int rounds = 0;
            const long present = blocks_over_rounds(s, [&](const int v) { return reference_order(v, s); }, &rounds);
            const long now = blocks_over_rounds(s, [&](const int v) { return qk_unit_decode(v, mt, wc, inv_mt, inv_wc); });
            const bool mok = now <= present && (rounds <= 1 || now < present);
            ++n_mod, bad_mod += !mok, n_multi += rounds > 1;
            if (!mok && bad_mod <= 10) std::printf("      dual %d NW %d pd %d mt %d w %d: present %ld, new %ld, %d rounds\n", (int)dual, NW, pd, mt, w, present, now, rounds);
          }
  // the record's word: for every step of nt column blocks in strips of W, the kernels' pick (w == W) is the reciprocal of that strip's column units
  long n_word = 0, bad_word = 0;
  for (const bool dual : {true, false})
    for (int W = 1; W <= 32; ++W)
      for (int nt = W; nt <= 32; ++nt) {
        const int word = qk_unit_recips(nt, W, dual);
        bool ok = true;
        for (int s0 = 0; s0 < nt; s0 += W) {
          const int w = std::min(W, nt - s0);
          ok = ok && qk_unit_recip_of(word, w == W) == qk_recip15(qk_unit_cols(w, dual));
        }
        ++n_word, bad_word += !ok;
      }
  failed += report("every unit exactly once, decode == its definition (both orders)", n_dec, bad_dec);
  failed += report("reciprocals == divisions for every argument", n_rec, bad_rec);
  failed += report("the record's word gives every strip its reciprocal", n_word, bad_word);
  failed += report("blocks per round: new <= present, < with more than one round", n_mod, bad_mod);
  std::printf("      (%ld of the shapes have more than one round)\n", n_multi);

  struct Row {
    const char* name;
    Shape s;
    long distinct, present, bound;
  };
  const Row rows[] = {
    {"dual, 6 x 6 tiles, pd 2", {2, 6, 6, 12, true}, 24, 48, 36},
    {"dual, 8 x 8, pd 2", {2, 8, 8, 12, true}, 32, 96, 70},
    {"dual, merged step 5 x 5, pd 4", {4, 5, 5, 12, true}, 40, 108, 63},
    {"dual, merged step 6 x 6, pd 4", {4, 6, 6, 12, true}, 48, 120, 72},
    {"one-tile, 4 x 4, pd 2", {2, 4, 4, 8, false}, 16, 40, 24},
    {"one-tile, merged 3 x 3, pd 4", {4, 3, 3, 8, false}, 24, 60, 36},
  };
  for (const Row& r : rows) {
    const Shape& s = r.s;
    const int wc = s.wc();
    const long distinct = (long)s.pd * s.mt + (long)s.pd * s.w;
    const long present = blocks_over_rounds(s, [&](const int v) { return reference_order(v, s); });
    const long now = blocks_over_rounds(s, [&](const int v) { return qk_unit_decode(v, s.mt, wc, qk_recip20(s.mt), qk_recip15(wc)); });
    const bool ok = distinct == r.distinct && present == r.present && now <= r.bound;
    std::printf("%s  %s: distinct %ld, present order %ld, new order %ld (bound %ld)\n", ok ? "ok  " : "FAIL", r.name, distinct, present, now, r.bound);
    failed += !ok;
  }
  return failed ? 1 : 0;
}
