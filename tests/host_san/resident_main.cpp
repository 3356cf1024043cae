// The residency of X in a step of the site-fused sweep (qk_resident, qk_rec_resident; csrc/qk_plan.h), on the CPU.  Exhaustive over the
// padded bonds a, a', b, b' in 16 .. 256 in steps of 16, pd in {2, 4}, X at the low and at the top end of the buffer, for the launch
// shapes (segmentation buffer, residency buffer, round): 12-wave dual 8192 / large, 12-wave one-tile 8192 / large, 8-wave 4608 / 4608, and
// the 12-wave shapes with the large buffer switched off:
//   * inside:   X' (wherever the step keeps it whole in LDS) and every panel of X that phase 1 reads from LDS lie inside the buffer;
//   * apart:    in a side-by-side or partially resident step X' and the panels that stay never overlap, and of a partially resident step
//               the panel next to the ones that stay does overlap X' (the rule keeps as many as fit);
//   * side:     a step whose X and X' fit the buffer side by side keeps every panel and evicts nothing;
//   * parent:   with the residency buffer set to the segmentation buffer and partial residency off the rule is the classification the kernels
//               had before it: LDS-resident <=> qk_seg_small, X' at the other end <=> small and side by side, else X' at 0, a step that is not
//               LDS-resident reads no panel from LDS;
//   * strips:   a step whose X or X' does not fit the segmentation buffer keeps nothing and builds X' at 0, whatever the residency buffer;
//   * record:   the step table's word (qk_step_record) decodes to the same answer for both ends (qk_rec_resident).
//   * choice:   qk_choose_sweep gives the 12-wave launches the large buffer (QkSweepRun.big, lds_launch) exactly when their tables fit the room
//               behind it and QK_FUSED_BIG is not 0 -- a long chain and the DET form of wide bonds fall back --, never the 8-wave launch,
//               and leaves every other field of the choice as it is without the large buffer.
// Built with -fsanitize=address,undefined and run by tests/test_resident_host.py; prints one line per check, exits 1 on a failure.
#include "../../qml-cutensornet_amd/csrc/qk_plan.h"

#include <vector>

namespace {

int report(const char* what, const long checked, const long bad) {
  std::printf("%s  %s: %ld checked, %ld bad\n", bad ? "FAIL" : "ok  ", what, checked, bad);
  return bad ? 1 : 0;
}

struct Shape {
  QkSegRule rule;
  const char* name;
};

}  // namespace

int main() {
  static_assert(QKF_RCAP_ONE >= QKF_XCAP_ONE && QKF_RCAP_ONE % (QK_TILE * QK_TILE) == 0, "the large buffer holds whole blocks and at least the segmentation's buffer");
  const std::vector<Shape> shapes = {
      {{QKF_XCAP_ONE, 12, true, QKF_RCAP_ONE, true}, "12-wave dual, large buffer"},
      {{QKF_XCAP_ONE, 24, false, QKF_RCAP_ONE, true}, "12-wave one-tile, large buffer"},
      {{QKF_XCAP_ONE, 12, true, QKF_XCAP_ONE, true}, "12-wave dual, fallback"},
      {{QKF_XCAP_ONE, 24, false, QKF_XCAP_ONE, true}, "12-wave one-tile, fallback"},
      {{QKF_XCAP_TWO, 8, false, QKF_XCAP_TWO, true}, "8-wave"},
  };
  long n = 0, bad_inside = 0, bad_apart = 0, bad_side = 0, bad_parent = 0, bad_strips = 0, bad_record = 0;
  long kinds[4] = {0, 0, 0, 0}, part_one = 0, part_all_but_one = 0, part_none = 0;
  for (const Shape& sh : shapes) {
    const QkSegRule& r = sh.rule;
    const int rcap = qk_res_cap(r);
    QkSegRule parent = r;  // the same shape as the kernels classified it before the rule
    parent.rcap = 0, parent.partial = false;
    for (int pd = 2; pd <= 4; pd += 2)
      for (int a = 16; a <= 256; a += 16)
        for (int a2 = 16; a2 <= 256; a2 += 16)
          for (int b = 16; b <= 256; b += 16)
            for (int b2 = 16; b2 <= 256; b2 += 16) {
              const int n_in = a * b, n_out = a2 * b2, mt = a / QK_TILE, panel = b * QK_TILE;
              const bool small = qk_seg_small(r, a, a2, b, b2, pd), fits = n_in <= r.xcap && n_out <= r.xcap;
              const int32_t xd[3] = {a, a2, a2}, yd[3] = {b, b2, b2};  // (a plain step reads entries 0 and 1, a merged one 0 and 2)
              const QkStepRec rec = qk_step_record(xd, xd, yd, yd, 0, pd / 2, 0, false, r, false);
              for (int top = 0; top < 2; ++top) {
                if (top && n_in > r.xcap) continue;  // (an X that does not fit the segmentation's buffer never sits in LDS)
                ++n;
                const int xb = top ? rcap - n_in : 0;
                const QkResident s = qk_resident(r, a, a2, b, b2, pd, top != 0);
                const QkResident p = qk_resident(parent, a, a2, b, b2, pd, top != 0);
                if (!top) ++kinds[s.kind];
                bool inside = s.klo >= 0 && s.klo <= s.khi && s.khi <= mt && s.ob >= 0 && s.ob % (QK_TILE * QK_TILE) == 0;
                if (n_out <= r.xcap) inside = inside && s.ob + n_out <= rcap;
                if (s.khi > s.klo) inside = inside && n_in <= r.xcap && xb >= 0 && xb + s.khi * panel <= rcap;
                bool apart = true;
                const int k0 = xb + s.klo * panel, k1 = xb + s.khi * panel;  // the elements of the panels that stay
                if (s.kind == QK_RES_SIDE || s.kind == QK_RES_PART) {
                  apart = fits && (s.khi == s.klo || k1 <= s.ob || k0 >= s.ob + n_out) && s.ob == (top ? 0 : rcap - n_out);
                  apart = apart && (top ? s.khi == mt : s.klo == 0);  // the panels at the far end from X' stay
                }
                if (s.kind == QK_RES_PART) {
                  apart = apart && !small && r.partial && s.khi - s.klo < mt;
                  // the next panel towards X' does not fit beside it
                  if (top) apart = apart && xb + (s.klo - 1) * panel < s.ob + n_out;
                  else apart = apart && xb + (s.khi + 1) * panel > s.ob;
                  if (!top) part_one += s.khi - s.klo == 1, part_all_but_one += s.khi - s.klo == mt - 1, part_none += s.khi == s.klo;
                }
                if (s.kind == QK_RES_INPLACE) apart = apart && small && s.ob == 0 && s.klo == 0 && s.khi == mt && qk_seg_one_round(r, pd * mt, b2 / QK_TILE);
                const bool together = fits && n_in + n_out <= rcap;
                const bool side = together == (s.kind == QK_RES_SIDE) && (!together || (s.klo == 0 && s.khi == mt));
                // the classification of the kernels before the rule (qk_fused.h of the parent: small, pingpong, ob)
                const bool small_p = qk_seg_small(parent, a, a2, b, b2, pd), pingpong_p = small_p && n_in + n_out <= r.xcap;
                const int xb_p = top ? r.xcap - n_in : 0, ob_p = !small_p ? 0 : pingpong_p ? (xb_p == 0 ? r.xcap - n_out : 0) : 0;
                bool par = (p.kind == QK_RES_SIDE) == pingpong_p && (p.kind == QK_RES_INPLACE) == (small_p && !pingpong_p) && (p.kind == QK_RES_NONE) == !small_p && p.kind != QK_RES_PART;
                par = par && p.ob == ob_p && (small_p ? (p.klo == 0 && p.khi == mt) : p.khi == p.klo);
                par = par && small == small_p && ((rec.w[7] & QK_REC_SMALL) != 0) == small_p;  // the larger buffer does not change what the table calls LDS-resident
                const bool strips = fits || (s.kind == QK_RES_NONE && s.ob == 0 && s.khi == s.klo);
                const QkResident d = qk_rec_resident(rec.w[7], mt, n_out, rcap, top != 0);
                bool record = d.kind == s.kind && d.ob == s.ob && d.klo == s.klo && d.khi == s.khi;
                for (int ta = 0; ta < mt; ++ta) record = record && (((qk_res_global_mask(d) >> ta) & 1u) != 0) == (ta < s.klo || ta >= s.khi);  // (the kernels' word)
                bad_inside += !inside, bad_apart += !apart, bad_side += !side, bad_parent += !par, bad_strips += !strips, bad_record += !record;
                if (!(inside && apart && side && par && strips && record))
                  std::printf("      %s: pd %d a %d a' %d b %d b' %d top %d -> kind %d ob %d panels [%d, %d): inside %d apart %d side %d parent %d strips %d record %d\n", sh.name, pd, a, a2, b, b2, top,
                              s.kind, s.ob, s.klo, s.khi, (int)inside, (int)apart, (int)side, (int)par, (int)strips, (int)record);
              }
            }
  }
  // ---- the choice of the instantiation (256 CUs; sets of 60 sites and bonds 128 unless said otherwise)
  long n_choice = 0, bad_choice = 0;
  {
    struct Want {
      const char* name;
      int sites, pad;
      bool det, dual, big_ok, two_wg, split;
      int kernel;
      bool big0, big1;  // of the first and of the second launch
    };
    const Want wants[] = {
        {"dual", 60, 128, false, true, true, false, false, QK_KERNEL_FUSED_DUAL, true, false},
        {"dual, QK_FUSED_BIG=0", 60, 128, false, true, false, false, false, QK_KERNEL_FUSED_DUAL, false, false},
        {"one-tile", 60, 128, false, false, true, false, false, QK_KERNEL_FUSED1, true, false},
        {"dual, 119 sites", 119, 128, false, true, true, false, false, QK_KERNEL_FUSED_DUAL, true, false},  // 272 + 119 * 64 = 7888 <= 8192
        {"dual, 130 sites: tables too long", 130, 128, false, true, true, false, false, QK_KERNEL_FUSED_DUAL, false, false},
        {"DET dual, bonds 128", 60, 128, true, true, true, false, false, QK_KERNEL_FUSED_DUAL_DET, true, false},
        {"DET dual, bonds 512: turn counters too long", 60, 512, true, true, true, false, false, QK_KERNEL_FUSED_DUAL_DET, false, false},
        {"8-wave", 60, 128, false, true, true, true, false, QK_KERNEL_FUSED2, false, false},
        {"split: dual large, 8-wave not", 60, 256, false, true, true, false, true, QK_KERNEL_FUSED_DUAL, true, false},
    };
    for (const Want& w : wants) {
      ++n_choice;
      QkSweepPolicy pol;
      pol.deterministic = w.det, pol.fused_dual = w.dual, pol.fused_big = w.big_ok, pol.fused_wgs = w.two_wg ? 2 : 0;
      qk_plan plan;
      plan.pairs.assign(2 * 125250, 0);
      plan.n_first = w.split ? 60000 : 125250, plan.nq = 16, plan.fit_two = 0.5, plan.fit_narrow = 1.0;
      const QkSetShape set{w.pad, 64, w.sites};
      const QkSweepChoice ch = qk_choose_sweep(pol, plan, set, set, 256);
      QkSweepPolicy off = pol;
      off.fused_big = false;
      const QkSweepChoice ch0 = qk_choose_sweep(off, plan, set, set, 256);
      bool ok = ch.rc == QK_OK && ch.n_runs == (w.split ? 2 : 1) && ch.run[0].kernel == w.kernel && ch.run[0].big == w.big0 && ch.run[1].big == w.big1 && ch0.n_runs == ch.n_runs;
      for (int i = 0; ok && i < ch.n_runs; ++i) {
        const QkSweepRun &r = ch.run[i], &r0 = ch0.run[i];
        const size_t meta = r.lds - (size_t)(r.kernel == QK_KERNEL_FUSED2 || r.kernel == QK_KERNEL_FUSED2_DET ? QKF_XCAP_TWO : QKF_XCAP_ONE) * 16;
        ok = r.lds_launch == (r.big ? (size_t)QKF_RCAP_ONE * 16 + meta : r.lds) && r.lds_launch <= (size_t)QKF_LDS_BYTES && (!r.big || meta <= (size_t)QKF_META_ROOM);
        ok = ok && !r0.big && r0.lds_launch == r0.lds && r0.kernel == r.kernel && r0.grid == r.grid && r0.lds == r.lds && r0.first == r.first && r0.count == r.count;
      }
      ok = ok && ch0.scratch_bytes == ch.scratch_bytes && ch0.launched_grid == ch.launched_grid;
      bad_choice += !ok;
      if (!ok) std::printf("      choice %s: kernel %d big %d %d lds %zu -> %zu\n", w.name, ch.run[0].kernel, (int)ch.run[0].big, (int)ch.run[1].big, ch.run[0].lds, ch.run[0].lds_launch);
    }
  }
  int failed = 0;
  failed += report("choice: the large buffer where the tables fit behind it", n_choice, bad_choice);
  failed += report("inside: X' and the panels read from LDS lie in the buffer", n, bad_inside);
  failed += report("apart: X' and the panels that stay never overlap, as many stay as fit", n, bad_apart);
  failed += report("side: side-by-side steps keep every panel", n, bad_side);
  failed += report("parent: segmentation buffer and no partial residency give the former classification", n, bad_parent);
  failed += report("strips: a step that does not fit keeps nothing", n, bad_strips);
  failed += report("record: the step table's word decodes to the rule", n, bad_record);
  std::printf("      (X low: %ld strip or evicted-whole, %ld side by side, %ld partial, %ld in place; partial steps that keep one panel %ld, all but one %ld, none %ld)\n", kinds[QK_RES_NONE],
              kinds[QK_RES_SIDE], kinds[QK_RES_PART], kinds[QK_RES_INPLACE], part_one, part_all_but_one, part_none);
  if (!(kinds[QK_RES_PART] > 0 && kinds[QK_RES_SIDE] > 0 && kinds[QK_RES_INPLACE] > 0 && kinds[QK_RES_NONE] > 0 && part_one > 0 && part_all_but_one > 0 && part_none > 0)) failed += report("every kind occurs", 1, 1);
  return failed ? 1 : 0;
}
