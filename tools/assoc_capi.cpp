// A C entry to the segmentation of the site-fused sweep WITH the association of its steps (qk_segment_chain with assoc, csrc/qk_plan.h)
// for tools/merge_potential.py and the tests: the same function the device runs, compiled for the host (g++ -O2 -shared -fPIC) and
// called through ctypes.  Not part of the product.  (tools/segment_capi.cpp is the entry without orientations.)
#include "../qml-cutensornet_amd/csrc/qk_plan.h"

// x_true / y_true: [states][n_sites + 1] true bonds; pairs: [n_pairs][2] = (x state, y state).  Per pair: four words (the merges, the
// orientations -- what qk_segment_kernel stores), the matrix instructions of its steps, the steps, the switches, and flags: bit 0 = the
// chain starts in orientation 1, bit 1 = it ends in orientation 1, bit 2 = its FIRST step switches, bit 3 = its LAST step switches, bit 4 =
// a merged step switches, bit 5 = a step that is not LDS-resident (a strip step) lies between two switches, bit 6 = a step whose X and X'
// do not fit the buffer side by side (one round, in place) switches, bit 7 = a step with X and X' side by side (ping-pong) switches.
extern "C" void qk_assoc_pairs(const int32_t* x_true, const int32_t* y_true, int32_t n_sites, const int32_t* pairs, int64_t n_pairs, int32_t ek, int32_t xcap, int32_t cap, int32_t dual,
                               int32_t assoc, int32_t switch_price, uint64_t* masks, int64_t* instr, int32_t* steps, int32_t* switches, int32_t* flags) {
  const QkSegRule rule{xcap, cap, dual != 0};
  const int n1 = n_sites + 1, m = n_sites - 2 * ek;
  std::vector<int32_t> xd(n1), yd(n1);
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t* xt = x_true + (int64_t)pairs[2 * p] * n1;
    const int32_t* yt = y_true + (int64_t)pairs[2 * p + 1] * n1;
    for (int i = 0; i < n1; ++i) xd[i] = qk_pad16(xt[i]), yd[i] = qk_pad16(yt[i]);
    long long obj = 0;
    int st = 0, sw = 0;
    QkSegMask o{{0ull, 0ull}};
    const QkSegMask k = qk_segment_chain(xd.data(), xt, yd.data(), yt, n_sites, ek, rule, 3, false, &obj, &st, assoc, switch_price, &o, &sw);
    masks[4 * p] = k.w[0], masks[4 * p + 1] = k.w[1], masks[4 * p + 2] = o.w[0], masks[4 * p + 3] = o.w[1];
    instr[p] = obj - (long long)st * QK_STEP_PRICE - (long long)sw * switch_price, steps[p] = st, switches[p] = sw;
    int f = (qk_seg_bit(o.w[0], o.w[1], 0) ? 1 : 0) | (qk_seg_bit(o.w[0], o.w[1], m) ? 2 : 0), seen = 0, strip_since = 0;
    for (int i = 0; i < m;) {
      const int len = qk_seg_bit(k.w[0], k.w[1], i) ? 2 : 1, e = ek + i;
      const bool o1 = qk_seg_bit(o.w[0], o.w[1], i), s = qk_seg_bit(o.w[0], o.w[1], i + len) != o1;
      const int a = o1 ? yd[e] : xd[e], a2 = o1 ? yd[e + len] : xd[e + len], b = o1 ? xd[e] : yd[e], b2 = o1 ? xd[e + len] : yd[e + len];
      if (!qk_seg_small(rule, a, a2, b, b2, 2 * len) && seen) strip_since = 1;
      if (s) {
        f |= (i == 0 ? 4 : 0) | (i + len >= m ? 8 : 0) | (len == 2 ? 16 : 0) | (strip_since ? 32 : 0) | (a * b + a2 * b2 <= rule.xcap ? 128 : 64);
        seen = 1, strip_since = 0;
      }
      i += len;
    }
    flags[p] = f;
  }
}

// What the column blocks of phase 2 (csrc/qk_fused.h: qkf_p2_onesum) meet on the chains of the same pairs: per pair two words of case
// bits -- [0] of its ordinary steps, [1] of its switch steps -- and the blocks its ordinary and its switch steps run (a block = one column
// block tn of one unit: a pair of tiles in the dual shape, one tile otherwise; strips are counted as one strip).  Case bits of a step with
// nn column blocks of a', nt tiles of b', true bond `at` of a and physical dimension pd:
//   bit 0 nn = 1, bit 1 nn = 2, bit 2 nn odd >= 3, bit 3 nn even >= 4;  bits 4 .. 7: the last block of rows of a has 1, 2, 3, 4 k-steps;
//   bit 8 a unit with a single tile (dual shape: nt odd), bit 9 a unit with a pair of tiles (nt >= 2);  bit 10 a plain step (pd = 2), bit 11 a
//   merged step (pd = 4);  bit 12 a strip step (not LDS-resident).
extern "C" void qk_onesum_pairs(const int32_t* x_true, const int32_t* y_true, int32_t n_sites, const int32_t* pairs, int64_t n_pairs, int32_t ek, int32_t xcap, int32_t cap, int32_t dual,
                                int32_t assoc, int32_t switch_price, int32_t* cases, int64_t* blocks) {
  const QkSegRule rule{xcap, cap, dual != 0};
  const int n1 = n_sites + 1, m = n_sites - 2 * ek;
  std::vector<int32_t> xd(n1), yd(n1);
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t* xt = x_true + (int64_t)pairs[2 * p] * n1;
    const int32_t* yt = y_true + (int64_t)pairs[2 * p + 1] * n1;
    for (int i = 0; i < n1; ++i) xd[i] = qk_pad16(xt[i]), yd[i] = qk_pad16(yt[i]);
    long long obj = 0;
    int st = 0, sw = 0;
    QkSegMask o{{0ull, 0ull}};
    const QkSegMask k = qk_segment_chain(xd.data(), xt, yd.data(), yt, n_sites, ek, rule, 3, false, &obj, &st, assoc, switch_price, &o, &sw);
    cases[2 * p] = cases[2 * p + 1] = 0, blocks[2 * p] = blocks[2 * p + 1] = 0;
    for (int i = 0; i < m;) {
      const int len = qk_seg_bit(k.w[0], k.w[1], i) ? 2 : 1, e = ek + i;
      const bool o1 = qk_seg_bit(o.w[0], o.w[1], i), s = qk_seg_bit(o.w[0], o.w[1], i + len) != o1;
      const int a = o1 ? yd[e] : xd[e], a2 = o1 ? yd[e + len] : xd[e + len], b = o1 ? xd[e] : yd[e], b2 = o1 ? xd[e + len] : yd[e + len];
      const int at = o1 ? yt[e] : xt[e];
      const int nn = a2 / 16, nt = b2 / 16, mt = a / 16, pd = 2 * len;
      const int klast = (at - (mt - 1) * 16 + 3) >> 2;  // k-steps of the last block of rows of a: 1 .. 4
      int c = (nn == 1 ? 1 : nn == 2 ? 2 : (nn & 1) ? 4 : 8) | (16 << (klast - 1)) | (pd == 4 ? 2048 : 1024);
      if (dual != 0) c |= ((nt & 1) ? 256 : 0) | (nt >= 2 ? 512 : 0);
      else c |= 256;
      if (!qk_seg_small(rule, a, a2, b, b2, pd)) c |= 4096;
      cases[2 * p + (s ? 1 : 0)] |= c;
      blocks[2 * p + (s ? 1 : 0)] += (long long)pd * mt * (dual != 0 ? (nt + 1) / 2 : nt) * nn;
      i += len;
    }
  }
}

// The residency of X (csrc/qk_plan.h: qk_resident) along the chains of the same pairs, walked the way the kernels walk them: X behind the
// left edge at element 0, behind a step at the end where that step built X' (or in the global buffer when X' left the LDS in strips).
// rcap / partial: the elements the residency may use and whether a step may keep part of X (QkSegRule); parities: 3 = merged steps chosen by
// the dynamic programme (QK_MERGE=2), 0 = every site a step of its own in orientation 0 (QK_MERGE=0).  Per pair one word of case bits and
// QK_RESIDENT_STATS numbers:
//   stats [0 .. 4]  matrix instructions of the steps that are side by side, in place (one round), partially resident, evicted whole with X'
//                   whole in LDS (X or the rule's answer leaves no panel), in strips (X or X' does not fit the segmentation's buffer)
//   stats [5]       phase-1 matrix instructions of the units of partially resident steps whose panel stays (they run the LDS form)
//   stats [6]       elements of X copied from LDS to the global buffer
//   stats [7], [8]  panels of X in the partially resident steps, and how many of them stay
//   stats [9]       phase-1 matrix instructions of the partially resident steps
// Case bits of a chain: bit 0 a partially resident step with X at the low end, bit 1 with X at the top, bit 2 two partially resident steps in
// a row (X low, then top, or the reverse), bit 3 a partially resident step keeps exactly one panel, bit 4 all but one, bit 5 none, bit 6 a
// merged step (pd = 4) is partially resident, bit 7 a partially resident step is directly followed by a step that is not LDS-resident and keeps
// nothing, bit 8 directly preceded by one (its X came from the global buffer and its X' stayed whole in LDS), bit 9 the last block of rows of a
// partially resident step has fewer than 4 k-steps (a ragged true bond), bit 10 that block's panel stays, bit 11 it is evicted, bit 12 a step
// is side by side in `rcap` elements but not in the segmentation's xcap, bit 13 a partially resident step switches (never: a switch step is
// LDS-resident).
static constexpr int QK_RESIDENT_STATS = 10;
extern "C" void qk_resident_pairs(const int32_t* x_true, const int32_t* y_true, int32_t n_sites, const int32_t* pairs, int64_t n_pairs, int32_t ek, int32_t xcap, int32_t cap, int32_t dual,
                                  int32_t rcap, int32_t partial, int32_t parities, int32_t assoc, int32_t switch_price, int32_t* cases, int64_t* stats) {
  const QkSegRule rule{xcap, cap, dual != 0, rcap, partial != 0};
  const int n1 = n_sites + 1, m = n_sites - 2 * ek;
  std::vector<int32_t> xd(n1), yd(n1);
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t* xt = x_true + (int64_t)pairs[2 * p] * n1;
    const int32_t* yt = y_true + (int64_t)pairs[2 * p + 1] * n1;
    for (int i = 0; i < n1; ++i) xd[i] = qk_pad16(xt[i]), yd[i] = qk_pad16(yt[i]);
    QkSegMask o{{0ull, 0ull}};
    const QkSegMask k = qk_segment_chain(xd.data(), xt, yd.data(), yt, n_sites, ek, rule, parities, false, nullptr, nullptr, parities ? assoc : 0, switch_price, &o, nullptr);
    int64_t* const st = stats + QK_RESIDENT_STATS * p;
    for (int i = 0; i < QK_RESIDENT_STATS; ++i) st[i] = 0;
    int c = 0, xb = 0, prev = -1;  // prev: what the step before was -- 0 LDS-resident or side by side, 1 partially resident, 2 neither
    bool prev_top = false;
    for (int i = 0; i < m;) {
      const int len = qk_seg_bit(k.w[0], k.w[1], i) ? 2 : 1, e = ek + i;
      const bool o1 = qk_seg_bit(o.w[0], o.w[1], i), s = qk_seg_bit(o.w[0], o.w[1], i + len) != o1;
      const int a = o1 ? yd[e] : xd[e], a2 = o1 ? yd[e + len] : xd[e + len], b = o1 ? xd[e] : yd[e], b2 = o1 ? xd[e + len] : yd[e + len];
      const int at = o1 ? yt[e] : xt[e], bt = o1 ? xt[e] : yt[e];
      const int mt = a / 16, nt = b2 / 16, pd = 2 * len;
      const bool top = xb != 0, x_lds = a * b <= xcap;
      const QkResident r = qk_resident(rule, a, a2, b, b2, pd, top);
      const long long instr = qk_step_instr(pd, a, a2, b, b2, at, bt), p1_panel = 3ll * pd * nt * ((bt + 3) >> 2);  // phase 1 of the units of one row block
      const bool strips = a * b > xcap || a2 * b2 > xcap;
      st[r.kind == QK_RES_SIDE ? 0 : r.kind == QK_RES_INPLACE ? 1 : r.kind == QK_RES_PART ? 2 : strips ? 4 : 3] += instr;
      if (x_lds) st[6] += (long long)(mt - (r.khi - r.klo)) * b * 16;
      if (r.kind == QK_RES_SIDE && a * b + a2 * b2 > xcap) c |= 1 << 12;
      if (r.kind == QK_RES_PART) {
        const int keep = r.khi - r.klo, klast = (at - (mt - 1) * 16 + 3) >> 2;
        st[5] += p1_panel * keep, st[7] += mt, st[8] += keep, st[9] += p1_panel * mt;
        c |= (top ? 2 : 1) | (keep == 1 ? 8 : 0) | (keep == mt - 1 ? 16 : 0) | (keep == 0 ? 32 : 0) | (pd == 4 ? 64 : 0) | (s ? 1 << 13 : 0);
        if (prev == 1 && prev_top != top) c |= 4;
        if (prev == 2) c |= 1 << 8;
        if (klast < 4) c |= (1 << 9) | (mt - 1 >= r.klo && mt - 1 < r.khi ? 1 << 10 : 1 << 11);
      } else if (r.kind == QK_RES_NONE && prev == 1) {
        c |= 1 << 7;
      }
      prev = r.kind == QK_RES_PART ? 1 : r.kind == QK_RES_NONE ? 2 : 0, prev_top = top;
      if (a2 * b2 > xcap) xb = 0, prev = -1;  // X' left the LDS in strips: the next step finds X in the global buffer
      else xb = r.ob;
      i += len;
    }
    cases[p] = c;
  }
}

extern "C" int32_t qk_rcap_one() { return QKF_RCAP_ONE; }  // the large buffer of the 12-wave shapes as the kernels are built
