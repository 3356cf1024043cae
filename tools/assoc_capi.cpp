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
