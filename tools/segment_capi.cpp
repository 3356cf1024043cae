// A C entry to the segmentation of the site-fused sweep (qk_segment_chain, csrc/qk_plan.h) for tools/merge_potential.py and the tests:
// the same function the device runs, compiled for the host (g++ -O2 -shared -fPIC) and called through ctypes.  Not part of the product.
#include "../qml-cutensornet_amd/csrc/qk_plan.h"

// x_true / y_true: [states][n_sites + 1] true bonds; pairs: [n_pairs][2] = (x state, y state).  Per pair: the mask (two words), the matrix
// instructions of its steps and the number of steps.  greedy != 0: every admissible merge at an allowed start (QK_MERGE=1 with parities 1).
extern "C" void qk_segment_pairs(const int32_t* x_true, const int32_t* y_true, int32_t n_sites, const int32_t* pairs, int64_t n_pairs, int32_t ek, int32_t xcap, int32_t cap, int32_t dual,
                                 int32_t parities, int32_t greedy, uint64_t* masks, int64_t* instr, int32_t* steps) {
  const QkSegRule rule{xcap, cap, dual != 0};
  const int n1 = n_sites + 1;
  std::vector<int32_t> xd(n1), yd(n1);
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t* xt = x_true + (int64_t)pairs[2 * p] * n1;
    const int32_t* yt = y_true + (int64_t)pairs[2 * p + 1] * n1;
    for (int i = 0; i < n1; ++i) xd[i] = qk_pad16(xt[i]), yd[i] = qk_pad16(yt[i]);
    long long obj = 0;
    int st = 0;
    const QkSegMask m = qk_segment_chain(xd.data(), xt, yd.data(), yt, n_sites, ek, rule, parities, greedy != 0, &obj, &st);  // (parities 0: every site a step)
    masks[2 * p] = m.w[0], masks[2 * p + 1] = m.w[1];
    instr[p] = obj - (long long)st * QK_STEP_PRICE, steps[p] = st;
  }
}
