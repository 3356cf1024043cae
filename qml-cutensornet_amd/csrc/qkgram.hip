// qkgram.hip -- MI355X (gfx950 / CDNA4) engine for the quantum-kernel Gram hot path.
//
// What it replaces (reference = mmetcalf14/qml-cutensornet, G = gpu_backend/kernel_state_ansatz.py):
//   G:372-400  the Python double loop calling  x_mps.vdot(y_mps)  once per Gram entry
//   G:380      MPS.vdot -> one cuTensorNet contraction + a device->host sync per entry
// by ONE persistent kernel launch per Gram share: every workgroup pulls (x_i, y_j) pairs
// from a device-side queue and carries the whole transfer-matrix sweep
//     X_0 = 1,   X_{k+1}[r,R] = sum_{L,l,p} X_k[l,L] * conj(A_k[L,p,R]) * B_k[l,p,r]
// on chip/L2 as a chain of complex GEMMs on the f64 matrix cores
// (v_mfma_f64_16x16x4_f64), and finally writes |<x|y>|^2.
//
//
// Files: this one = C ABI (include/qkgram.h), packing, the kernels that make a set's derived images (interleaved tensors, edge blocks,
// merged steps), small kernels, launches;  qk_planner.cpp = the host planner (plain C++);  qk_fused.h = the site-fused sweep (the fp64 hot
// path, plain and DET forms) and the 2 x 2-tile one-wave sweep (fp64, bonds <= 32);  qk_ring.h = the ring sweep (complex64, very large
// bonds), the LDS-resident small-bond sweep and the one-tile one-wave sweep;  qk_build.hip = the device MPS builder;  qk_comm.hip = the
// multi-GPU entry points.  lab/qk_lab.hip (experimental / diagnostic kernels) is NOT part of libqkgram.so: it is linked only into
// libqklab.so (-DQK_LAB), which lab/tools load for A/B measurements.
// Written for gfx950 only: 64-lane wavefronts, 160 KiB LDS per CU, no portability layer.
#include "qk_host.h"
#include "qk_ring.h"
#include "qk_fused.h"
#ifndef QKF_QUAD
#define QKF_QUAD 0  // lab builds only (-DQKF_QUAD=1 -I lab): the quad form of the site-fused sweep (lab/qk_quad.h) stands in for the plain dual form
#endif
#if QKF_QUAD
#include "qk_quad.h"
#endif

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

// ----------------------------------------------------------------------------------------
// errors
// ----------------------------------------------------------------------------------------
static thread_local std::string g_err;

int qk_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define fail qk_fail

extern "C" const char* qk_last_error(void) { return g_err.c_str(); }

#include <atomic>
uint64_t qk_next_uid() {
  static std::atomic<uint64_t> next{1};
  return next.fetch_add(1);
}

// ----------------------------------------------------------------------------------------
// roctx ranges around the phases of the path (build / upload / sweep / all-gather / scatter: the reference's timing sites
// G:379-381 and its profiling keys), so that ONE `rocprofv3 --marker-trace --kernel-trace` run yields the phase table.
// The marker library is resolved at first use -- only when a profiler is attached (rocprofv3 preloads its tool library)
// or QK_ROCTX=1 -- and the calls are no-ops otherwise.
// ----------------------------------------------------------------------------------------
#include <dlfcn.h>
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
};
Roctx& roctx() {
  static Roctx r = [] {
    Roctx x;
    const char* e = std::getenv("QK_ROCTX");
    const char* pre = std::getenv("LD_PRELOAD");
    const bool attached = std::getenv("ROCP_TOOL_LIBRARIES") || (pre && std::strstr(pre, "rocprofiler"));
    if (e ? std::atoi(e) == 0 : !attached) return x;
    void* h = nullptr;
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return x;
    x.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    x.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!x.push || !x.pop) x.push = nullptr, x.pop = nullptr;
    return x;
  }();
  return r;
}
}  // namespace
extern "C" int qk_range_push(const char* name) {
  Roctx& r = roctx();
  return (r.push && name) ? r.push(name) : 0;
}
extern "C" int qk_range_pop(void) {
  Roctx& r = roctx();
  return r.pop ? r.pop() : 0;
}

static inline int pad16(int x) { return (x + TILE - 1) / TILE * TILE; }

// ----------------------------------------------------------------------------------------
// host: packing one MPS into the padded planar device image
// ----------------------------------------------------------------------------------------
extern "C" int64_t qk_pack_state_size(int32_t n_sites, const int32_t* bond_dims) {
  int64_t tot = 0;
  for (int k = 0; k < n_sites; ++k) tot += 2ll * pad16(bond_dims[k]) * 2 * pad16(bond_dims[k + 1]);
  return tot;
}

extern "C" int qk_pack_state(int32_t n_sites, const int32_t* bond_dims, const double* const* site_tensors,
                             int32_t layout, double* out, int64_t* site_offsets) {
  if (n_sites <= 0 || !bond_dims || !site_tensors || !out) return fail(QK_EINVAL, "qk_pack_state: null argument");
  if (layout != QK_LAYOUT_LPR && layout != QK_LAYOUT_LRP) return fail(QK_EINVAL, "qk_pack_state: unknown layout %d", layout);
  if (bond_dims[0] != 1 || bond_dims[n_sites] != 1) return fail(QK_EINVAL, "qk_pack_state: boundary bonds must be 1");
  int64_t off = 0;
  for (int k = 0; k < n_sites; ++k) {
    const int cl = bond_dims[k], cr = bond_dims[k + 1];
    if (cl <= 0 || cr <= 0) return fail(QK_EINVAL, "qk_pack_state: non-positive bond at site %d", k);
    const int pl = pad16(cl), pr = pad16(cr);
    const int64_t plane = (int64_t)pl * 2 * pr;
    double* re = out + off;
    double* im = re + plane;
    std::memset(re, 0, sizeof(double) * 2 * plane);
    const double* src = site_tensors[k];
    if (!src) return fail(QK_EINVAL, "qk_pack_state: null tensor at site %d", k);
    for (int l = 0; l < cl; ++l)
      for (int p = 0; p < 2; ++p)
        for (int r = 0; r < cr; ++r) {
          const int64_t s = (layout == QK_LAYOUT_LPR) ? (((int64_t)l * 2 + p) * cr + r) : (((int64_t)l * cr + r) * 2 + p);
          const int64_t d = ((int64_t)l * 2 + p) * pr + r;
          re[d] = src[2 * s];
          im[d] = src[2 * s + 1];
        }
    if (site_offsets) site_offsets[k] = off;
    off += 2 * plane;
  }
  return QK_OK;
}

// ----------------------------------------------------------------------------------------
// The planner (work model, contraction order, tiles, ranks, queues) is qk_planner.cpp; the launch shapes it plans for:
// ----------------------------------------------------------------------------------------
// shapes of the two instantiations: waves per workgroup, T slots per wave, waves per SIMD (experiment builds override them)
#ifndef QKF_ONE_NW
#define QKF_ONE_NW 12  // three waves per SIMD at 168 VGPRs: 452 against 482 ms for 8 waves x 4 slots on the headline set (16 x 1: 455)
#define QKF_ONE_S 2
#define QKF_ONE_WPS 3
#endif
#ifndef QKF_TWO_NW
#define QKF_TWO_NW 8  // four waves per SIMD at 128 VGPRs, one slot: 16.4 against 18.2 ms for 4 waves x 4 slots on the 40-qubit x 4-layer set
#define QKF_TWO_S 1
#define QKF_TWO_WPS 4
#endif
#define QKF_KERNEL_ONE qk_sweep_fused_kernel<QKF_ONE_NW, QKF_ONE_S, QKF_XCAP_ONE, QKF_ONE_WPS>
#define QKF_KERNEL_TWO qk_sweep_fused_kernel<QKF_TWO_NW, QKF_TWO_S, QKF_XCAP_TWO, QKF_TWO_WPS>
#ifndef QKF_DUAL_NW
#define QKF_DUAL_NW 12
#define QKF_DUAL_WPS 3
#endif
#define QKF_KERNEL_DUAL qk_sweep_fused_dual_kernel<QKF_DUAL_NW, QKF_XCAP_ONE, QKF_DUAL_WPS>
// the DET forms (QK_DETERMINISTIC=1): ordered accumulation into X' (qk_fused.h: qkf_turn_add) -- bit-reproducible Grams
#define QKF_KERNEL_ONE_DET qk_sweep_fused_kernel<QKF_ONE_NW, QKF_ONE_S, QKF_XCAP_ONE, QKF_ONE_WPS, true>
#define QKF_KERNEL_TWO_DET qk_sweep_fused_kernel<QKF_TWO_NW, QKF_TWO_S, QKF_XCAP_TWO, QKF_TWO_WPS, true>
#define QKF_KERNEL_DUAL_DET qk_sweep_fused_dual_kernel<QKF_DUAL_NW, QKF_XCAP_ONE, QKF_DUAL_WPS, true>
// the 12-wave shapes with the large X buffer (qk_plan.h: QKF_RCAP_ONE; the segmentation still counts on QKF_XCAP_ONE): launch_sweep takes them
// whenever the launch's tables fit behind the larger buffer
#define QKF_KERNEL_ONE_BIG qk_sweep_fused_kernel<QKF_ONE_NW, QKF_ONE_S, QKF_XCAP_ONE, QKF_ONE_WPS, false, QKF_RCAP_ONE>
#define QKF_KERNEL_DUAL_BIG qk_sweep_fused_dual_kernel<QKF_DUAL_NW, QKF_XCAP_ONE, QKF_DUAL_WPS, false, QKF_RCAP_ONE>
#define QKF_KERNEL_ONE_DET_BIG qk_sweep_fused_kernel<QKF_ONE_NW, QKF_ONE_S, QKF_XCAP_ONE, QKF_ONE_WPS, true, QKF_RCAP_ONE>
#define QKF_KERNEL_DUAL_DET_BIG qk_sweep_fused_dual_kernel<QKF_DUAL_NW, QKF_XCAP_ONE, QKF_DUAL_WPS, true, QKF_RCAP_ONE>
#if QKF_QUAD  // (lab builds: lab/qk_quad.h, 2 x 2 tiles per wave, 8 waves at two per SIMD)
#define QKF_QUAD_NW 8
#define QKF_KERNEL_QUAD qk_sweep_fused_quad_kernel<QKF_QUAD_NW, QKF_XCAP_ONE, 2>
#endif

extern "C" int qk_plan_destroy(qk_plan* plan) {
  if (!plan) return QK_OK;
  if (plan->d_pairs) (void)hipFree(plan->d_pairs);
  if (plan->d_groups) (void)hipFree(plan->d_groups);
  if (plan->d_seg) (void)hipFree(plan->d_seg);
  delete plan;
  return QK_OK;
}
// ----------------------------------------------------------------------------------------
// small kernels of the product path (the sweep kernels are in qk_ring.h)
// ----------------------------------------------------------------------------------------
__global__ void qk_convert_f32_kernel(const double* __restrict__ src, float* __restrict__ dst, const long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) dst[e] = (float)src[e];
}

__global__ void qk_scatter_kernel(const int32_t* __restrict__ pairs, const double* __restrict__ vals, long long n,
                                  double* __restrict__ K, long long ld, int mirror) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int i = pairs[2 * t], j = pairs[2 * t + 1];
  if (i < 0) return;  // padding entry of an all-gathered list
  const double v = vals[t];
  K[(long long)j * ld + i] = v;
  if (mirror) K[(long long)i * ld + j] = v;
}

// ----------------------------------------------------------------------------------------
// Derived images of a set (made once per set, on the cold path of its first Gram): both are chains of small complex products and run
// on the f64 matrix cores, reading the interleaved image like the sweep does.
// ----------------------------------------------------------------------------------------
typedef double qk_v2d __attribute__((ext_vector_type(2)));

// One 16 x 16 complex tile  C[m][n] = sum_{k < 4 ks4} P[k][m] Q[k][n]  (3M product).  Element (k, m) of P at P + k pk + m pm, element
// (k, n) of Q at Q + k qk + n qn (complex elements); the tile comes back in the C/D register layout (register r of lane (q, j) = C[q + 4 r][j]).
__device__ __forceinline__ void qk_ctile(QkfTile& t, const qk_v2d* __restrict__ P, const long pk, const long pm, const qk_v2d* __restrict__ Q, const long qk, const long qn, const int ks4,
                                         const int q, const int j) {
  const qk_v2d* pp = P + q * pk + j * pm;
  const qk_v2d* qq = Q + q * qk + j * qn;
  v4d p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0};
  qk_v2d a = pp[0], b = qq[0];
  for (int ks = 0; ks < ks4; ++ks) {
    const qk_v2d a0 = a, b0 = b;
    if (ks + 1 < ks4) a = pp[(long)4 * (ks + 1) * pk], b = qq[(long)4 * (ks + 1) * qk];
    qkf_kstep<false>(p1, p2, p3, a0.x, a0.y, b0.x, b0.y);
  }
  t.re = p1 - p2, t.im = p3 - p1 - p2;
}

// Edge blocks of a set (SweepArgs.edge_k; qk_fused.h): per state the first k sites contracted into L[s][a] (s = the configuration of
// the first k physical legs, row index built as 2 s + p site by site; a = bond k, padded) and the last k sites into R[s][a] (a = bond
// n - k).  One workgroup per (state, side) at a time; a step multiplies the block so far by one site tensor of the interleaved image --
// out[2 s + p][c] = sum_l in[s][l] A[l][p][c] on the left, A[c][p][l] on the right: 16 x 16 tiles dealt to the workgroup's wavefronts,
// K up to the TRUE bond --, ping-pong between two scratch buffers of the workgroup, the last step writes the destination.
__global__ __launch_bounds__(256) void qk_edge_kernel(const qk_v2d* __restrict__ il, const int32_t* __restrict__ dims, const int32_t* __restrict__ dtrue, const int64_t* __restrict__ offs,
                                                      const int n_sites, const int k, const long long n_states, qk_v2d* __restrict__ edge, const long long* __restrict__ edge_offs,
                                                      qk_v2d* __restrict__ tmp, const long long tmp_elems) {
  qk_v2d* const t0 = tmp + (long long)blockIdx.x * 2 * tmp_elems;
  qk_v2d* const t1 = t0 + tmp_elems;
  const int n1 = n_sites + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, j = lane & 15, q = lane >> 4;
  for (long long t = blockIdx.x; t < 2 * n_states; t += gridDim.x) {
    const long long st = t >> 1;
    const int right = (int)(t & 1);
    const int32_t* d = dims + st * n1;
    const int32_t* dt = dtrue + st * n1;
    qk_v2d* const dst = edge + edge_offs[t];
    // the block before the first step: one row, 1 at [0][0] (the boundary bond is 1, padded to 16); the other 15 rows of its tile are zero
    for (int e = threadIdx.x; e < 256; e += blockDim.x) t0[e] = (qk_v2d){e == 0 ? 1.0 : 0.0, 0.0};
    __syncthreads();
    const qk_v2d* in = t0;
    for (int jj = 0; jj < k; ++jj) {
      const int site = right ? n_sites - 1 - jj : jj;
      const int lp = d[site], rp = d[site + 1];  // padded bonds of the site tensor [lp][2][rp]
      const qk_v2d* const A = il + (offs[st * n_sites + site] >> 1);
      const int ld_in = right ? rp : lp, ld_out = right ? lp : rp, rows_in = 1 << jj;
      const int ks4 = ((right ? dt[site + 1] : dt[site]) + 3) >> 2;  // k-steps below the true bond that is summed over
      qk_v2d* const out = (jj + 1 == k) ? dst : (in == t0 ? t1 : t0);
      const int nts = (rows_in + 15) >> 4, ntc = ld_out >> 4;
      for (int u = wave; u < nts * 2 * ntc; u += nw) {
        const int tc = u % ntc, pp = (u / ntc) & 1, ts = u / (2 * ntc);
        QkfTile T;
        // left: Q[l][c] = A[l][pp][c];  right: Q[l][c] = A[c][pp][l]
        if (right) qk_ctile(T, in + (long)(ts * 16) * ld_in, 1, ld_in, A + (long)pp * rp + (long)(tc * 16) * 2 * rp, 1, 2 * rp, ks4, q, j);
        else qk_ctile(T, in + (long)(ts * 16) * ld_in, 1, ld_in, A + (long)pp * rp + tc * 16, 2 * rp, 1, ks4, q, j);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s_ = ts * 16 + q + 4 * r;
          if (s_ < rows_in) out[(long)(2 * s_ + pp) * ld_out + tc * 16 + j] = (qk_v2d){T.re[r], T.im[r]};
        }
      }
      __syncthreads();
      in = out;
    }
  }
}

// Merged image of a set (SweepArgs.merge_steps; qk_fused.h): task t of state st = the chain's sites s = k + stride t and s + 1 contracted
// over the bond between them (stride 1: every start; 2: the even starts only), written at out_offs[st][s - k]:
// M[l][2 p1 + p2][r] = sum_m A_s[l][p1][m] A_{s+1}[m][p2][r] (padded bonds; the padding of the image is zero, so is M's).  A UNIT is one 16 x 16 block (tl, tr) of one step with its four physical combinations: the two fragments of A_s and the two
// of A_{s+1} of a k-step feed four complex products (12 matrix instructions per 4 loads), K up to the true bond between the sites.  Units
// of all steps and states are numbered through a prefix table (unit_start) and dealt to the wavefronts of the grid, so the launch
// does not end with the largest state.  Reads and writes interleaved complex.  Once per set: not part of a sweep.
__global__ __launch_bounds__(256, 2) void qk_merge_kernel(const qk_v2d* __restrict__ il, const int32_t* __restrict__ dims, const int32_t* __restrict__ dtrue, const int64_t* __restrict__ offs,
                                                          const int n_sites, const int k, const int steps, const int stride, const int n_starts, const long long n_tasks, const long long* __restrict__ unit_start,
                                                          qk_v2d* __restrict__ out, const int64_t* __restrict__ out_offs) {
  const int n1 = n_sites + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, j = lane & 15, q = lane >> 4;
  const long long n_units = unit_start[n_tasks];
  for (long long u = (long long)blockIdx.x * nw + wave; u < n_units; u += (long long)gridDim.x * nw) {
    long long lo = 0, hi = n_tasks;  // the task of unit u: the last t with unit_start[t] <= u
    while (hi - lo > 1) {
      const long long mid = (lo + hi) >> 1;
      if (unit_start[mid] <= u) lo = mid;
      else hi = mid;
    }
    const long long t = lo, st = t / steps;
    const int step = (int)(t - st * steps), s_ = k + stride * step, v = (int)(u - unit_start[t]);
    const int32_t* d = dims + st * n1;
    const int lp = d[s_], mp = d[s_ + 1], rp = d[s_ + 2], ntr = rp >> 4, tl = v / ntr, tr = v - tl * ntr;
    (void)lp;
    const int ks4 = (dtrue[st * n1 + s_ + 1] + 3) >> 2;
    const qk_v2d* const A1 = il + (offs[st * n_sites + s_] >> 1);      // [lp][2][mp]
    const qk_v2d* const A2 = il + (offs[st * n_sites + s_ + 1] >> 1);  // [mp][2][rp]
    // lane (q, j) of k-step ks: A1[16 tl + j][p1][4 ks + q], A2[4 ks + q][p2][16 tr + j]
    const qk_v2d* pa = A1 + ((long)(tl * 16 + j) * 2) * mp + q;
    const qk_v2d* pb = A2 + ((long)q * 2) * rp + tr * 16 + j;
    v4d acc[4][3];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 3; ++e) acc[c][e] = (v4d){0, 0, 0, 0};
    qk_v2d a0 = pa[0], a1 = pa[mp], b0 = pb[0], b1 = pb[rp];
    for (int ks = 0; ks < ks4; ++ks) {
      const qk_v2d x0 = a0, x1 = a1, y0 = b0, y1 = b1;
      if (ks + 1 < ks4) {
        pa += 4, pb += (long)8 * rp;
        a0 = pa[0], a1 = pa[mp], b0 = pb[0], b1 = pb[rp];
      }
      qkf_kstep<false>(acc[0][0], acc[0][1], acc[0][2], x0.x, x0.y, y0.x, y0.y);
      qkf_kstep<false>(acc[1][0], acc[1][1], acc[1][2], x0.x, x0.y, y1.x, y1.y);
      qkf_kstep<false>(acc[2][0], acc[2][1], acc[2][2], x1.x, x1.y, y0.x, y0.y);
      qkf_kstep<false>(acc[3][0], acc[3][1], acc[3][2], x1.x, x1.y, y1.x, y1.y);
    }
    qk_v2d* const dst = out + (out_offs[st * n_starts + stride * step] >> 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const v4d re = acc[c][0] - acc[c][1], im = acc[c][2] - acc[c][0] - acc[c][1];
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(long)(4 * (tl * 16 + q + 4 * r) + c) * rp + tr * 16 + j] = (qk_v2d){re[r], im[r]};
    }
  }
}

// The segmentation masks of a launch's pairs (SweepArgs.seg; qk_plan.h: qk_segment_chain; four words per pair: merges, orientations): one thread per pair.  Once per plan, sets and
// launch shape (ensure_segments): not part of a steady-state sweep.
__global__ __launch_bounds__(256) void qk_segment_kernel(const int32_t* __restrict__ xdims, const int32_t* __restrict__ xtrue, const int32_t* __restrict__ ydims, const int32_t* __restrict__ ytrue,
                                                         const int n_sites, const int ek, const int32_t* __restrict__ pairs, const long long npairs, const QkSegRule rule, const int parities,
                                                         const bool greedy, const int assoc, const int switch_price, unsigned long long* __restrict__ seg) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  const long long xo = (long long)pairs[2 * p] * (n_sites + 1), yo = (long long)pairs[2 * p + 1] * (n_sites + 1);
  QkSegMask o{{0ull, 0ull}};  // the orientations of the steps (qk_plan.h: the association of a step)
  const QkSegMask m = qk_segment_chain(xdims + xo, xtrue + xo, ydims + yo, ytrue + yo, n_sites, ek, rule, parities, greedy, nullptr, nullptr, assoc, switch_price, &o);
  seg[4 * p] = m.w[0], seg[4 * p + 1] = m.w[1], seg[4 * p + 2] = o.w[0], seg[4 * p + 3] = o.w[1];
}

#ifdef QK_LAB
__global__ void qk_lab_fold_kernel(const int64_t* __restrict__ src, int64_t* __restrict__ dst, const long long n, const long long win) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = (src[i] % win) & ~1ll;
}
#endif
// self-test: C[16x16] = sum_{k<16} P[k][m] * Q[k][n] with the fragment maps used above
__global__ void qk_selftest_f32_kernel(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ C) {
  const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  v4f acc = {0, 0, 0, 0};
  for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(P[(4 * ks + q) * 16 + j], Q[(4 * ks + q) * 16 + j], acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) C[(4 * q + r) * 16 + j] = acc[r];
}

__global__ void qk_selftest_kernel(const double* __restrict__ P, const double* __restrict__ Q, double* __restrict__ C) {
  const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  v4d acc = {0, 0, 0, 0};
  for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(P[(4 * ks + q) * 16 + j], Q[(4 * ks + q) * 16 + j], acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) C[(q + 4 * r) * 16 + j] = acc[r];
}

// ----------------------------------------------------------------------------------------
// host API
// ----------------------------------------------------------------------------------------
extern "C" int qk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static int ctx_init(qk_ctx* c, int device_id, int num_cus);

extern "C" int qk_ctx_create(int device_id, qk_ctx** out) {
  if (!out) return fail(QK_EINVAL, "qk_ctx_create: null out");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(QK_EDEVICE, "qk_ctx_create: no HIP device available (%s); this engine has no CPU fallback",
                e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= n) return fail(QK_EINVAL, "qk_ctx_create: device %d out of range [0,%d)", device_id, n);
  HIP_TRY(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(QK_EDEVICE, "qk_ctx_create: device %d is %s; this library is built for gfx950 only", device_id, prop.gcnArchName);
  qk_ctx* c = new (std::nothrow) qk_ctx;
  if (!c) return fail(QK_ENOMEM, "qk_ctx_create: out of memory");
  const int rc_init = ctx_init(c, device_id, prop.multiProcessorCount);
  if (rc_init != QK_OK) {
    qk_ctx_destroy(c);  // releases whatever was created before the failure
    return rc_init;
  }
  *out = c;
  return QK_OK;
}

static int ctx_init(qk_ctx* c, int device_id, int num_cus) {
  c->device = device_id;
  c->num_cus = num_cus;
  HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipEventCreate(&c->ev_mid));
  HIP_TRY(hipEventCreate(&c->ev_d));
  HIP_TRY(c->counter.alloc((QK_NQ_MAX * QK_QSTRIDE + 8 + 2 * 8 * QK_QSTRIDE) * sizeof(unsigned long long)));  // queue heads (8 per launch of a split sweep), tail clocks
  HIP_TRY(c->prof.alloc(8 * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(c->prof.get(), 0, 8 * sizeof(unsigned long long)));
  // the dynamic LDS the sweep kernels may ask for: 80 KiB (two workgroups per CU), a whole CU's 160 KiB, or its share per workgroup of the small-site shape
  for (const void* k : {(const void*)qk_sweep_ring_kernel<float>, (const void*)qk_sweep_ring_kernel<double>, (const void*)qk_sweep_small_kernel<double>, (const void*)qk_sweep_small_kernel<float>})
    HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
  for (const void* k : {(const void*)QKF_KERNEL_ONE, (const void*)QKF_KERNEL_DUAL, (const void*)QKF_KERNEL_ONE_DET, (const void*)QKF_KERNEL_DUAL_DET, (const void*)QKF_KERNEL_ONE_BIG,
                        (const void*)QKF_KERNEL_DUAL_BIG, (const void*)QKF_KERNEL_ONE_DET_BIG, (const void*)QKF_KERNEL_DUAL_DET_BIG})
    HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  for (const void* k : {(const void*)QKF_KERNEL_TWO, (const void*)QKF_KERNEL_TWO_DET}) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 / QKF_TWO_WGS));
#if QKF_QUAD
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(QKF_KERNEL_QUAD), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#endif
  QkSweepPolicy& p = c->policy;
#ifdef QK_LAB  // libqklab.so only: the experimental kernels of qk_lab.hip, selectable with QK_VARIANT
  {
    const int rc = qk_lab_init(c);
    if (rc != QK_OK) return rc;
  }
  if (const char* v = std::getenv("QK_VARIANT")) p.variant = std::atoi(v);
#endif
  if (const char* v = std::getenv("QK_SMALL")) p.small_path = std::atoi(v) != 0;
  if (const char* v = std::getenv("QK_WAVE")) p.wave_path = std::atoi(v) != 0;
  if (const char* v = std::getenv("QK_WAVE2")) p.wave2_path = std::atoi(v) != 0, p.wave2_ring = std::atoi(v) != 2;
  if (const char* v = std::getenv("QK_FUSED")) p.fused_path = std::atoi(v);
  if (const char* v = std::getenv("QK_MERGE")) p.merge_mode = std::max(0, std::min(2, std::atoi(v)));
  if (const char* v = std::getenv("QK_ASSOC")) p.assoc_mode = std::max(0, std::min(3, std::atoi(v)));
  if (const char* v = std::getenv("QK_SWITCH_PRICE")) p.switch_price = std::max(0, std::min(100000, std::atoi(v)));
  // QK_DETERMINISTIC=1: bit-reproducible Grams.  By default the site-fused sweep sums the tiles of a column with LDS atomics in arrival
  // order (two launches on the same inputs differ in the last bits, <= 9e-16); in this mode it takes its DET forms, which add in a fixed
  // order (qk_fused.h: qkf_turn_add); the ring sweep, the small-bond sweep and the one-wave sweeps add in a fixed order anyway.  The order
  // in which workgroups pull pairs never matters (a pair's result does not depend on the workgroup that sweeps it).
  if (const char* v = std::getenv("QK_DETERMINISTIC"))
    if (std::atoi(v) != 0) p.deterministic = true, p.assoc_mode = 0;  // (the ordered forms have no switch step: orientation 0 throughout)
  if (const char* v = std::getenv("QK_FUSED_SPLIT")) p.fused_split = std::max(0, std::min(2, std::atoi(v)));
  if (const char* v = std::getenv("QK_FUSED_WGS")) p.fused_wgs = std::max(0, std::min(2, std::atoi(v)));
  if (const char* v = std::getenv("QK_WGS_PER_CU")) p.wgs_per_cu = std::max(1, std::min(4, std::atoi(v)));
  return QK_OK;
}

extern "C" int qk_ctx_destroy(qk_ctx* c) {
  if (!c) return QK_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev_mid) (void)hipEventDestroy(c->ev_mid);
  if (c->ev_d) (void)hipEventDestroy(c->ev_d);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // its buffers go with it (qk_devmem.h)
  return QK_OK;
}

extern "C" int qk_ctx_trim(qk_ctx* c) {
  if (!c) return fail(QK_EINVAL, "qk_ctx_trim: null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (QkGrowBuf* b : {&c->scratch, &c->build_arena, &c->build_work, &c->derive_tmp, &c->local_scratch}) b->reset();
  return QK_OK;
}

extern "C" int qk_ctx_set_stream(qk_ctx* c, void* s) {
  if (!c) return fail(QK_EINVAL, "qk_ctx_set_stream: null context");
  c->stream = reinterpret_cast<hipStream_t>(s);  // NULL = HIP's null stream
  return QK_OK;
}

extern "C" int qk_ctx_use_own_stream(qk_ctx* c) {
  if (!c) return fail(QK_EINVAL, "qk_ctx_use_own_stream: null context");
  c->stream = c->own_stream;
  return QK_OK;
}

extern "C" int qk_ctx_synchronize(qk_ctx* c) {
  if (!c) return fail(QK_EINVAL, "qk_ctx_synchronize: null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QK_OK;
}

int qk_mps_set_alloc(qk_ctx* c, int n_states, int n_sites, int64_t data_bytes, int precision, qk_mps_set** out, const char* who) {
  qk_mps_set* m = new (std::nothrow) qk_mps_set;
  if (!m) return fail(QK_ENOMEM, "%s: out of memory", who);
  m->ctx = c, m->n_states = n_states, m->n_sites = n_sites, m->precision = precision, m->bytes = data_bytes;
  const size_t nd = (size_t)n_states * (n_sites + 1), no = (size_t)n_states * n_sites;
  hipError_t e = m->d_data.alloc((size_t)data_bytes);
  if (e == hipSuccess) e = m->d_dims.alloc(nd * sizeof(int32_t));
  if (e == hipSuccess) e = m->d_true.alloc(nd * sizeof(int32_t));
  if (e == hipSuccess) e = m->d_offs.alloc(no * sizeof(int64_t));
  if (e != hipSuccess) {
    qk_mps_set_destroy(m);
    return fail(QK_EDEVICE, "%s: hipMalloc of a set of %lld bytes and its tables failed: %s", who, (long long)data_bytes, hipGetErrorString(e));
  }
  *out = m;
  return QK_OK;
}

extern "C" int qk_mps_set_create(qk_ctx* c, int32_t n_states, int32_t n_sites, const int32_t* bond_dims,
                                 const double* const* site_tensors, int32_t layout, qk_mps_set** out) {
  if (!c || !out || !bond_dims || !site_tensors) return fail(QK_EINVAL, "qk_mps_set_create: null argument");
  if (n_states <= 0 || n_sites <= 0) return fail(QK_EINVAL, "qk_mps_set_create: empty set (%d states, %d sites)", n_states, n_sites);
  QkRangeGuard range_("qk:upload");
  HIP_TRY(hipSetDevice(c->device));
  const int stride = n_sites + 1;
  std::vector<int32_t> pad((size_t)n_states * stride);
  std::vector<int64_t> offs((size_t)n_states * n_sites);
  std::vector<int64_t> state_off(n_states + 1, 0);
  int max_pad = 0;
  for (int s = 0; s < n_states; ++s) {
    const int32_t* d = bond_dims + (size_t)s * stride;
    if (d[0] != 1 || d[n_sites] != 1) return fail(QK_EINVAL, "qk_mps_set_create: state %d: boundary bonds must be 1", s);
    for (int k = 0; k <= n_sites; ++k) {
      if (d[k] <= 0) return fail(QK_EINVAL, "qk_mps_set_create: state %d: non-positive bond %d", s, k);
      pad[(size_t)s * stride + k] = pad16(d[k]);
      max_pad = std::max(max_pad, pad16(d[k]));
    }
    state_off[s + 1] = state_off[s] + qk_pack_state_size(n_sites, d);
  }
  qk_mps_set* m = nullptr;
  int rc = qk_mps_set_alloc(c, n_states, n_sites, state_off[n_states] * (int64_t)sizeof(double), 64, &m, "qk_mps_set_create");
  if (rc != QK_OK) return rc;
  m->max_pad = max_pad;
  m->dims_true.assign(bond_dims, bond_dims + (size_t)n_states * stride);
  hipError_t e = hipSuccess;
  std::vector<double> stage;
  std::vector<int64_t> so(n_sites);
  for (int s = 0; s < n_states; ++s) {
    const int64_t sz = state_off[s + 1] - state_off[s];
    stage.resize((size_t)sz);
    rc = qk_pack_state(n_sites, bond_dims + (size_t)s * stride, site_tensors + (size_t)s * n_sites, layout, stage.data(), so.data());
    if (rc != QK_OK) {
      qk_mps_set_destroy(m);
      return rc;
    }
    for (int k = 0; k < n_sites; ++k) offs[(size_t)s * n_sites + k] = state_off[s] + so[k];
    e = hipMemcpy(m->d_data.get<double>() + state_off[s], stage.data(), (size_t)sz * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      qk_mps_set_destroy(m);
      return fail(QK_EDEVICE, "qk_mps_set_create: upload failed: %s", hipGetErrorString(e));
    }
  }
  e = hipMemcpy(m->d_dims.get(), pad.data(), pad.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_true.get(), bond_dims, pad.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_offs.get(), offs.data(), offs.size() * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    qk_mps_set_destroy(m);
    return fail(QK_EDEVICE, "qk_mps_set_create: table upload failed: %s", hipGetErrorString(e));
  }
  *out = m;
  return QK_OK;
}

extern "C" int qk_mps_set_destroy(qk_mps_set* m) {
  if (!m) return QK_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  delete m;  // its images and tables go with it (qk_devmem.h)
  return QK_OK;
}

extern "C" int qk_mps_set_info(const qk_mps_set* m, int32_t* n_states, int32_t* n_sites, int32_t* max_padded_bond, int64_t* device_bytes) {
  if (!m) return fail(QK_EINVAL, "qk_mps_set_info: null set");
  if (n_states) *n_states = m->n_states;
  if (n_sites) *n_sites = m->n_sites;
  if (max_padded_bond) *max_padded_bond = m->max_pad;
  if (device_bytes) *device_bytes = m->bytes * (m->d_il ? 2 : 1) + m->edge_bytes + m->mg_bytes;  // the interleaved twin the fused / wave2 sweeps make on first use counts
  return QK_OK;
}

extern "C" int qk_mps_set_precision(const qk_mps_set* m) { return m ? m->precision : 0; }

extern "C" int qk_mps_set_image(const qk_mps_set* m, int64_t* n_doubles, const double** planes_dev, int32_t* dims_true, int64_t* offsets) {
  if (!m) return fail(QK_EINVAL, "qk_mps_set_image: null set");
  if (m->precision != 64) return fail(QK_EINVAL, "qk_mps_set_image: only fp64 sets are exchanged");
  if (n_doubles) *n_doubles = m->bytes / (int64_t)sizeof(double);
  if (planes_dev) *planes_dev = m->d_data.get<double>();
  if (dims_true) std::memcpy(dims_true, m->dims_true.data(), m->dims_true.size() * sizeof(int32_t));
  if (offsets) {
    HIP_TRY(hipSetDevice(m->ctx->device));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    HIP_TRY(hipMemcpy(offsets, m->d_offs.get<int64_t>(), (size_t)m->n_states * m->n_sites * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  return QK_OK;
}

extern "C" int qk_mps_set_copy_image(const qk_mps_set* m, double* dst, int64_t n_doubles) {
  if (!m || !dst) return fail(QK_EINVAL, "qk_mps_set_copy_image: null argument");
  if (m->precision != 64) return fail(QK_EINVAL, "qk_mps_set_copy_image: only fp64 sets are exchanged");
  if (n_doubles * (int64_t)sizeof(double) < m->bytes) return fail(QK_EINVAL, "qk_mps_set_copy_image: destination holds %lld doubles, the image has %lld", (long long)n_doubles, (long long)(m->bytes / 8));
  HIP_TRY(hipSetDevice(m->ctx->device));
  HIP_TRY(hipMemcpyAsync(dst, m->d_data.get<double>(), (size_t)m->bytes, hipMemcpyDefault, m->ctx->stream));
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  return QK_OK;
}

extern "C" int qk_mps_set_from_packed(qk_ctx* c, int32_t n_states, int32_t n_sites, const int32_t* dims_true, const int64_t* offsets,
                                      const double* planes_dev, int64_t n_doubles, qk_mps_set** out) {
  if (!c || !out || !dims_true || !offsets || !planes_dev) return fail(QK_EINVAL, "qk_mps_set_from_packed: null argument");
  if (n_states <= 0 || n_sites <= 0 || n_doubles <= 0) return fail(QK_EINVAL, "qk_mps_set_from_packed: empty set");
  const int stride = n_sites + 1;
  std::vector<int32_t> pad((size_t)n_states * stride);
  int max_pad = 0;
  for (int s = 0; s < n_states; ++s) {
    const int32_t* d = dims_true + (size_t)s * stride;
    if (d[0] != 1 || d[n_sites] != 1) return fail(QK_EINVAL, "qk_mps_set_from_packed: state %d: boundary bonds must be 1", s);
    for (int k = 0; k <= n_sites; ++k) {
      if (d[k] <= 0) return fail(QK_EINVAL, "qk_mps_set_from_packed: state %d: non-positive bond %d", s, k);
      pad[(size_t)s * stride + k] = pad16(d[k]);
      max_pad = std::max(max_pad, pad16(d[k]));
    }
    for (int k = 0; k < n_sites; ++k) {  // every tensor must lie inside the buffer, 16-byte aligned
      const int64_t off = offsets[(size_t)s * n_sites + k], sz = 2ll * pad[(size_t)s * stride + k] * 2 * pad[(size_t)s * stride + k + 1];
      if (off < 0 || (off & 1) || off + sz > n_doubles) return fail(QK_EINVAL, "qk_mps_set_from_packed: state %d site %d: tensor [%lld, %lld) outside the %lld-double image", s, k, (long long)off, (long long)(off + sz), (long long)n_doubles);
    }
  }
  HIP_TRY(hipSetDevice(c->device));
  qk_mps_set* m = nullptr;
  const int rc = qk_mps_set_alloc(c, n_states, n_sites, n_doubles * (int64_t)sizeof(double), 64, &m, "qk_mps_set_from_packed");
  if (rc != QK_OK) return rc;
  m->max_pad = max_pad;
  m->dims_true.assign(dims_true, dims_true + (size_t)n_states * stride);
  hipError_t e = hipMemcpyAsync(m->d_data.get(), planes_dev, (size_t)m->bytes, hipMemcpyDefault, c->stream);  // device or host source
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_dims.get(), pad.data(), pad.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_true.get(), dims_true, pad.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_offs.get(), offsets, (size_t)n_states * n_sites * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    qk_mps_set_destroy(m);
    return fail(QK_EDEVICE, "qk_mps_set_from_packed: %s", hipGetErrorString(e));
  }
  *out = m;
  return QK_OK;
}

extern "C" int qk_mps_set_to_f32(qk_ctx* c, const qk_mps_set* src, qk_mps_set** out) {
  if (!c || !src || !out) return fail(QK_EINVAL, "qk_mps_set_to_f32: null argument");
  if (src->ctx != c) return fail(QK_EINVAL, "qk_mps_set_to_f32: the set belongs to another context");
  if (src->precision != 64) return fail(QK_EINVAL, "qk_mps_set_to_f32: the source set is not fp64");
  HIP_TRY(hipSetDevice(c->device));
  const long long n = src->bytes / (long long)sizeof(double);
  qk_mps_set* m = nullptr;
  const int rc = qk_mps_set_alloc(c, src->n_states, src->n_sites, n * (long long)sizeof(float), 32, &m, "qk_mps_set_to_f32");
  if (rc != QK_OK) return rc;
  m->max_pad = src->max_pad;
  m->dims_true = src->dims_true;
  const size_t nd = (size_t)src->n_states * (src->n_sites + 1), no = (size_t)src->n_states * src->n_sites;
  hipError_t e = hipMemcpyAsync(m->d_dims.get(), src->d_dims.get(), nd * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_true.get(), src->d_true.get(), nd * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_offs.get(), src->d_offs.get(), no * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) {
    qk_convert_f32_kernel<<<dim3(4 * c->num_cus), dim3(256), 0, c->stream>>>(src->d_data.get<double>(), m->d_data.get<float>(), n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    qk_mps_set_destroy(m);
    return fail(QK_EDEVICE, "qk_mps_set_to_f32: %s", hipGetErrorString(e));
  }
  *out = m;
  return QK_OK;
}

// the interleaved complex128 image of a set, made once on the device from the split planes
static int ensure_interleaved(qk_ctx* c, qk_mps_set* m) {
  if (m->d_il) return QK_OK;
  QkDevBuf il;  // published only after the conversion has been launched without error (released otherwise)
  HIP_TRY(il.alloc((size_t)m->bytes));
  const long long nt = (long long)m->n_states * m->n_sites;
  const dim3 grid((unsigned)std::min<long long>(nt, 64ll * c->num_cus));
  if (m->precision == 64) qk_interleave_kernel<double><<<grid, dim3(256), 0, c->stream>>>(m->d_data.get<double>(), il.get<double>(), m->d_dims.get<int32_t>(), m->d_offs.get<int64_t>(), m->n_sites, nt);
  else  // complex64 image of an fp32 set (same offsets, counted in floats)
    qk_interleave_kernel<float><<<grid, dim3(256), 0, c->stream>>>(m->d_data.get<float>(), il.get<float>(), m->d_dims.get<int32_t>(), m->d_offs.get<int64_t>(), m->n_sites, nt);
  HIP_TRY(hipGetLastError());
  m->d_il = std::move(il);
  return QK_OK;
}

// the edge blocks of a set for `k` sites at either end (made once per set and k; fp64 sets; needs the interleaved image).
// Asynchronous: the kernel is enqueued on the context's stream and nothing waits for it here (the staging tables live in the set,
// the workgroups' scratch in the context), so that a caller with several devices can enqueue all of them before any of them is done.
static int ensure_edges(qk_ctx* c, qk_mps_set* m, const int k) {
  if (k <= 0 || (m->d_edge && m->edge_k == k)) return QK_OK;
  if (m->d_edge || m->d_edge_offs) HIP_TRY(hipStreamSynchronize(c->stream));  // (a plan with another k: the old blocks may still be read)
  m->d_edge.reset(), m->d_edge_offs.reset(), m->edge_k = 0, m->edge_bytes = 0;
  const int n = m->n_sites, stride = n + 1;
  std::vector<long long>& offs = m->h_edge_offs;
  offs.assign((size_t)m->n_states * 2, 0);
  long long total = 0;
  int maxld = 16;
  for (int s_ = 0; s_ < m->n_states; ++s_) {
    const int32_t* d = m->dims_true.data() + (size_t)s_ * stride;
    offs[(size_t)2 * s_] = total;
    total += (long long)(1 << k) * pad16(d[k]);
    offs[(size_t)2 * s_ + 1] = total;
    total += (long long)(1 << k) * pad16(d[n - k]);
    for (int jj = 0; jj <= k; ++jj) maxld = std::max(maxld, std::max(pad16(d[jj]), pad16(d[n - jj])));
  }
  const long long tmp_elems = (long long)std::max(1 << (k - 1), 16) * maxld;  // the largest intermediate block (at least one 16-row tile)
  const int grid = (int)std::min<long long>(2ll * m->n_states, 4ll * c->num_cus);
  const size_t tmp_bytes = (size_t)grid * 2 * tmp_elems * 2 * sizeof(double);
  if (tmp_bytes > c->derive_tmp.bytes) HIP_TRY(hipStreamSynchronize(c->stream));  // (the old one may still be in use)
  HIP_TRY(c->derive_tmp.ensure(tmp_bytes));
  QkDevBuf eb, ob;
  HIP_TRY(eb.alloc((size_t)total * 2 * sizeof(double)));
  HIP_TRY(ob.alloc(offs.size() * sizeof(long long)));
  HIP_TRY(hipMemcpyAsync(ob.get(), offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  qk_edge_kernel<<<dim3(grid), dim3(256), 0, c->stream>>>(m->d_il.get<qk_v2d>(), m->d_dims.get<int32_t>(), m->d_true.get<int32_t>(), m->d_offs.get<int64_t>(), n, k, m->n_states, eb.get<qk_v2d>(),
                                                          ob.get<long long>(), c->derive_tmp.get<qk_v2d>(), tmp_elems);
  HIP_TRY(hipGetLastError());
  m->d_edge = std::move(eb), m->d_edge_offs = std::move(ob);
  m->edge_k = k, m->edge_bytes = total * 2 * (long long)sizeof(double);
  return QK_OK;
}

static void free_merged(qk_mps_set* m) {
  m->d_mg.reset(), m->d_mg_offs.reset(), m->d_mg_units.reset(), m->mg_k = -1, m->mg_steps = 0, m->mg_stride = 0, m->mg_bytes = 0;
}

// the merged image of a set for a chain that starts `k` sites in (made once per set and k; fp64 sets; needs the interleaved image):
// every start (stride 1) or the even starts only (stride 2).  An image of every start serves a call that asks for the even ones; when
// the image of every start does not fit the device, the set gets the even starts (the caller then restricts the segmentation to them).
// Asynchronous like ensure_edges.
static int ensure_merged(qk_ctx* c, qk_mps_set* m, const int k, int stride) {
  if (m->mg_full_failed) stride = 2;
  if (m->d_mg && m->mg_k == k && m->mg_stride <= stride) return QK_OK;
  if (m->d_mg) HIP_TRY(hipStreamSynchronize(c->stream));
  free_merged(m);
  const int n = m->n_sites, n1 = n + 1, starts = n - 2 * k - 1;
  if (starts < 1) return fail(QK_EINVAL, "ensure_merged: a chain of %d sites", n - 2 * k);
  std::vector<int64_t>& mo = m->h_mg_offs;
  std::vector<long long>& us = m->h_mg_units;
  QkDevBuf ib, ob, ub;
  int steps = 0;
  long long total = 0, units = 0;  // complex elements; 16 x 16 blocks (with their four physical combinations)
  for (;; stride = 2) {
    steps = (starts + stride - 1) / stride;
    mo.assign((size_t)m->n_states * starts, 0);
    us.assign((size_t)m->n_states * steps + 1, 0);
    total = units = 0;
    for (int s_ = 0; s_ < m->n_states; ++s_) {
      const int32_t* d = m->dims_true.data() + (size_t)s_ * n1;
      for (int t = 0; t < steps; ++t) {
        const long long lp = pad16(d[k + stride * t]), rp = pad16(d[k + stride * t + 2]);
        mo[(size_t)s_ * starts + stride * t] = 2 * total;
        us[(size_t)s_ * steps + t] = units;
        total += 4ll * lp * rp;
        units += (lp / 16) * (rp / 16);
      }
    }
    us.back() = units;
    if (ib.alloc((size_t)total * 2 * sizeof(double)) == hipSuccess) break;
    (void)hipGetLastError();  // (the failed allocation's sticky error)
    if (stride == 2) return fail(QK_EDEVICE, "ensure_merged: no device memory for %lld bytes of merged steps", total * 2 * (long long)sizeof(double));
    m->mg_full_failed = true;
  }
  HIP_TRY(ob.alloc(mo.size() * sizeof(int64_t)));
  HIP_TRY(ub.alloc(us.size() * sizeof(long long)));
  HIP_TRY(hipMemcpyAsync(ob.get(), mo.data(), mo.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(ub.get(), us.data(), us.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  const long long tasks = (long long)m->n_states * steps;
  const unsigned grid = (unsigned)std::min<long long>((units + 3) / 4, 4ll * c->num_cus);  // 4 wavefronts per workgroup, two workgroups per SIMD row
  qk_merge_kernel<<<dim3(grid), dim3(256), 0, c->stream>>>(m->d_il.get<qk_v2d>(), m->d_dims.get<int32_t>(), m->d_true.get<int32_t>(), m->d_offs.get<int64_t>(), n, k, steps, stride, starts, tasks,
                                                          ub.get<long long>(), ib.get<qk_v2d>(), ob.get<int64_t>());
  HIP_TRY(hipGetLastError());
  m->d_mg = std::move(ib), m->d_mg_offs = std::move(ob), m->d_mg_units = std::move(ub);
  m->mg_k = k, m->mg_steps = starts, m->mg_stride = stride, m->mg_bytes = total * 2 * (long long)sizeof(double);
  return QK_OK;
}

static int ensure_plan_uploaded(qk_ctx* c, qk_plan* p) {
  if (p->d_pairs && p->up_ctx == c) return QK_OK;
  if (p->d_pairs) (void)hipFree(p->d_pairs);
  if (p->d_groups) (void)hipFree(p->d_groups);
  if (p->d_seg) (void)hipFree(p->d_seg);
  p->d_pairs = nullptr, p->d_groups = nullptr, p->d_seg = nullptr, p->up_ctx = nullptr;
  if (p->pairs.empty()) return QK_OK;
  QkDevBuf pairs, groups;  // published together, once both copies are on the device (the plan keeps raw pointers: qk_plan.h has no HIP type)
  HIP_TRY(pairs.alloc(p->pairs.size() * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(pairs.get(), p->pairs.data(), p->pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(groups.alloc(p->groups.size() * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(groups.get(), p->groups.data(), p->groups.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  p->d_pairs = static_cast<int32_t*>(pairs.release()), p->d_groups = static_cast<int32_t*>(groups.release()), p->up_ctx = c;
  return QK_OK;
}

// the site-fused sweep's derived images of the two sets (edge blocks, merged steps) as the plan asks for them, into the launch's arguments
static int derive_fused_images(qk_ctx* c, const qk_mps_set* xs, const qk_mps_set* ys, const qk_plan* plan, const int merge_mode, SweepArgs& a) {
  // the ends of the chain from the sets' edge blocks: k chosen by the planner -- unless a set already holds blocks for another k
  // (made for an earlier plan, e.g. the training Gram before the test Gram on the same X): any k gives the same overlaps and the
  // model's choices lie within 0.5 % of each other, so the set keeps the k of its first use instead of being rebuilt per call
  int ek = plan->edge_k, rc = QK_OK;
  if (ek > 0) {
    if (xs->edge_k > 0 && (ys == xs || ys->edge_k == 0 || ys->edge_k == xs->edge_k)) ek = xs->edge_k;
    else if (xs->edge_k == 0 && ys->edge_k > 0) ek = ys->edge_k;
    for (const qk_mps_set* m : {xs, ys})
      if ((rc = ensure_edges(c, const_cast<qk_mps_set*>(m), ek)) != QK_OK) return rc;
    a.xedge = xs->d_edge.get<double>(), a.xedge_offs = xs->d_edge_offs.get<long long>(), a.yedge = ys->d_edge.get<double>(), a.yedge_offs = ys->d_edge_offs.get<long long>(), a.edge_k = ek;
  }
  if (merge_mode > 0 && xs->n_sites - 2 * ek >= 2) {  // neighbouring sites of the chain contracted in twos: the pair's mask says which steps walk them (ensure_segments)
    for (const qk_mps_set* m : {xs, ys})
      if ((rc = ensure_merged(c, const_cast<qk_mps_set*>(m), ek, merge_mode >= 2 ? 1 : 2)) != QK_OK) return rc;
    a.xmg = xs->d_mg.get<double>(), a.xmg_offs = xs->d_mg_offs.get<int64_t>(), a.ymg = ys->d_mg.get<double>(), a.ymg_offs = ys->d_mg_offs.get<int64_t>(), a.merge_steps = xs->mg_steps;
  }
#ifdef QK_LAB  // TIMING EXPERIMENT (wrong results): every tensor read from the first MiB of its image -- what would perfect L2 hits buy?
  if (const char* v = std::getenv("QK_DEBUG_ALIAS")) {
    const long long win = std::atoll(v);  // window in doubles (e.g. 131072 = 1 MiB)
    if (win > 0) {
      auto fold = [&](const int64_t* src, const long long n) -> const int64_t* {
        QkDevBuf buf;
        if (buf.alloc((size_t)n * sizeof(int64_t)) != hipSuccess) return src;
        int64_t* dst = static_cast<int64_t*>(buf.release());  // (leaked: experiment)
        qk_lab_fold_kernel<<<dim3(256), dim3(256), 0, c->stream>>>(src, dst, n, win);
        return dst;
      };
      a.xoffs = fold(a.xoffs, (long long)xs->n_states * xs->n_sites), a.yoffs = fold(a.yoffs, (long long)ys->n_states * ys->n_sites);
      if (a.merge_steps > 0)
        a.xmg_offs = fold(a.xmg_offs, (long long)xs->n_states * xs->mg_steps), a.ymg_offs = fold(a.ymg_offs, (long long)ys->n_states * ys->mg_steps);
    }
  }
#endif
  return QK_OK;
}

// the shape of a site-fused launch as the segmentation sees it (cap 0: not a site-fused kernel)
static QkSegRule seg_rule_of(const int kernel) {
  switch (kernel) {
    case QK_KERNEL_FUSED1: case QK_KERNEL_FUSED1_DET: return {QKF_XCAP_ONE, QKF_ONE_NW * QKF_ONE_S, false};
    case QK_KERNEL_FUSED2: case QK_KERNEL_FUSED2_DET: return {QKF_XCAP_TWO, QKF_TWO_NW * QKF_TWO_S, false};
#if QKF_QUAD
    case QK_KERNEL_FUSED_DUAL: return {QKF_XCAP_ONE, QKF_QUAD_NW, true};
#else
    case QK_KERNEL_FUSED_DUAL: return {QKF_XCAP_ONE, QKF_DUAL_NW, true};
#endif
    case QK_KERNEL_FUSED_DUAL_DET: return {QKF_XCAP_ONE, QKF_DUAL_NW, true};
    default: return {0, 0, false};
  }
}

// whether a launch's kernel has the switch step (qk_fused.h: qkf_p2_switch): the plain forms of the shipped site-fused kernels.  The masks
// of any other launch are made with orientation 0 throughout.
static bool seg_assoc_of(const int kernel) {
#if QKF_QUAD  // (lab builds: the quad form stands in for the plain dual form and has no switch step)
  if (kernel == QK_KERNEL_FUSED_DUAL) return false;
#endif
  return kernel == QK_KERNEL_FUSED_DUAL || kernel == QK_KERNEL_FUSED1 || kernel == QK_KERNEL_FUSED2;
}

// the segmentation masks of the plan's pairs for the launches of `ch` (a.merge_steps > 0: the sets hold merged images for a.edge_k), into
// a.seg.  Made on the sweep's stream by qk_segment_kernel, one launch per site-fused run with that run's shape, and kept in the plan: a
// later call with the same sets, edge_k, rule, launches, QK_ASSOC and switch price finds them there.
static int ensure_segments(qk_ctx* c, const qk_mps_set* xs, const qk_mps_set* ys, qk_plan* plan, const QkSweepChoice& ch, const int merge_mode, SweepArgs& a) {
  const long long np = (long long)plan->pairs.size() / 2;
  const bool both = merge_mode >= 2 && xs->mg_stride == 1 && ys->mg_stride == 1;  // else the even starts only: QK_MERGE=1, or a set without the image of every start
  const int assoc = merge_mode >= 2 ? c->policy.assoc_mode : 0, switch_price = c->policy.switch_price;  // (the orientations are chosen by the programme that chooses the merges)
  const unsigned long long key[8] = {2ull | ((unsigned long long)assoc << 8) | ((unsigned long long)switch_price << 16),
                                     xs->uid,
                                     ys->uid,
                                     (unsigned long long)a.edge_k,
                                     both ? 3ull : 1ull,
                                     merge_mode == 1 ? 1ull : 0ull,
                                     (unsigned long long)ch.run[0].kernel | ((unsigned long long)(ch.n_runs > 1 ? ch.run[1].kernel : 0) << 32),
                                     (unsigned long long)ch.run[0].count};
  if (plan->d_seg && std::equal(key, key + 8, plan->seg_key)) return a.seg = plan->d_seg, QK_OK;
  if (plan->d_seg) {
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a sweep may still read the old masks)
    (void)hipFree(plan->d_seg), plan->d_seg = nullptr;
  }
  QkDevBuf seg;
  HIP_TRY(seg.alloc((size_t)np * 4 * sizeof(unsigned long long)));
  unsigned long long* const d = seg.get<unsigned long long>();
  for (int i = 0; i < ch.n_runs; ++i) {
    const QkSweepRun& r = ch.run[i];
    const QkSegRule rule = seg_rule_of(r.kernel);
    if (r.count <= 0) continue;
    if (rule.cap == 0) {  // (the one-wave launch of a mixed sweep reads no mask)
      HIP_TRY(hipMemsetAsync(d + 4 * r.first, 0, (size_t)r.count * 4 * sizeof(unsigned long long), c->stream));
      continue;
    }
    qk_segment_kernel<<<dim3((unsigned)((r.count + 255) / 256)), dim3(256), 0, c->stream>>>(a.xdims, a.xtrue, a.ydims, a.ytrue, a.n_sites, a.edge_k, a.pairs + 2 * r.first, r.count, rule, both ? 3 : 1,
                                                                                            merge_mode == 1, seg_assoc_of(r.kernel) ? assoc : 0, switch_price, d + 4 * r.first);
  }
  HIP_TRY(hipGetLastError());
  plan->d_seg = static_cast<unsigned long long*>(seg.release());
  std::copy(key, key + 8, plan->seg_key);
  a.seg = plan->d_seg;
  return QK_OK;
}

// one launch of a product sweep kernel (QK_KERNEL_*; f32: the set's planes are complex64) with `lds` bytes of dynamic LDS.  big: the choice
// (qk_plan.h: qk_choose_sweep) gave a 12-wave site-fused launch the instantiation with QKF_RCAP_ONE elements -- the same plan, masks and step
// table, more steps with X and X' side by side (qk_resident) -- and `lds` is sized for it.
static int launch_sweep(const int kernel, const bool f32, const long long grid_, const size_t lds, const hipStream_t s, const SweepArgs& a, const bool big) {
  const dim3 grid((unsigned)grid_);
  if (big) {
    const size_t lds_big = lds;
    switch (kernel) {
      case QK_KERNEL_FUSED1: QKF_KERNEL_ONE_BIG<<<grid, dim3(64 * QKF_ONE_NW), lds_big, s>>>(a); return QK_OK;
      case QK_KERNEL_FUSED1_DET: QKF_KERNEL_ONE_DET_BIG<<<grid, dim3(64 * QKF_ONE_NW), lds_big, s>>>(a); return QK_OK;
#if !QKF_QUAD
      case QK_KERNEL_FUSED_DUAL: QKF_KERNEL_DUAL_BIG<<<grid, dim3(64 * QKF_DUAL_NW), lds_big, s>>>(a); return QK_OK;
#endif
      case QK_KERNEL_FUSED_DUAL_DET: QKF_KERNEL_DUAL_DET_BIG<<<grid, dim3(64 * QKF_DUAL_NW), lds_big, s>>>(a); return QK_OK;
      default: return fail(QK_EINVAL, "qk_gram_values: kernel %d has no instantiation with the large X buffer", kernel);
    }
  }
  switch (kernel) {
    case QK_KERNEL_WAVE: qk_sweep_wave_kernel<0><<<grid, dim3(64), lds, s>>>(a); break;
    case QK_KERNEL_WAVE2: if (f32) qk_sweep_wave2_kernel<3, float><<<grid, dim3(64), lds, s>>>(a); else qk_sweep_wave2_kernel<3, double><<<grid, dim3(64), lds, s>>>(a); break;  // (an fp32 set: complex64 storage, fp64 arithmetic)
    case QK_KERNEL_WAVE2_PLAIN: qk_sweep_wave2_kernel<0, double><<<grid, dim3(64), lds, s>>>(a); break;
    case QK_KERNEL_SMALL: if (f32) qk_sweep_small_kernel<float><<<grid, dim3(512), lds, s>>>(a); else qk_sweep_small_kernel<double><<<grid, dim3(512), lds, s>>>(a); break;
    case QK_KERNEL_RING: if (f32) qk_sweep_ring_kernel<float><<<grid, dim3(512), lds, s>>>(a); else qk_sweep_ring_kernel<double><<<grid, dim3(512), lds, s>>>(a); break;  // (complex64 sweep of an fp32 set: SURVEY 8f N4)
    case QK_KERNEL_FUSED1: QKF_KERNEL_ONE<<<grid, dim3(64 * QKF_ONE_NW), lds, s>>>(a); break;
    case QK_KERNEL_FUSED1_DET: QKF_KERNEL_ONE_DET<<<grid, dim3(64 * QKF_ONE_NW), lds, s>>>(a); break;
    case QK_KERNEL_FUSED2: QKF_KERNEL_TWO<<<grid, dim3(64 * QKF_TWO_NW), lds, s>>>(a); break;
    case QK_KERNEL_FUSED2_DET: QKF_KERNEL_TWO_DET<<<grid, dim3(64 * QKF_TWO_NW), lds, s>>>(a); break;
#if QKF_QUAD  // lab builds: the quad form stands in for the plain dual form
    case QK_KERNEL_FUSED_DUAL: QKF_KERNEL_QUAD<<<grid, dim3(64 * QKF_QUAD_NW), lds, s>>>(a); break;
#else
    case QK_KERNEL_FUSED_DUAL: QKF_KERNEL_DUAL<<<grid, dim3(64 * QKF_DUAL_NW), lds, s>>>(a); break;
#endif
    case QK_KERNEL_FUSED_DUAL_DET: QKF_KERNEL_DUAL_DET<<<grid, dim3(64 * QKF_DUAL_NW), lds, s>>>(a); break;
    default: return fail(QK_EINVAL, "qk_gram_values: no kernel for this call");
  }
  return QK_OK;
}

extern "C" int qk_gram_values(qk_ctx* c, const qk_mps_set* xs, const qk_mps_set* ys, const qk_plan* plan_c, double* values_dev, double* z_dev) {
  if (!c || !xs || !plan_c || !values_dev) return fail(QK_EINVAL, "qk_gram_values: null argument");
  qk_plan* plan = const_cast<qk_plan*>(plan_c);
  if (!ys) ys = xs;
  if (xs->ctx != c || ys->ctx != c) return fail(QK_EINVAL, "qk_gram_values: sets belong to another context");
  if (xs->n_sites != ys->n_sites || xs->n_sites != plan->n_sites) return fail(QK_EINVAL, "qk_gram_values: site counts differ (%d, %d, plan %d)", xs->n_sites, ys->n_sites, plan->n_sites);
  if (plan->nx != xs->n_states || plan->ny != ys->n_states) return fail(QK_EINVAL, "qk_gram_values: plan is for %dx%d states, sets hold %dx%d", plan->nx, plan->ny, xs->n_states, ys->n_states);
  QkRangeGuard range_("qk:sweep");
  HIP_TRY(hipSetDevice(c->device));
  const long long np = (long long)plan->pairs.size() / 2;
  c->last = plan->stats;
  c->split_pending = c->tail_pending = false;
  c->last.max_bond = std::max(xs->max_pad, ys->max_pad);
  c->last.kernel_ms = 0, c->last.grid = 0, c->last.kernel = QK_KERNEL_NONE, c->last.precision = xs->precision;
  if (np == 0) return QK_OK;
  int rc = ensure_plan_uploaded(c, plan);
  if (rc != QK_OK) return rc;
  if (xs->precision != ys->precision) return fail(QK_EINVAL, "qk_gram_values: the two sets differ in precision (fp%d, fp%d)", xs->precision, ys->precision);
  const bool f32 = (xs->precision == 32);
  if (f32) c->last.bytes *= 0.5;  // complex64 planes

  QkSweepPolicy pol = c->policy;  // three of the switches are read per call
  if (const char* v = std::getenv("QK_FUSED_DUAL")) pol.fused_dual = std::atoi(v) != 0;
  if (const char* v = std::getenv("QK_FUSED_BIG")) pol.fused_big = std::atoi(v) != 0;
  if (const char* v = std::getenv("QK_GANG")) pol.gang = std::atoi(v) != 0;
  const QkSweepChoice ch = qk_choose_sweep(pol, *plan, {xs->max_pad, xs->precision, xs->n_sites}, {ys->max_pad, ys->precision, ys->n_sites}, c->num_cus);
  if (ch.rc != QK_OK) return fail(ch.rc, "%s", ch.err);
  c->last.queues = ch.queues, c->last.tail_frac = c->last.second_tail_frac = 0;
  if (ch.scratch_bytes > c->scratch.bytes) HIP_TRY(hipStreamSynchronize(c->stream));  // (the old one may still be in use)
  HIP_TRY(c->scratch.ensure(ch.scratch_bytes));
  SweepArgs a{};  // (what is not set here is null / zero)
  a.xdata = xs->d_data.get<double>(), a.xdims = xs->d_dims.get<int32_t>(), a.xtrue = xs->d_true.get<int32_t>(), a.xoffs = xs->d_offs.get<int64_t>();
  a.ydata = ys->d_data.get<double>(), a.ydims = ys->d_dims.get<int32_t>(), a.ytrue = ys->d_true.get<int32_t>(), a.yoffs = ys->d_offs.get<int64_t>();
  a.n_sites = xs->n_sites;
  a.pairs = plan->d_pairs, a.npairs = np;
  a.groups = plan->d_groups, a.ngroups = (long long)plan->groups.size() / 2;
  a.values = values_dev, a.z = z_dev;
  a.scratch = c->scratch.get<double>(), a.x_plane = ch.x_plane, a.t_plane = ch.t_plane, a.turn_ints = ch.turn_ints;
  unsigned long long* const counter = c->counter.get<unsigned long long>();
  a.counter = counter, a.prof = c->prof.get<unsigned long long>();
  for (int s_ = 0; s_ <= QK_NQ_MAX; ++s_) a.qstart[s_] = plan->nq > 1 ? plan->qstart[s_] : (s_ == 0 ? 0 : np);
  // device clocks for the tail accounting behind the queue heads (launch 1 uses [0] [1] [4], launch 2 [2] [3] [6]), the DET error word, the gang words
  a.tail = counter + QK_NQ_MAX * QK_QSTRIDE, a.err = a.tail + 7, a.gang = a.tail + 8;
#ifdef QK_LAB  // timing experiments of the lab kernels (they give wrong results by construction): libqklab.so only
  if (const char* v = std::getenv("QK_DEBUG_FLAGS")) a.debug_flags = std::atoi(v);
  if (const char* v = std::getenv("QK_PRIO")) a.prio_mode = std::atoi(v);
#endif
  HIP_TRY(hipEventRecord(c->ev_d, c->stream));
  HIP_TRY(hipMemsetAsync(counter, 0, (QK_NQ_MAX * QK_QSTRIDE + 8 + 2 * 8 * QK_QSTRIDE) * sizeof(unsigned long long), c->stream));
  HIP_TRY(hipMemsetAsync(a.tail, 0xFF, 4 * sizeof(unsigned long long), c->stream));  // the four minima
  // the sets' derived images (made on their first use): between ev_d and ev0, not part of the sweep
  if (ch.interleaved) {
    for (const qk_mps_set* m : {xs, ys})
      if ((rc = ensure_interleaved(c, const_cast<qk_mps_set*>(m))) != QK_OK) return rc;
    a.xdata = xs->d_il.get<double>(), a.ydata = ys->d_il.get<double>();
  }
  if (ch.fused_images && (rc = derive_fused_images(c, xs, ys, plan, pol.merge_mode, a)) != QK_OK) return rc;
  if (a.merge_steps > 0 && (rc = ensure_segments(c, xs, ys, plan, ch, pol.merge_mode, a)) != QK_OK) return rc;
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  for (int i = 0; i < ch.n_runs; ++i) {
    const QkSweepRun& r = ch.run[i];
    SweepArgs ar = a;
    ar.npairs = r.count, ar.nq = r.nq, ar.gang_n = r.gang_n;
    if (i == 1) {  // the second class of pairs: its part of the list, and queue heads, tail clocks (and gang words) behind the first launch's
      HIP_TRY(hipEventRecord(c->ev_mid, c->stream));
      ar.pairs = a.pairs + 2 * r.first, ar.values = a.values + r.first, ar.z = a.z ? a.z + 2 * r.first : nullptr, ar.seg = a.seg ? a.seg + 4 * r.first : nullptr;
      ar.counter = counter + 8 * QK_QSTRIDE, ar.tail = a.tail + 2;
      if (plan->nq > 1)
        for (int s_ = 0; s_ <= 8; ++s_) ar.qstart[s_] = plan->qstart[8 + s_] - r.first;
      if (r.gang2) ar.gang = a.gang + 8 * QK_QSTRIDE;
      c->last.second_pairs = plan->second.pairs, c->last.second_flops = plan->second.flops, c->last.second_padded_flops = plan->second.padded_flops;
      c->last.second_bytes = plan->second.bytes, c->last.second_kernel = r.kernel;
      c->split_pending = true;
    }
#ifdef QK_LAB
    if (r.kernel == QK_KERNEL_LAB) rc = plan->quad ? qk_lab_launch_quad(c, ar, (int)r.grid, xs->n_sites, f32) : qk_lab_launch(c, pol.variant, ar, (int)r.grid, xs->n_sites);
    else
#endif
      rc = launch_sweep(r.kernel, f32, r.grid, r.lds_launch, c->stream, ar, r.big);
    if (rc != QK_OK) return rc;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  c->ev_pending = true;
  c->last.lds_bytes = (int32_t)ch.run[0].lds_launch, c->last.second_lds_bytes = ch.n_runs > 1 ? (int32_t)ch.run[1].lds_launch : 0;
  c->last.kernel = ch.run[0].kernel, c->last.grid = (int)ch.launched_grid;
  c->tail_pending = ch.tails;
  return QK_OK;
}

extern "C" int qk_gram_values_host(qk_ctx* c, const qk_mps_set* xs, const qk_mps_set* ys, const qk_plan* plan, double* values_host, double* z_host) {
  if (!c || !plan || !values_host) return fail(QK_EINVAL, "qk_gram_values_host: null argument");
  const int64_t np = qk_plan_num_pairs(plan);
  if (np == 0) return QK_OK;
  HIP_TRY(hipSetDevice(c->device));
  QkDevBuf vals, z;  // released on every exit path
  HIP_TRY(vals.alloc((size_t)np * sizeof(double)));
  if (z_host) HIP_TRY(z.alloc((size_t)np * 2 * sizeof(double)));
  const int rc = qk_gram_values(c, xs, ys, plan, vals.get<double>(), z.get<double>());
  if (rc != QK_OK) return rc;
  HIP_TRY(hipMemcpyAsync(values_host, vals.get(), (size_t)np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (z_host) HIP_TRY(hipMemcpyAsync(z_host, z.get(), (size_t)np * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QK_OK;
}

extern "C" int qk_scatter(qk_ctx* c, const int32_t* pairs_dev, const double* values_dev, int64_t n, double* k_dev, int64_t ld, int32_t mirror) {
  if (!c || !pairs_dev || !values_dev || !k_dev) return fail(QK_EINVAL, "qk_scatter: null argument");
  if (n <= 0) return QK_OK;
  QkRangeGuard range_("qk:scatter");
  HIP_TRY(hipSetDevice(c->device));
  const int bs = 256;
  hipLaunchKernelGGL(qk_scatter_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, c->stream, pairs_dev, values_dev, (long long)n, k_dev, (long long)ld, (int)mirror);
  HIP_TRY(hipGetLastError());
  return QK_OK;
}

extern "C" const char* qk_kernel_name(int32_t kernel, int32_t precision) {
  const bool f32 = precision == 32;
  switch (kernel) {
    case QK_KERNEL_WAVE: return "qk_sweep_wave_kernel<0>";
    case QK_KERNEL_SMALL: return f32 ? "qk_sweep_small_kernel<float>" : "qk_sweep_small_kernel<double>";
    case QK_KERNEL_FUSED1: return "qk_sweep_fused_kernel<12, 2, 8192, 3, false>";
    case QK_KERNEL_FUSED2: return "qk_sweep_fused_kernel<8, 1, 4608, 4, false>";
    case QK_KERNEL_FUSED1_DET: return "qk_sweep_fused_kernel<12, 2, 8192, 3, true>";
    case QK_KERNEL_FUSED2_DET: return "qk_sweep_fused_kernel<8, 1, 4608, 4, true>";
    case QK_KERNEL_FUSED_DUAL_DET: return "qk_sweep_fused_dual_kernel<12, 8192, 3, true>";
    case QK_KERNEL_RING: return f32 ? "qk_sweep_ring_kernel<float>" : "qk_sweep_ring_kernel<double>";
    case QK_KERNEL_WAVE2: return precision == 32 ? "qk_sweep_wave2_kernel<3, float>" : "qk_sweep_wave2_kernel<3, double>";
    case QK_KERNEL_WAVE2_PLAIN: return "qk_sweep_wave2_kernel<0, double>";
    case QK_KERNEL_FUSED_DUAL: return "qk_sweep_fused_dual_kernel<12, 8192, 3, false>";
    case QK_KERNEL_LAB: return "(lab kernel)";
    default: return "(none)";
  }
}
#ifndef QKF_EXPERIMENT
static_assert(QKF_ONE_NW == 12 && QKF_ONE_S == 2 && QKF_ONE_WPS == 3 && QKF_TWO_NW == 8 && QKF_TWO_S == 1 && QKF_TWO_WPS == 4 && QKF_XCAP_ONE == 8192 && QKF_XCAP_TWO == 4608,
              "qk_kernel_name spells the fused sweep's template arguments");
#endif

extern "C" int qk_get_stats(qk_ctx* c, qk_stats* out) {
  if (!c || !out) return fail(QK_EINVAL, "qk_get_stats: null argument");
  if (c->ev_pending) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last.kernel_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_d, c->ev0));
    c->last.derive_ms = ms;  // device time ahead of the sweep: the derived images of the sets (interleaved, edge blocks, merged steps) on their first Gram
    if (c->tail_pending) {  // device clocks of the launch(es): share of the duration during which the chip was draining
      unsigned long long t[8];
      HIP_TRY(hipMemcpy(t, c->counter.get<unsigned long long>() + QK_NQ_MAX * QK_QSTRIDE, sizeof t, hipMemcpyDeviceToHost));
      auto frac = [](const unsigned long long start, const unsigned long long first_exit, const unsigned long long last_exit) {
        return (last_exit > start && first_exit <= last_exit && first_exit >= start) ? (double)(last_exit - first_exit) / (double)(last_exit - start) : 0.0;
      };
      if (t[7] != 0) return fail(QK_EDEVICE, "qk_get_stats: the ordered accumulation of the last sweep ran out of patience (a bug: please report); its results are not valid");
      c->last.tail_frac = frac(t[0], t[1], t[4]);
      if (c->split_pending) c->last.second_tail_frac = frac(t[2], t[3], t[6]);
      c->tail_pending = false;
    }
    if (c->split_pending) {
      HIP_TRY(hipEventElapsedTime(&ms, c->ev_mid, c->ev1));
      c->last.second_ms = ms;
      c->split_pending = false;
    }
    c->ev_pending = false;
#ifdef QKF_PROF  // experiment builds: the section sums of the launch(es) since the last call (wave cycles, all waves)
    {
      unsigned long long pf[8];
      HIP_TRY(hipMemcpy(pf, c->prof.get(), sizeof pf, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemset(c->prof.get(), 0, sizeof pf));
      const double tot = pf[7] > 0 ? (double)pf[7] : 1.0;
      fprintf(stderr, "[qkf_prof] pair set-up %.3f  step set-up %.3f  phase1 %.3f  wait1 %.3f  phase2 %.3f  wait2 %.3f  tail %.3f  (of %.3e wave cycles)\n", pf[0] / tot, pf[1] / tot, pf[2] / tot,
              pf[3] / tot, pf[4] / tot, pf[5] / tot, pf[6] / tot, tot);
    }
#endif
  }
  *out = c->last;
  return QK_OK;
}

// dims table of a set as the planner wants it
static int plan_for_sets(const qk_mps_set* xs, const qk_mps_set* ys, qk_plan** plan) {
  const bool sym = (ys == nullptr || ys == xs);
  return qk_plan_create(xs->n_sites, xs->n_states, xs->dims_true.data(), sym ? xs->n_states : ys->n_states,
                        sym ? nullptr : ys->dims_true.data(), sym ? (QK_PLAN_SYMMETRIC | QK_PLAN_ORIENT) : 0u, 1, 0, 0, plan);
}

struct PlanGuard {  // a plan owned by one call
  qk_plan* p = nullptr;
  ~PlanGuard() { qk_plan_destroy(p); }
};

extern "C" int qk_gram_host(qk_ctx* c, const qk_mps_set* xs, const qk_mps_set* ys, double* out, int64_t ld) {
  if (!c || !xs || !out) return fail(QK_EINVAL, "qk_gram_host: null argument");
  const bool sym = (ys == nullptr || ys == xs);
  const int nx = xs->n_states, ny = sym ? nx : ys->n_states;
  if (ld < nx) return fail(QK_EINVAL, "qk_gram_host: ld %lld < %d columns", (long long)ld, nx);
  PlanGuard plan;
  int rc = plan_for_sets(xs, ys, &plan.p);
  if (rc != QK_OK) return rc;
  const int64_t np = qk_plan_num_pairs(plan.p);
  QkDevBuf vals, k;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(vals.alloc((size_t)np * sizeof(double)));
  HIP_TRY(k.alloc((size_t)ny * nx * sizeof(double)));
  HIP_TRY(hipMemsetAsync(k.get(), 0, (size_t)ny * nx * sizeof(double), c->stream));
  rc = qk_gram_values(c, xs, ys, plan.p, vals.get<double>(), nullptr);
  if (rc == QK_OK) rc = qk_scatter(c, plan.p->d_pairs, vals.get<double>(), np, k.get<double>(), nx, sym ? 1 : 0);
  if (rc != QK_OK) return rc;
  HIP_TRY(hipMemcpy2DAsync(out, (size_t)ld * sizeof(double), k.get(), (size_t)nx * sizeof(double), (size_t)nx * sizeof(double), (size_t)ny, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QK_OK;
}

extern "C" int qk_overlaps_host(qk_ctx* c, const qk_mps_set* xs, const qk_mps_set* ys, double* out) {
  if (!c || !xs || !out) return fail(QK_EINVAL, "qk_overlaps_host: null argument");
  if (!ys) ys = xs;
  const int nx = xs->n_states, ny = ys->n_states;
  PlanGuard plan;  // all ny*nx pairs (no symmetry: z[i][j] = conj z[j][i] is left to the caller)
  int rc = qk_plan_create(xs->n_sites, nx, xs->dims_true.data(), ny, ys->dims_true.data(), 0u, 1, 0, 16, &plan.p);
  if (rc != QK_OK) return rc;
  const int64_t np = qk_plan_num_pairs(plan.p);
  QkDevBuf vals, zd;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(vals.alloc((size_t)np * sizeof(double)));
  HIP_TRY(zd.alloc((size_t)np * 2 * sizeof(double)));
  rc = qk_gram_values(c, xs, ys, plan.p, vals.get<double>(), zd.get<double>());
  if (rc != QK_OK) return rc;
  std::vector<double> z((size_t)np * 2);
  HIP_TRY(hipMemcpyAsync(z.data(), zd.get(), z.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int32_t* pr = qk_plan_pairs(plan.p);
  for (int64_t t = 0; t < np; ++t) {
    const int64_t o = ((int64_t)pr[2 * t + 1] * nx + pr[2 * t]) * 2;
    out[o] = z[2 * t], out[o + 1] = z[2 * t + 1];
  }
  return QK_OK;
}

extern "C" int qk_selftest_mfma(qk_ctx* c) {
  if (!c) return fail(QK_EINVAL, "qk_selftest_mfma: null context");
  HIP_TRY(hipSetDevice(c->device));
  double hp[256], hq[256], hc[256], ref[256];
  for (int k = 0; k < 16; ++k)
    for (int m = 0; m < 16; ++m) {
      hp[k * 16 + m] = 1.0 + 0.25 * k - 0.5 * m + 0.125 * ((k * 7 + m * 3) % 5);  // asymmetric on purpose
      hq[k * 16 + m] = -2.0 + 0.5 * k + 0.75 * m - 0.25 * ((k * 5 + m * 11) % 7);
    }
  for (int m = 0; m < 16; ++m)
    for (int n = 0; n < 16; ++n) {
      double s = 0;
      for (int k = 0; k < 16; ++k) s += hp[k * 16 + m] * hq[k * 16 + n];
      ref[m * 16 + n] = s;
    }
  QkDevBuf bp, bq, bc;
  HIP_TRY(bp.alloc(sizeof hp));
  HIP_TRY(bq.alloc(sizeof hq));
  HIP_TRY(bc.alloc(sizeof hc));
  double *dp = bp.get<double>(), *dq = bq.get<double>(), *dc = bc.get<double>();
  HIP_TRY(hipMemcpy(dp, hp, sizeof hp, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dq, hq, sizeof hq, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(qk_selftest_kernel, dim3(1), dim3(64), 0, c->stream, dp, dq, dc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(hc, dc, sizeof hc, hipMemcpyDeviceToHost));
  double worst = 0;
  for (int e = 0; e < 256; ++e) worst = std::max(worst, std::fabs(hc[e] - ref[e]));
  if (worst > 1e-9) return fail(QK_EDEVICE, "qk_selftest_mfma: f64 MFMA fragment map mismatch (max abs error %.3g)", worst);
  // the same product through v_mfma_f32_16x16x4_f32 (operands are exact in fp32; sums of 16 such products too)
  float fp[256], fq[256], fc[256];
  for (int e = 0; e < 256; ++e) fp[e] = (float)hp[e], fq[e] = (float)hq[e];
  QkDevBuf be, bf, bg;
  HIP_TRY(be.alloc(sizeof fp));
  HIP_TRY(bf.alloc(sizeof fq));
  HIP_TRY(bg.alloc(sizeof fc));
  float *ep = be.get<float>(), *eq = bf.get<float>(), *ec = bg.get<float>();
  HIP_TRY(hipMemcpy(ep, fp, sizeof fp, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(eq, fq, sizeof fq, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(qk_selftest_f32_kernel, dim3(1), dim3(64), 0, c->stream, ep, eq, ec);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(fc, ec, sizeof fc, hipMemcpyDeviceToHost));
  worst = 0;
  for (int e = 0; e < 256; ++e) worst = std::max(worst, std::fabs((double)fc[e] - ref[e]));
  if (worst > 1e-3) return fail(QK_EDEVICE, "qk_selftest_mfma: f32 MFMA fragment map mismatch (max abs error %.3g)", worst);
  return QK_OK;
}

