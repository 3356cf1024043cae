// qk_host.h -- host-side state shared by the translation units:
//   qkgram.hip    the C ABI, the planner and the shipped sweep kernels      } libqkgram.so
//   qk_build.hip  the device MPS builder, the bond spectra's factorisation  }
//   qk_local.hip  local Bloch vectors and the projected-kernel Gram          }
//   qk_comm.hip   the multi-GPU entry points                                 }
//   qk_lab.hip    experimental / diagnostic kernels for A/B measurements: only in lab/libqklab.so (-DQK_LAB, lab/tools)
// Device memory has one kind of owner (qk_devmem.h): a QkDevBuf frees in its destructor, a QkGrowBuf is kept and regrown.  The
// context and the sets below hold their device memory as such members, so no destroy / trim function keeps a list of pointers,
// and a call's temporaries are local QkDevBufs: HIP_TRY may return from anywhere.  Kernels still take raw pointers (get<T>()).
#pragma once
#include "../../include/qkgram.h"
#include "qk_plan.h"

#include <hip/hip_runtime.h>

#include "qk_devmem.h"

#include <cstdint>
#include <vector>

struct QkRangeGuard {  // a roctx range (qk_range_push / qk_range_pop) that closes on every exit path
  explicit QkRangeGuard(const char* n) { qk_range_push(n); }
  ~QkRangeGuard() { qk_range_pop(); }
};

#define HIP_TRY(expr)                                                                                 \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return qk_fail(QK_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));  \
  } while (0)
#define HIP_TRY_AS(what, expr) /* the same, with the entry point's name in front */                             \
  do {                                                                                                          \
    hipError_t e_ = (expr);                                                                                     \
    if (e_ != hipSuccess) return qk_fail(QK_EDEVICE, "%s: %s failed: %s", what, #expr, hipGetErrorString(e_));  \
  } while (0)

struct qk_ctx {
  int device = 0;
  int num_cus = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  bool split_pending = false;  // the last sweep was two launches: second_ms is still to be read from the events
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mid = nullptr;  // ev_mid: between the two launches of a split sweep
  hipEvent_t ev_d = nullptr;  // at the start of qk_gram_values: what runs between it and ev0 are the kernels that make a set's derived images (first Gram of a set)
  bool ev_pending = false;
  QkGrowBuf scratch;  // the sweep's per-workgroup X / T planes, kept between calls (qk_gram_values)
  QkDevBuf counter;   // unsigned long long: work-queue heads (QK_NQ_MAX of them, QK_QSTRIDE apart) + 2 x 4 tail clocks behind them
  bool tail_pending = false;
  QkDevBuf prof;  // unsigned long long: 8 cycle sums of the diagnostic variant
  QkSweepPolicy policy;  // the switches of the sweep's choice of kernels (qk_plan.h), set by ctx_init
  qk_stats last{};
  // the device MPS builder's per-workgroup arena and workspace, kept between calls (qk_build.hip)
  QkGrowBuf build_arena, build_work;
  // scratch of the workgroups that make a set's edge blocks (qk_edge_kernel), kept between calls
  QkGrowBuf derive_tmp;
  // the local sweep's tables, rho partial sums and per-state environments (qk_local.hip), kept between calls
  QkGrowBuf local_scratch;
};

uint64_t qk_next_uid();

struct qk_mps_set {
  qk_ctx* ctx = nullptr;
  uint64_t uid = qk_next_uid();  // unique per set of this process: caches keyed on a set's address also compare this (a freed address may come back)
  int n_states = 0, n_sites = 0, max_pad = 0;
  int precision = 64;         // bits of a real: 64 (complex128 planes) or 32 (complex64 planes, same element offsets)
  QkDevBuf d_data;  // double: the planes; floats when precision == 32
  QkDevBuf d_il;    // double: made on first use by the site-fused sweep: the same image with re/im interleaved (complex128; complex64 of an fp32 set), same offsets
  QkDevBuf d_dims;  // int32_t: padded bonds [n_states][n_sites+1]
  QkDevBuf d_true;  // int32_t: true bonds   [n_states][n_sites+1]
  QkDevBuf d_offs;  // int64_t: re-plane offsets (doubles) [n_states][n_sites]
  std::vector<int32_t> dims_true;
  int centre = -1;  // provenance: the orthogonality centre every state has (a snapshot of the device builder), -1: gauge unknown (every other origin)
  int64_t bytes = 0;
  // edge blocks of the site-fused sweep (made on first use for the plan's edge_k; qk_device.h: SweepArgs.edge_k)
  QkDevBuf d_edge;       // double: interleaved complex: per state the left block [2^k][pad(chi_k)], then the right block [2^k][pad(chi_{n-k})]
  QkDevBuf d_edge_offs;  // long long: [n_states][2] element offsets
  int edge_k = 0;
  int64_t edge_bytes = 0;
  // merged image of the site-fused sweep (SweepArgs.merge_steps; made on first use for the plan's edge_k): neighbouring sites s, s + 1 of
  // the chain [k, n - k) contracted in twos, interleaved complex [l][4][r] -- for every start s (mg_stride 1) or for the even starts
  // s = k + 2 t only (mg_stride 2: QK_MERGE=1, or the full image did not fit the device)
  QkDevBuf d_mg;        // double
  QkDevBuf d_mg_offs;   // int64_t: offsets in doubles [n_states][mg_steps], entry s - k
  QkDevBuf d_mg_units;  // long long: first 16 x 16 block of each (state, start) in the numbering of qk_merge_kernel's units [n_states * starts per state + 1]
  std::vector<long long> h_edge_offs, h_mg_units;  // host staging of the tables above (they outlive the asynchronous copies)
  std::vector<int64_t> h_mg_offs;
  int mg_k = -1, mg_steps = 0, mg_stride = 0;
  bool mg_full_failed = false;  // the image of every start did not fit once: not tried again for this set
  int64_t mg_bytes = 0;
};

// the one allocator of a set (qkgram.hip): the object and its four device arrays (d_data of `data_bytes`, d_dims, d_true, d_offs),
// nothing uploaded.  `who` names the entry point in the error text.  A constructor that fails later calls qk_mps_set_destroy.
int qk_mps_set_alloc(qk_ctx* c, int n_states, int n_sites, int64_t data_bytes, int precision, qk_mps_set** out, const char* who);

// the bond spectra (qk_local.hip makes the environments, qk_build.hip owns the factorisation primitive): the (state, bond) tasks of a
// state batch, taken in turn by `grid` workgroups with one workspace each
struct QkSpectraArgs {
  const double* env;      // the batch's environments (qk_local.hip: LocArgs.scratch) and its tables
  const int32_t* dims;    // padded bonds [n_states][n_sites + 1]
  const int32_t* tru;     // true bonds
  const int32_t* states;  // batch entry -> state of the set
  const int32_t* pmax;    // batch entry -> P
  const int64_t* sbase;   // batch entry -> first double of its environments
  const int64_t* roff;    // [batch][n_sites + 1]: R_k at sbase + rmul P^2 + roff[k] (the layout is described in qk_local_plan.h)
  const int64_t* loff;    // likewise L_k
  const int2* tasks;      // (batch entry, bond k), true bond >= 2
  int n_tasks;
  char* work;             // workgroup w: work + w * work_bytes
  long long work_bytes;
  int qmax;               // largest true bond of the tasks
  double* out;            // [n_states][n_sites - 1][max_values], zero-filled
  int n_sites, max_values, rmul;
  int* error;             // 32 ints of the caller, zeroed by the launcher: [0] error bits, then the Jacobi statistics
};
size_t qk_bond_spectra_work_bytes(int qmax);
// launches, waits and turns a factorisation that did not converge into QK_EDEVICE
int qk_bond_spectra_launch(qk_ctx* c, QkSpectraArgs a, int grid, const char* what);

// the compress sweep (qk_build.hip: qk_compress_kernel, qk_mps_set_compress): the states of a batch, taken in turn by `grid`
// workgroups with one workspace each; a state's sites live in its slots of the staging buffer from the first read to the pack
struct QkCompressArgs {
  const double* planes;   // the source set's padded split planes and its tables
  const int32_t* pad;     // padded bonds [n_states][n_sites + 1]
  const int32_t* tru;     // true bonds
  const int64_t* offs;    // re-plane offsets (doubles) [n_states][n_sites]
  int s0, n_batch, n_sites;
  double* stage;              // interleaved complex: site (s0 + i, k) at stage + 2 * stage_offs[i * n_sites + k], sized by the input bonds
  const long long* stage_offs;
  int32_t* dims_new;      // [n_states][n_sites + 1]: after pass 1 the ranks, after pass 2 the new bonds
  double* fidelity;       // [n_states]
  double* discarded;      // [n_states][n_sites - 1]
  int cap;                // 0: no cap
  double budget, zero;
  char* work;             // workgroup w: work + w * work_bytes
  long long work_bytes;
  int qmax;               // largest true bond of the batch
  int* error;             // 32 ints, zeroed by the launcher: [0] error bits, the Jacobi statistics, [25] 1 + a state of norm 0
};
size_t qk_compress_work_bytes(int qmax);
// launches, waits and turns a factorisation that did not converge or a state of norm 0 into QK_EDEVICE
int qk_compress_launch(qk_ctx* c, QkCompressArgs a, int grid, const char* what);

struct SweepArgs;
// qk_lab.hip: raise the LDS limit of the lab kernels; launch lab variant `variant` (returns QK_EINVAL if it is not one)
int qk_lab_init(qk_ctx* c);
int qk_lab_launch(qk_ctx* c, int variant, const SweepArgs& a, int grid, int n_sites);
int qk_lab_launch_quad(qk_ctx* c, const SweepArgs& a, int grid, int n_sites, bool f32);  // QK_PLAN_QUADS plans
