// qk_build.hip -- device MPS builder: the input producer of the Gram path on the GPU.
// Replaces simulate(libhandle, circ, SimulationAlgorithm.MPSxGate, config) of the reference
// (gpu_backend/kernel_state_ansatz.py:141-144, 221, 263; truncation criterion as KernelPkg.jl:68) for the ansatz gate
// program (H, Rz, Rx, Ry; XXPhase, YYPhase, ZZPhase, SWAP on adjacent qubits; 2x2 and 4x4 unitaries from a matrix table:
// qml-cutensornet_amd/ansatz.py).  Same algorithm as the host
// builder (csrc/qk_builder.cpp, mps.py:_simulate) -- orthogonality centre carried along, one SVD per two-qubit gate,
// fewest singular values whose weight keeps the fidelity -- restated for the device:
//   * all data points share ONE gate structure and differ only in the angles, so the whole list is one persistent
//     launch: a workgroup pulls a state index from a device counter and runs that state's complete gate program;
//   * the only dense factorisation is a one-sided (Hestenes) Jacobi sweep over column pairs, GL = 8 lanes per pair and
//     BT / GL = 32 pairs per step in round-robin order (256-thread workgroups): it serves as the SVD of a gate's theta
//     matrix and, with the same code, as the rank-revealing orthogonalisation of a centre move (M = (W/s)(s V^H)
//     instead of QR).  When A and V fit they are factorised in LDS (odd leading dimension: conflict-free for the 16-byte
//     elements), otherwise from the L2-resident workspace;
//   * site tensors live in a per-workgroup arena (fixed slots of 2*cap^2 complex), theta / V / temporaries in a
//     per-workgroup workspace -- L2-resident at the bonds of the reference's workloads; finished states are packed
//     into one heap (atomic bump) and described by dims / offsets / fidelity arrays.
// Where it stands: wins over the 16-core host pool at bonds <= 33 with hundreds of states, loses
// beyond bond ~64 (a block Jacobi on the matrix cores is the missing piece); build_kernel_matrix uses it only where no
// state can outgrow its bond cap (QK_BUILDER=auto).
#include "qk_host.h"
#include "qk_local_plan.h"
#include "qk_program.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>

namespace {
typedef double cd __attribute__((ext_vector_type(2)));  // complex128 as (re, im); a native vector so that LDS-typed pointers work

constexpr int MAX_SWEEPS = 40;


// CHAN = false: the question as a kernel instantiation without the channel steps asks it (code 11 cannot occur there: the host
// refuses it before the launch), so that its code is that of the kernel before the channels
template <bool CHAN = true>
__host__ __device__ inline bool is_two_qubit(int o) { return o == OP_XX || o == OP_SWAP || o == OP_YY || o == OP_ZZ || o == OP_M2 || (CHAN && o == OP_K2); }

enum { ERR_BOND = 1, ERR_HEAP = 2, ERR_SWEEPS = 4, ERR_GATE = 8, ERR_OP = 16, ERR_NORM0 = 32, ERR_CHANNEL = 64 };

// What the channel steps (op codes 10 and 11) read and write: one instance in device memory behind BuildArgs::chan, so that a program
// without channels pays one pointer.
struct ChanArgs {
  const cd* kraus;          // [n_channels][4][2][2] the channel table
  const int32_t* n_kraus;   // [n_channels] matrices of each channel (validated by the host: 1..4)
  const cd* kraus2;         // [n_channels2][16][4][4] the two-qubit channel table (null: none, code 11 is unknown)
  const int32_t* n_kraus2;  // [n_channels2] matrices of each two-qubit channel (validated by the host: 1..16)
  const int32_t* channel;   // [n_ops] channel of a channel gate (validated: inside kraus where op is 10, inside kraus2 where op is 11)
  const int32_t* branch;    // [branch_stride ? n_states : 1][n_ops] -1: the branch is drawn, k: branch k is forced
  const int32_t* kgate;     // [n_ops] how many channel gates precede gate i: the column of its branch in branch_out
  int branch_stride;        // 0 (one row for all states) or n_ops
  int n_kgates;             // channel gates of the program, codes 10 and 11 together
  unsigned seed_lo, seed_hi, first_gate;  // the Philox key; the position of gate 0 in the uninterrupted program
  const uint32_t* state_index;  // [n_states] the names of the trajectories: Philox counter (first_gate + i, trajectory, state_index, 2)
  const uint32_t* trajectory;   // [n_states]
  const int32_t* cond_col;  // [n_ops] classical control: the column kgate[cond_gate[i]] of branch_out that decides whether gate i runs, -1: unconditional (null: no conditions)
  const uint32_t* cond_mask; // [n_ops] bit v: branch v lets gate i run (read where cond_col[i] >= 0)
  int8_t* branch_out;       // [n_states][n_kgates] the branch taken (-1 where the state's program stopped early, -2 where the gate was skipped)
  double* logw_out;         // [n_ckpt][n_states] sum of log(p_b / N) so far
  const double* init_logw;  // [n_states] of the initial snapshot (read when init_heap is set)
};

struct BuildArgs {
  int n_states, n_qubits, n_ops, cap;
  const int8_t* op;
  const int32_t* q0;
  const double* alpha;  // [n_states][n_ops] half-turns
  const cd* mats;       // [mats_stride ? n_states : 1][n_mats][4][4] the matrix table of op codes 8 and 9 (null: no table, the codes are unknown)
  const int32_t* mat;   // [n_ops] table entry of a matrix gate (validated by the host: 0 .. n_mats-1 where op is 8 or 9)
  int mats_stride;      // matrices from one state's table to the next: 0 (one table for all states) or n_mats
  double budget, zero;
  cd* arena;  // per workgroup: n_qubits slots of 2 cap^2
  cd* work;   // per workgroup: 4 buffers of (2 cap + 32)^2
  int block;  // the preconditioned block Jacobi for factorisations beyond the LDS working set (QK_BUILD_BLOCK=0: scalar kernel)
  cd* heap;
  unsigned long long heap_cap;
  unsigned long long* heap_top;
  int n_ckpt;              // snapshots per state: after ckpt[j] gates (strictly increasing, the last one n_ops)
  const int32_t* ckpt;     // [n_ckpt]
  int32_t* dims_out;       // [n_ckpt][n_states][n_qubits + 1]
  double* fid_out;         // [n_ckpt][n_states] the fidelity product so far
  double* secs_out;        // [n_states] seconds of workgroup time the state took (device clock)
  long long* offs_out;     // [n_ckpt][n_states] complex elements into heap
  int32_t* centre_out;     // [n_ckpt][n_states] the site of the orthogonality centre
  const cd* init_heap;     // a resumed build: the heap of the source (null: every state starts as |0...0>), and of its snapshot ...
  const long long* init_offs;   // [n_states] ... the offsets,
  const int32_t* init_dims;     // [n_states][n_qubits + 1] the bond tables (<= cap),
  const double* init_fid;       // [n_states] the fidelities
  const int32_t* init_centre;   // [n_states] and the centres
  unsigned long long* counter;
  int* error;     // [0] error bits, [1..4] Jacobi statistics: factorisations, sweeps, most sweeps, unconverged
  int jl_offset;  // doubles from the start of the dynamic LDS to the Jacobi working set
  int jl_elems;   // complex elements it holds
  int partial;    // a state that outgrows cap is dropped (fidelity -1) instead of failing the call
  int truncate;   // bonds are cut at cap (the chi of pytket-cutensornet's Config) instead
  const int32_t* order;  // queue position -> state index: states expected to be expensive first
  const ChanArgs* chan;  // the channel table of op code 10 and the trajectories' names (null: the program holds no channel gate, the code is unknown)
};


// Shared scalars of a workgroup (one instance in LDS).
struct WgShared {
  int flag, keep, state, pad;
  double frac, nrm;
  unsigned long long off;
  unsigned long long worst;  // bits of the largest squared relative inner product rotated in the current sweep
  double logw;               // the log-weight of the trajectory so far (channels, op code 10)
  double pad16;              // the struct stays a multiple of 16 bytes: the dynamic LDS behind it holds complex numbers read 16 bytes at a time, and
                             // 8 bytes more of static LDS cost the builder 5 % (bonds <= 32) to 47 % (cfg4) until this field restored the alignment
};
static_assert(sizeof(WgShared) % 16 == 0, "WgShared must keep the dynamic LDS 16-byte aligned");


// Built states -> the Gram engine's set image: site (s, k) of the heap ([l][2][r] complex, interleaved) becomes two planes
// [pad16(l)][2][pad16(r)] (re, im) in a zero-initialised allocation (the layout of qk_pack_state, qkgram.hip).
__global__ __launch_bounds__(256) void qk_pack_built_kernel(const cd* __restrict__ heap, const long long* __restrict__ src_offs,
                                                            const long long* __restrict__ dst_offs, const int32_t* __restrict__ dims_true,
                                                            const int32_t* __restrict__ dims_pad, int n_sites, double* __restrict__ data) {
  const int s = blockIdx.x / n_sites, k = blockIdx.x - s * n_sites;
  const int cl = dims_true[(long)s * (n_sites + 1) + k], cr = dims_true[(long)s * (n_sites + 1) + k + 1];
  const int pl = dims_pad[(long)s * (n_sites + 1) + k], pr = dims_pad[(long)s * (n_sites + 1) + k + 1];
  const cd* src = heap + src_offs[blockIdx.x];
  double* re = data + dst_offs[blockIdx.x];
  double* im = re + (long)pl * 2 * pr;
  for (int e = threadIdx.x; e < cl * 2 * cr; e += 256) {
    const int row = e / cr, c = e - row * cr;
    const cd v = src[e];
    re[(long)row * pr + c] = v.x;
    im[(long)row * pr + c] = v.y;
  }
}

// The inverse (qk_built_from_set, verbatim path): site (s, k) of a set's image, two planes [pad16(l)][2][pad16(r)], becomes the
// interleaved packed [l][2][r] of a builder's heap.  One workgroup per (state, site); true bonds only, nothing is rescaled: the bits
// of the heap are the bits of the set.
__global__ __launch_bounds__(256) void qk_unpack_set_kernel(const double* __restrict__ data, const long long* __restrict__ src_offs,
                                                            const long long* __restrict__ dst_offs, const int32_t* __restrict__ dims_true,
                                                            const int32_t* __restrict__ dims_pad, int n_sites, cd* __restrict__ heap) {
  const int s = blockIdx.x / n_sites, k = blockIdx.x - s * n_sites;
  const int cl = dims_true[(long)s * (n_sites + 1) + k], cr = dims_true[(long)s * (n_sites + 1) + k + 1];
  const int pl = dims_pad[(long)s * (n_sites + 1) + k], pr = dims_pad[(long)s * (n_sites + 1) + k + 1];
  const double* re = data + src_offs[blockIdx.x];
  const double* im = re + (long)pl * 2 * pr;
  cd* dst = heap + dst_offs[blockIdx.x];
  for (int e = threadIdx.x; e < cl * 2 * cr; e += 256) {
    const int row = e / cr, c = e - row * cr;
    dst[e] = cd{re[(long)row * pr + c], im[(long)row * pr + c]};
  }
}

// The finite check of the sweep path: one workgroup per (state, site) reads the true-bond corner of the site's planes and raises the
// state's flag (zeroed by the host) when an element is not finite.  Every writer of a flag writes the same 1.
__global__ __launch_bounds__(256) void qk_seed_finite_kernel(const double* __restrict__ data, const long long* __restrict__ src_offs,
                                                             const int32_t* __restrict__ dims_true, const int32_t* __restrict__ dims_pad, int n_sites,
                                                             int32_t* __restrict__ flags) {
  const int s = blockIdx.x / n_sites, k = blockIdx.x - s * n_sites;
  const int cl = dims_true[(long)s * (n_sites + 1) + k], cr = dims_true[(long)s * (n_sites + 1) + k + 1];
  const int pl = dims_pad[(long)s * (n_sites + 1) + k], pr = dims_pad[(long)s * (n_sites + 1) + k + 1];
  const double* re = data + src_offs[blockIdx.x];
  const double* im = re + (long)pl * 2 * pr;
  int bad = 0;
  for (int e = threadIdx.x; e < cl * 2 * cr; e += 256) {
    const int row = e / cr, c = e - row * cr;
    bad |= !(isfinite(re[(long)row * pr + c]) && isfinite(im[(long)row * pr + c]));
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) flags[s] = 1;
}

}  // namespace

#define QKB_NS qkb256
#define QK_BUILD_BT 256
#include "qk_build_kernels.h"
#undef QKB_NS
#undef QK_BUILD_BT
#define QKB_NS qkb512
#define QK_BUILD_BT 512
#include "qk_build_kernels.h"
#undef QKB_NS
#undef QK_BUILD_BT

// The gather of the sweep path: one workgroup per state of a compress batch.  The state's sites lie compact at the start of their
// staging slots (sized by the INPUT bonds: gaps where a bond shrank); they become one contiguous heap record with the new bond table.
//
// Then the sites are polished, left to right.  From 48 columns on the sweep's factorisation forms an isometry as (A V) / sigma, which
// leaves a column sigma_max / sigma roundings from orthogonal to the others (1e-9 measured at bond 70).  With E = U^H U - 1 of site k
// (U as [2 l][r]) one Newton-Schulz step of the polar factor, U <- U (1 - E/2), squares the defect, and site k+1 <- (1 + E/2) site k+1
// keeps the state: (1 - E/2)(1 + E/2) = 1 - E^2/4.  A site is polished when max|E| lies above SEED_POLISH_TOL (below it E is the
// rounding of its own product) and not above SEED_POLISH_MAX (beyond it E^2 would show in the state: such a site stays as the sweep
// left it); a defect above SEED_POLISH_SURE is looked at again, at most three times.  The three products (U^H U, U E, E site k+1)
// are the builder's wg_gemm_mfma through `scratch` (E: the largest bond squared, then a product or conj(U): the largest site): one
// wavefront per tile in a fixed order, so the bits do not depend on the launch.
//
// The centre is the last site: its Frobenius norm is summed per thread over its strided elements in ascending order as one chain of
// fused multiply-adds, the partial sums go through LDS and are added in ascending thread order (no atomics), the site is divided by
// the norm and the norm written to norms[state].  A norm that is 0 or not finite is left for the host to name: the site then stays
// as it is.
constexpr double SEED_POLISH_TOL = 1e-13, SEED_POLISH_SURE = 1e-8, SEED_POLISH_MAX = 1e-6;

__global__ __launch_bounds__(256) void qk_seed_gather_kernel(const cd* __restrict__ stage, const long long* __restrict__ stage_offs,
                                                             const int32_t* __restrict__ dims_new, const long long* __restrict__ heap_offs, int s0,
                                                             int n_sites, cd* __restrict__ heap, double* __restrict__ norms, cd* __restrict__ scratch,
                                                             const long long* __restrict__ scratch_offs) {
  using namespace qkb256;
  __shared__ double part[256];
  const int tid = threadIdx.x, n = n_sites;
  const long long st = (long long)s0 + blockIdx.x;
  const int32_t* const dn = dims_new + st * (n + 1);
  const long long* const so = stage_offs + (long long)blockIdx.x * n;
  cd* const rec = heap + heap_offs[st];
  cd* site = rec;
  long rmax2 = 1;
  for (int k = 0; k < n; ++k) {
    const cd* const src = stage + so[k];
    const long cnt = 2L * dn[k] * dn[k + 1];
    for (long e = tid; e < cnt; e += 256) site[e] = src[e];
    site += cnt;
    rmax2 = max(rmax2, (long)dn[k + 1] * dn[k + 1]);
  }
  __syncthreads();
  cd* const E = scratch + scratch_offs[blockIdx.x];
  cd* const D = E + rmax2;
  site = rec;
  for (int k = 0; k + 1 < n; ++k) {
    const int m = 2 * dn[k], r = dn[k + 1], c2 = 2 * dn[k + 2];
    cd* const U = site;             // [m][r]
    cd* const N = site + (long)m * r;  // [r][c2]
    for (int it = 0; it < 3; ++it) {
      for (long e = tid; e < (long)m * r; e += 256) D[e] = cd{U[e].x, -U[e].y};
      __syncthreads();
      wg_gemm_mfma(E, r, r, m, D, 1, r, U, r, 1);  // U^H U
      double big = 0.0;
      for (long e = tid; e < (long)r * r; e += 256) {
        cd g = E[e];
        if (e / r == e % r) g.x -= 1.0, E[e] = g;
        big = fmax(big, fmax(fabs(g.x), fabs(g.y)));
      }
      part[tid] = big;
      __syncthreads();
      if (tid == 0) {
        double top = 0.0;
        for (int t = 0; t < 256; ++t) top = fmax(top, part[t]);
        part[0] = top;
      }
      __syncthreads();
      big = part[0];
      __syncthreads();
      if (!(big > SEED_POLISH_TOL) || !(big <= SEED_POLISH_MAX)) break;  // the same for every thread
      wg_gemm_mfma(D, m, r, r, U, r, 1, E, r, 1);
      for (long e = tid; e < (long)m * r; e += 256) {
        const cd u = U[e], d = D[e];
        U[e] = cd{u.x - 0.5 * d.x, u.y - 0.5 * d.y};
      }
      __syncthreads();
      wg_gemm_mfma(D, r, c2, r, E, r, 1, N, c2, 1);
      for (long e = tid; e < (long)r * c2; e += 256) {
        const cd v = N[e], d = D[e];
        N[e] = cd{v.x + 0.5 * d.x, v.y + 0.5 * d.y};
      }
      __syncthreads();
      if (big <= SEED_POLISH_SURE) break;  // its square is rounding: no second look
    }
    site += (long)m * r;
  }
  cd* const last = site;
  const long cnt = 2L * dn[n - 1] * dn[n];
  double acc = 0.0;
  for (long e = tid; e < cnt; e += 256) {
    const cd v = last[e];
    acc = fma(v.x, v.x, acc);
    acc = fma(v.y, v.y, acc);
  }
  part[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int t = 0; t < 256; ++t) tot += part[t];
    part[0] = sqrt(tot);
  }
  __syncthreads();
  const double nrm = part[0];
  if (nrm > 0.0 && isfinite(nrm))
    for (long e = tid; e < cnt; e += 256) {
      const cd v = last[e];
      last[e] = cd{v.x / nrm, v.y / nrm};
    }
  if (tid == 0) norms[st] = nrm;
}


// ---- entanglement spectra of a bond (qk_bond_spectra_host, qk_local.hip) ------------------------------------------------------
// One (state, bond k) per workgroup at a time, true bond q >= 2.  With the kept environments L_k, R_k (X[ket][bra] orientation,
// split re/im planes of the padded bond) and nrm = L_n[0][0]:
//   1. the true-bond corners become interleaved: A = L_k^T (Hermitian, positive semi-definite), Rm = R_k;
//   2. A V = W by the builder's Jacobi primitive (jacobi_auto: in LDS below 48 columns, preconditioned block Jacobi on the matrix
//      cores from 48 on): L_k^T = V S V^H with S = diag(sig);
//   3. F = S^{1/2} V^H and H_k = F R_k F^H / nrm by two workgroup GEMMs on the matrix cores: Hermitian, the eigenvalues of
//      N_k = R_k L_k^T / nrm;
//   4. the same primitive on H_k: its singular values are the eigenvalues (>= 0 by construction), written in descending order.
// The block path drops what lies below `cut` ||A||_F^2: the builder's 1e-22 would cost 1e-11 of a weight (oracle/jacobi_model.py:
// 1.5e-12 on a graded 48 x 48 matrix); 1e-30 leaves rounding alone (3e-16 on the same matrix, one or two sweeps more).
// The sweeps run until nothing is rotated (early = 0): step 3 needs L_k^T = V S V^H, and the builder's early exit leaves nearly
// degenerate columns (L_k = 1 + 1e-11 of a device-built state) 1e-11 from orthogonal -- measured as 2e-11 on a weight of cfg4.
constexpr double SPEC_CUT = 1e-30;
constexpr size_t SPEC_LDS = 76 * 1024;
// The LDS head (sig and ord) is reserved for the largest bond the entry point takes, whatever the batch holds: what is left for the
// Jacobi working set decides the path of a factorisation (LDS below 48 columns: 94 x 47 = 4418 elements) and the width of a
// Gram-Schmidt panel, and a state's bits must not depend on the other bonds of its batch.
constexpr int SPEC_QMAX = 512;
inline int spec_pad(int x, int m) { return (x + m - 1) / m * m; }
constexpr int SPEC_HEAD_DOUBLES = ((SPEC_QMAX * 12 + 15) / 16) * 2 + 2;  // sig and ord, 16-byte aligned
constexpr int SPEC_LDS_ELEMS = (int)((SPEC_LDS - SPEC_HEAD_DOUBLES * sizeof(double)) / (2 * sizeof(double)));
static_assert(SPEC_LDS_ELEMS >= 94 * 47, "a 47-column factorisation must fit the LDS working set");
inline long spec_lbuf_elems(int q) { return (long)spec_pad(q, 32) * spec_pad(q, 16); }

__global__ __launch_bounds__(256, 2) void qk_bond_spectra_kernel(const QkSpectraArgs g, const long lbuf_elems) {
  using namespace qkb256;
  extern __shared__ double sh_raw[];
  __shared__ WgShared sh;
  const int tid = threadIdx.x, n = g.n_sites, n1 = n + 1;
  const long Q2 = (long)g.qmax * g.qmax;
  double* const sig = sh_raw;
  int* const ord = reinterpret_cast<int*>(sig + SPEC_QMAX);
  cd* const lds = reinterpret_cast<cd*>(sh_raw + SPEC_HEAD_DOUBLES);
  constexpr int lds_elems = SPEC_LDS_ELEMS;
  cd* const A = reinterpret_cast<cd*>(g.work + (long long)blockIdx.x * g.work_bytes);
  cd* const V = A + Q2;
  cd* const Rm = V + Q2;
  cd* const S = Rm + Q2;
  cd* const LB = S + Q2;  // the block layout of the preconditioned path, the table of clean block pairs behind it
  for (int t = blockIdx.x; t < g.n_tasks; t += gridDim.x) {
    const int i = g.tasks[t].x, k = g.tasks[t].y;
    const long long st = g.states[i];
    const int q = g.tru[st * n1 + k], pk = g.dims[st * n1 + k];
    const long long P = g.pmax[i], P2 = P * P;
    const double* const E = g.env + g.sbase[i];
    const double nrm = E[0];  // L_n[0][0]
    const double* const Lre = E + g.rmul * P2 + g.loff[(long long)i * n1 + k];
    const double* const Rre = E + g.rmul * P2 + g.roff[(long long)i * n1 + k];
    const long long pl = (long long)pk * pk;
    for (int e = tid; e < q * q; e += 256) {
      const int a = e / q, b = e - a * q;
      A[e] = cd{Lre[(long long)b * pk + a], Lre[pl + (long long)b * pk + a]};
      Rm[e] = cd{Rre[(long long)a * pk + b], Rre[pl + (long long)a * pk + b]};
    }
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
      jacobi_auto<2>(A, q, 1, q, q, V, sig, ord, &sh, g.error, lds, lds_elems, S, LB, lbuf_elems, SPEC_CUT, 0.0);
      __syncthreads();
      if (pass == 0) {
        wg_gemm_mfma(S, q, q, q, Rm, q, 1, V, q, 1);  // R V
        for (int e = tid; e < q * q; e += 256) {
          const int j = e / q, a = e - j * q;
          const cd v = V[(long)a * q + j];
          const double f = sqrt(sig[j]);
          Rm[e] = cd{f * v.x, -f * v.y};  // F[j][a] = sqrt(s_j) conj(V[a][j])
        }
        for (int e = tid; e < q * q; e += 256) {
          const double f = sqrt(sig[e % q]) / nrm;
          S[e] = cd{S[e].x * f, S[e].y * f};  // R V S^{1/2} / nrm
        }
        __syncthreads();
        wg_gemm_mfma(A, q, q, q, Rm, q, 1, S, q, 1);  // H_k
      }
    }
    double* const o = g.out + (st * (n - 1) + (k - 1)) * g.max_values;
    for (int e = tid; e < min(q, g.max_values); e += 256) o[e] = sig[ord[e]];
    __syncthreads();
  }
}

size_t qk_bond_spectra_work_bytes(const int qmax) {
  const size_t q2 = (size_t)qmax * qmax, nbk = (size_t)spec_pad(qmax, 16) / 8;
  return ((4 * q2 + (size_t)spec_lbuf_elems(qmax)) * sizeof(cd) + nbk * nbk * sizeof(int) + 255) / 256 * 256;
}

int qk_bond_spectra_launch(qk_ctx* c, QkSpectraArgs a, const int grid, const char* what) {
  static_assert(SPEC_LDS_ELEMS >= qkb256::NWV * qkb256::BLK_LDS, "the block Jacobi's LDS matrices must fit");
  if (a.qmax > SPEC_QMAX) return qk_fail(QK_EINVAL, "%s: a bond of %d is beyond the %d the factorisation's LDS bookkeeping holds", what, a.qmax, SPEC_QMAX);
  HIP_TRY_AS(what, hipMemsetAsync(a.error, 0, 32 * sizeof(int), c->stream));
  HIP_TRY_AS(what, hipFuncSetAttribute(reinterpret_cast<const void*>(qk_bond_spectra_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPEC_LDS));
  qk_bond_spectra_kernel<<<dim3((unsigned)grid), dim3(256), SPEC_LDS, c->stream>>>(a, spec_lbuf_elems(a.qmax));
  HIP_TRY_AS(what, hipGetLastError());
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  int errv[32] = {0};
  HIP_TRY_AS(what, hipMemcpy(errv, a.error, sizeof errv, hipMemcpyDeviceToHost));
  if (errv[0]) return qk_fail(QK_EDEVICE, "%s: a Jacobi factorisation did not converge in %d sweeps", what, MAX_SWEEPS);
  return QK_OK;
}

// ---- compressing a set (qk_mps_set_compress below) ------------------------------------------------------------------------------
// One state per workgroup at a time, in the mould of the spectra kernel: the true-bond corners of the state's padded split planes
// become interleaved sites in the state's slots of the staging buffer (sized by the INPUT bonds: no bond grows, so every
// intermediate fits its slot and the offsets are known before the launch), and two passes work on them in place:
//   pass 1, k = n-1 .. 1: site k ([l][2 r], r already reduced) = carry (l x m) x Q (m x 2 r, orthonormal rows); site k-1 <- site k-1 x carry;
//   pass 2, k = 0 .. n-2: the centre ([2 l'][r]) = U S V^H, wg_kept chooses m; site k <- U_m, site k+1 <- (S_m V_m^H) f x site k+1
//           with f = sqrt(total / kept).
// Every factorisation is jacobi_auto on the SMALLER side of the matrix (columns <= rows, as the builder takes a gate's theta), with
// the spectra's settings: cut 1e-30 and sweeps that run until nothing rotates -- the sites of the result are isometries to rounding
// and its weights agree with the host mirror's LAPACK values to 1e-12.  The LDS head and working set are the spectra's constants
// (SPEC_QMAX): a state's path and bits do not depend on its batch.  The norm sits in the last site.
__global__ __launch_bounds__(256, 2) void qk_compress_kernel(const QkCompressArgs g, const long lbuf_elems) {
  using namespace qkb256;
  extern __shared__ double sh_raw[];
  __shared__ WgShared sh;
  const int tid = threadIdx.x, n = g.n_sites, n1 = n + 1;
  const long Q2 = (long)g.qmax * g.qmax;
  double* const sig = sh_raw;
  int* const ord = reinterpret_cast<int*>(sig + SPEC_QMAX);
  cd* const lds = reinterpret_cast<cd*>(sh_raw + SPEC_HEAD_DOUBLES);
  constexpr int lds_elems = SPEC_LDS_ELEMS;
  cd* const VV = reinterpret_cast<cd*>(g.work + (long long)blockIdx.x * g.work_bytes);  // V of a factorisation
  cd* const CM = VV + Q2;        // the matrix that goes into the neighbour: the carry, or S V^H
  cd* const TMP = CM + Q2;       // the factorisation's scratch, then the site's new tensor
  cd* const TH = TMP + 2 * Q2;   // the neighbour's new tensor
  cd* const LB = TH + 2 * Q2;    // the block layout of the preconditioned path, the table of clean block pairs behind it
  cd* const stage = reinterpret_cast<cd*>(g.stage);
  for (int i = blockIdx.x; i < g.n_batch; i += gridDim.x) {
    const long long st = (long long)g.s0 + i;
    const int32_t* const tru = g.tru + st * n1;
    const int32_t* const pad = g.pad + st * n1;
    const long long* const so = g.stage_offs + (long long)i * n;
    int32_t* const dn = g.dims_new + st * n1;
    for (int k = 0; k < n; ++k) {
      const int l = tru[k], r = tru[k + 1], pr = pad[k + 1];
      const double* const re = g.planes + g.offs[st * n + k];
      const double* const im = re + (long long)pad[k] * 2 * pr;
      cd* const dst = stage + so[k];
      for (int e = tid; e < l * 2 * r; e += 256) {
        const int row = e / r, c = e - row * r;
        dst[e] = cd{re[(long long)row * pr + c], im[(long long)row * pr + c]};
      }
    }
    for (int k = tid; k <= n; k += 256) dn[k] = tru[k];
    __syncthreads();
    bool bad = false;  // a state of norm 0: uniform over the workgroup
    // ---- pass 1: right to left, the ranks
    int r = 1;
    for (int k = n - 1; k >= 1; --k) {
      cd* const t = stage + so[k];
      cd* const d = stage + so[k - 1];
      const int l = tru[k], l0 = tru[k - 1], w = 2 * r;
      const bool cols = l <= w;  // t^T (w x l) has the fewer columns; otherwise t (l x w) is factorised as it lies
      const int q = cols ? l : w;
      if (cols) jacobi_auto<2>(t, 1, w, w, l, VV, sig, ord, &sh, g.error, lds, lds_elems, TMP, LB, lbuf_elems, SPEC_CUT, 0.0);
      else jacobi_auto<2>(t, w, 1, l, w, VV, sig, ord, &sh, g.error, lds, lds_elems, TMP, LB, lbuf_elems, SPEC_CUT, 0.0);
      __syncthreads();
      if (tid == 0) {
        double tot = 0;
        for (int j = 0; j < q; ++j) tot += sig[j] * sig[j];
        sh.nrm = tot;
      }
      __syncthreads();
      const double tot = sh.nrm;
      __syncthreads();
      if (!(tot > 0.0)) {
        bad = true;
        break;
      }
      wg_kept(sig, ord, q, 0.0, g.zero * sqrt(tot), &sh);
      const int m = sh.keep;
      // cols: t^T = W V^H, so t = [s conj(V)] [W / s]^T;  rows: t = W V^H
      for (int e = tid; e < m * w; e += 256) {  // the new site Q[jj][(p, c)]
        const int jj = e / w, ii = e - jj * w, c = ord[jj];
        if (cols) {
          const double inv = 1.0 / sig[c];
          const cd x = t[(long)c * w + ii];
          TMP[e] = cd{x.x * inv, x.y * inv};
        } else {
          const cd v = VV[(long)ii * w + c];
          TMP[e] = cd{v.x, -v.y};
        }
      }
      for (int e = tid; e < l * m; e += 256) {  // the carry [a][jj]
        const int a = e / m, jj = e - a * m, c = ord[jj];
        if (cols) {
          const double s = sig[c];
          const cd v = VV[(long)a * l + c];
          CM[e] = cd{s * v.x, -s * v.y};
        } else {
          CM[e] = t[(long)a * w + c];
        }
      }
      __syncthreads();
      wg_gemm_mfma(TH, 2 * l0, m, l, d, l, 1, CM, m, 1);  // carry x site: site k-1 ([2 l0][l]) x carry
      wg_copy(t, TMP, (long)m * w);
      wg_copy(d, TH, (long)2 * l0 * m);
      if (tid == 0) dn[k] = m;
      r = m;
      __syncthreads();
    }
    // ---- pass 2: left to right, the cut
    double fid = 1.0;
    int lp = 1;
    for (int k = 0; k < n - 1 && !bad; ++k) {
      cd* const t = stage + so[k];
      cd* const u = stage + so[k + 1];
      const int rr = dn[k + 1], r2 = dn[k + 2], m2 = 2 * lp;
      const bool cols = rr <= m2;  // the centre t ([m2][rr]) as it lies; otherwise its transpose
      const int q = cols ? rr : m2;
      if (cols) jacobi_auto<2>(t, rr, 1, m2, rr, VV, sig, ord, &sh, g.error, lds, lds_elems, TMP, LB, lbuf_elems, SPEC_CUT, 0.0);
      else jacobi_auto<2>(t, 1, rr, rr, m2, VV, sig, ord, &sh, g.error, lds, lds_elems, TMP, LB, lbuf_elems, SPEC_CUT, 0.0);
      __syncthreads();
      if (tid == 0) {
        double tot = 0;
        for (int j = 0; j < q; ++j) tot += sig[j] * sig[j];
        sh.nrm = tot;
      }
      __syncthreads();
      const double tot = sh.nrm;
      __syncthreads();
      if (!(tot > 0.0)) {
        bad = true;
        break;
      }
      wg_kept(sig, ord, q, g.budget, g.zero * sqrt(tot), &sh, g.cap);
      const int keep = sh.keep;
      if (tid == 0) {  // what the cut drops, summed from the small end
        double tail = 0;
        for (int j = q - 1; j >= keep; --j) tail += sig[ord[j]] * sig[ord[j]];
        sh.frac = tail / tot;
      }
      __syncthreads();
      const double disc = sh.frac;
      const double f = 1.0 / sqrt(1.0 - disc);
      // cols: t = W V^H = [W / s] [s V^H];  rows: t^T = W V^H, so t = conj(V) W^T
      for (int e = tid; e < m2 * keep; e += 256) {  // U[(a, p)][jj]
        const int row = e / keep, jj = e - row * keep, c = ord[jj];
        if (cols) {
          const double inv = 1.0 / sig[c];
          const cd x = t[(long)row * rr + c];
          TMP[e] = cd{x.x * inv, x.y * inv};
        } else {
          const cd v = VV[(long)row * m2 + c];
          TMP[e] = cd{v.x, -v.y};
        }
      }
      for (int e = tid; e < keep * rr; e += 256) {  // (S V^H) f [jj][c]
        const int jj = e / rr, col = e - jj * rr, c = ord[jj];
        if (cols) {
          const double s = sig[c] * f;
          const cd v = VV[(long)col * rr + c];
          CM[e] = cd{s * v.x, -s * v.y};
        } else {
          const cd x = t[(long)c * rr + col];
          CM[e] = cd{x.x * f, x.y * f};
        }
      }
      __syncthreads();
      wg_gemm_mfma(TH, keep, 2 * r2, rr, CM, rr, 1, u, 2 * r2, 1);  // S V^H x next site ([rr][2 r2])
      wg_copy(t, TMP, (long)m2 * keep);
      wg_copy(u, TH, (long)keep * 2 * r2);
      if (tid == 0) {
        dn[k + 1] = keep;
        g.discarded[st * (n - 1) + k] = disc;
      }
      fid *= 1.0 - disc;
      lp = keep;
      __syncthreads();
    }
    if (tid == 0) {
      g.fidelity[st] = bad ? -1.0 : fid;
      if (bad) {
        atomicOr(g.error, ERR_NORM0);
        atomicMax(g.error + 25, (int)st + 1);
      }
    }
    __syncthreads();
  }
}

size_t qk_compress_work_bytes(const int qmax) {
  const size_t q2 = (size_t)qmax * qmax, nbk = (size_t)spec_pad(qmax, 16) / 8;
  return ((6 * q2 + (size_t)spec_lbuf_elems(qmax)) * sizeof(cd) + nbk * nbk * sizeof(int) + 255) / 256 * 256;
}

int qk_compress_launch(qk_ctx* c, QkCompressArgs a, const int grid, const char* what) {
  if (a.qmax > SPEC_QMAX) return qk_fail(QK_EINVAL, "%s: a bond of %d is beyond the %d the factorisation's LDS bookkeeping holds", what, a.qmax, SPEC_QMAX);
  HIP_TRY_AS(what, hipMemsetAsync(a.error, 0, 32 * sizeof(int), c->stream));
  HIP_TRY_AS(what, hipFuncSetAttribute(reinterpret_cast<const void*>(qk_compress_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPEC_LDS));
  qk_compress_kernel<<<dim3((unsigned)grid), dim3(256), SPEC_LDS, c->stream>>>(a, spec_lbuf_elems(a.qmax));
  HIP_TRY_AS(what, hipGetLastError());
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  int errv[32] = {0};
  HIP_TRY_AS(what, hipMemcpy(errv, a.error, sizeof errv, hipMemcpyDeviceToHost));
  if (errv[0] & ERR_NORM0) return qk_fail(QK_EDEVICE, "%s: state %d has norm 0 (a site or a centre of the sweep is all zeros): nothing to compress", what, errv[25] - 1);
  if (errv[0]) return qk_fail(QK_EDEVICE, "%s: a Jacobi factorisation did not converge in %d sweeps", what, MAX_SWEEPS);
  return QK_OK;
}

extern "C" int qk_mps_set_compress(qk_ctx* c, const qk_mps_set* src, int32_t max_bond, double max_discard, double value_of_zero, qk_mps_set** out, double* fidelity,
                                   double* discarded) {
  static const char* what = "qk_mps_set_compress";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!src) return qk_fail(QK_EINVAL, "%s: src is null", what);
  if (!out) return qk_fail(QK_EINVAL, "%s: out is null", what);
  *out = nullptr;
  if (src->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (src->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; compressing needs an fp64 set", what);
  if (max_bond < 0) return qk_fail(QK_EINVAL, "%s: max_bond must be >= 0 (0: no cap), got %d", what, max_bond);
  if (!(max_discard >= 0.0) || !std::isfinite(max_discard)) return qk_fail(QK_EINVAL, "%s: max_discard must be >= 0 and finite (got %g)", what, max_discard);
  if (!(value_of_zero >= 0.0) || !std::isfinite(value_of_zero)) return qk_fail(QK_EINVAL, "%s: value_of_zero must be >= 0 and finite (got %g)", what, value_of_zero);
  const int ns = src->n_states, n = src->n_sites, n1 = n + 1;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  const int32_t* tru = src->dims_true.data();
  int qall = 1;
  for (size_t e = 0; e < (size_t)ns * n1; ++e) qall = std::max(qall, (int)tru[e]);
  if (qall > SPEC_QMAX) return qk_fail(QK_EINVAL, "%s: a bond of %d is beyond the %d the factorisation's LDS bookkeeping holds", what, qall, SPEC_QMAX);
  QkRangeGuard range_("qk:compress");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  auto pad16 = [](int x) { return (x + 15) / 16 * 16; };
  // a state's slots of the staging buffer (complex elements, by its input bonds); batches by the quarter-of-free-memory rule: the
  // staging buffer takes at most half of it (at least one state), the workgroups' workspaces the rest (at least one workgroup)
  std::vector<long long> need(ns, 0);
  for (int s = 0; s < ns; ++s)
    for (int k = 0; k < n; ++k) need[s] += 2ll * tru[(size_t)s * n1 + k] * tru[(size_t)s * n1 + k + 1];
  size_t free_b = 0, total_b = 0;
  HIP_TRY_AS(what, hipMemGetInfo(&free_b, &total_b));
  const long long budget = (long long)(free_b / 4);
  std::vector<int> bstart{0};
  for (long long acc = 0, s = 0; s < ns; ++s) {
    const long long w = need[s] * (long long)sizeof(cd);
    if (acc > 0 && acc + w > budget / 2) bstart.push_back((int)s), acc = 0;
    acc += w;
  }
  bstart.push_back(ns);
  QkDevBuf d_new, d_fid, d_disc, d_err, d_so, d_dst, d_pad;
  const size_t n_disc = std::max<size_t>(1, (size_t)ns * (n - 1));
  HIP_TRY_AS(what, d_new.alloc((size_t)ns * n1 * sizeof(int32_t)));
  HIP_TRY_AS(what, d_fid.alloc((size_t)ns * sizeof(double)));
  HIP_TRY_AS(what, d_disc.alloc(n_disc * sizeof(double)));
  HIP_TRY_AS(what, d_err.alloc(32 * sizeof(int)));
  HIP_TRY_AS(what, d_so.alloc((size_t)ns * n * sizeof(long long)));
  HIP_TRY_AS(what, d_dst.alloc((size_t)ns * n * sizeof(long long)));
  HIP_TRY_AS(what, d_pad.alloc((size_t)ns * n1 * sizeof(int32_t)));
  HIP_TRY_AS(what, hipMemsetAsync(d_disc.get(), 0, n_disc * sizeof(double), c->stream));
  std::vector<long long> so((size_t)ns * n), dst((size_t)ns * n);
  std::vector<int32_t> dims_new((size_t)ns * n1), pad_new((size_t)ns * n1);
  std::vector<QkDevBuf> chunks(bstart.size() - 1);  // the packed planes of each batch, until the new set is put together
  std::vector<long long> chunk_doubles(bstart.size() - 1, 0);
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    long long stage_elems = 0;
    int qmax = 1;
    for (int s = s0; s < s0 + nb; ++s)
      for (int k = 0; k < n; ++k) {
        so[(size_t)s * n + k] = stage_elems;
        stage_elems += 2ll * tru[(size_t)s * n1 + k] * tru[(size_t)s * n1 + k + 1];
        qmax = std::max(qmax, (int)tru[(size_t)s * n1 + k]);
      }
    const size_t per_wg = qk_compress_work_bytes(qmax);
    const long long room = budget - stage_elems * (long long)sizeof(cd);
    const int grid = (int)std::max<long long>(1, std::min<long long>({(long long)nb, 2ll * c->num_cus, room / (long long)per_wg}));
    QkDevBuf stage, work;
    HIP_TRY_AS(what, stage.alloc((size_t)stage_elems * sizeof(cd)));
    HIP_TRY_AS(what, work.alloc((size_t)grid * per_wg));
    HIP_TRY_AS(what, hipMemcpyAsync(d_so.get<long long>() + (size_t)s0 * n, so.data() + (size_t)s0 * n, (size_t)nb * n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    QkCompressArgs a{};
    a.planes = src->d_data.get<double>(), a.pad = src->d_dims.get<int32_t>(), a.tru = src->d_true.get<int32_t>(), a.offs = src->d_offs.get<int64_t>();
    a.s0 = s0, a.n_batch = nb, a.n_sites = n;
    a.stage = stage.get<double>(), a.stage_offs = d_so.get<long long>() + (size_t)s0 * n;
    a.dims_new = d_new.get<int32_t>(), a.fidelity = d_fid.get<double>(), a.discarded = d_disc.get<double>();
    a.cap = max_bond, a.budget = max_discard, a.zero = value_of_zero;
    a.work = work.get<char>(), a.work_bytes = (long long)per_wg, a.qmax = qmax, a.error = d_err.get<int>();
    if (const int rc = qk_compress_launch(c, a, grid, what)) return rc;  // synchronises and reads the error word
    // the new bonds of the batch -> its padded planes
    HIP_TRY_AS(what, hipMemcpy(dims_new.data() + (size_t)s0 * n1, d_new.get<int32_t>() + (size_t)s0 * n1, (size_t)nb * n1 * sizeof(int32_t), hipMemcpyDeviceToHost));
    long long doubles = 0;
    for (int s = s0; s < s0 + nb; ++s) {
      for (int k = 0; k <= n; ++k) {
        const int32_t x = dims_new[(size_t)s * n1 + k];
        if (x < 1 || x > tru[(size_t)s * n1 + k]) return qk_fail(QK_EDEVICE, "%s: state %d came back with bond %d of %d (was %d)", what, s, k, (int)x, (int)tru[(size_t)s * n1 + k]);
        pad_new[(size_t)s * n1 + k] = pad16(x);
      }
      for (int k = 0; k < n; ++k) {
        dst[(size_t)s * n + k] = doubles;
        doubles += 2ll * pad_new[(size_t)s * n1 + k] * 2 * pad_new[(size_t)s * n1 + k + 1];
      }
    }
    chunk_doubles[bi] = doubles;
    HIP_TRY_AS(what, chunks[bi].alloc((size_t)doubles * sizeof(double)));
    HIP_TRY_AS(what, hipMemsetAsync(chunks[bi].get(), 0, (size_t)doubles * sizeof(double), c->stream));
    HIP_TRY_AS(what, hipMemcpyAsync(d_dst.get<long long>() + (size_t)s0 * n, dst.data() + (size_t)s0 * n, (size_t)nb * n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY_AS(what, hipMemcpyAsync(d_pad.get<int32_t>() + (size_t)s0 * n1, pad_new.data() + (size_t)s0 * n1, (size_t)nb * n1 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    qk_pack_built_kernel<<<dim3((unsigned)(nb * n)), dim3(256), 0, c->stream>>>(stage.get<cd>(), d_so.get<long long>() + (size_t)s0 * n, d_dst.get<long long>() + (size_t)s0 * n,
                                                                              d_new.get<int32_t>() + (size_t)s0 * n1, d_pad.get<int32_t>() + (size_t)s0 * n1, n, chunks[bi].get<double>());
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the staging buffer and the workspaces go before the next batch
  }
  long long total = 0;
  int max_pad = 0;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {  // offsets within a batch's planes -> offsets within the set
    for (size_t e = (size_t)bstart[bi] * n; e < (size_t)bstart[bi + 1] * n; ++e) dst[e] += total;
    total += chunk_doubles[bi];
  }
  for (int32_t x : pad_new) max_pad = std::max(max_pad, (int)x);
  qk_mps_set* m = nullptr;
  if (const int rc = qk_mps_set_alloc(c, ns, n, total * (long long)sizeof(double), 64, &m, what)) return rc;
  m->max_pad = max_pad;
  m->dims_true = dims_new;
  hipError_t e = hipSuccess;
  long long pos = 0;
  for (size_t bi = 0; bi + 1 < bstart.size() && e == hipSuccess; ++bi) {
    e = hipMemcpyAsync(m->d_data.get<double>() + pos, chunks[bi].get(), (size_t)chunk_doubles[bi] * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    pos += chunk_doubles[bi];
  }
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_dims.get(), pad_new.data(), pad_new.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_true.get(), dims_new.data(), dims_new.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_offs.get(), dst.data(), dst.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess && fidelity) e = hipMemcpy(fidelity, d_fid.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && discarded && n > 1) e = hipMemcpy(discarded, d_disc.get(), (size_t)ns * (n - 1) * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    qk_mps_set_destroy(m);
    return qk_fail(QK_EDEVICE, "%s: %s", what, hipGetErrorString(e));
  }
  *out = m;
  return QK_OK;
}

struct qk_built {
  qk_ctx* ctx = nullptr;
  int n_states = 0, n_qubits = 0;
  QkDevBuf heap;  // cd: the packed states, every snapshot of every state (a slot each, in the order the workgroups took them)
  std::vector<int32_t> checkpoints;  // gates done at each snapshot; the last one is the whole program
  // per snapshot j and state s at [j * n_states + s]: bond table, fidelity so far, offset into the heap, orthogonality centre
  std::vector<int32_t> all_dims;
  std::vector<double> all_fidelity;
  std::vector<int64_t> all_offsets;
  std::vector<int32_t> all_centre;
  std::vector<double> all_logw;      // the log-weight of the trajectory so far (0 for a program without channels)
  int n_kgates = 0;                  // channel gates (op codes 10 and 11) of the program
  bool noisy = false;                // built with a channel table, or resumed from such a build: pins the launch shape
  std::vector<int8_t> branches;      // [n_states][n_kgates] the branch every channel gate took (-1: the state stopped before it)
  std::vector<int32_t> dims;  // the last snapshot, the finished states: what qk_built_info and qk_mps_set_from_built read
  std::vector<double> fidelity;
  std::vector<double> secs;  // workgroup time per state
  std::vector<int64_t> offsets;
  int64_t total = 0;  // complex elements of the heap in use
  double kernel_ms = 0;
  int32_t grid = 0, threads = 0, slots = 0;  // the launch: workgroups, threads of each, and the slots (workgroups per CU x CUs) the grid was clipped to
  int n_snapshots() const { return (int)checkpoints.size(); }
};

static const char* const what = "qk_build_program";  // in front of every message of build_impl

// the body of qk_build_program (which has compared the sizes); the QK_EINVAL checks come in the order of the entries this one replaced
static int build_impl(qk_ctx* c, const qk_program& prog, const qk_build_run& run, qk_built** out) {
  const int32_t n_states = prog.n_states, n_qubits = prog.n_qubits, n_ops = prog.n_ops, max_bond = run.max_bond, init_j = run.initial_snapshot;
  const int8_t* const op = prog.op;
  const int32_t* const q0 = prog.q0;
  const double* const alpha = prog.alpha;
  const double trunc_budget = run.trunc_budget, value_of_zero = run.value_of_zero;
  const uint32_t flags = run.flags;
  const qk_built* const init = run.initial;
  std::string wrong;
  if (!qk_program_check_tables(prog, &wrong)) return qk_fail(QK_EINVAL, "%s: %s", what, wrong.c_str());
  const int32_t whole = n_ops;  // without checkpoints: one snapshot after the whole program, which may be empty
  const bool scan = run.checkpoints && run.n_checkpoints > 0;
  const int32_t n_ckpt = scan ? run.n_checkpoints : 1;
  const int32_t* const ckpt = scan ? run.checkpoints : &whole;
  if (run.n_checkpoints < 0) return qk_fail(QK_EINVAL, "%s: no checkpoints", what);
  for (int j = 0; scan && j < n_ckpt; ++j)
    if (ckpt[j] < 1 || ckpt[j] > n_ops || (j > 0 && ckpt[j] <= ckpt[j - 1]))
      return qk_fail(QK_EINVAL, "%s: checkpoints must be strictly increasing gate counts in 1..%d (checkpoint %d is %d)", what, n_ops, j, (int)ckpt[j]);
  if (ckpt[n_ckpt - 1] != n_ops) return qk_fail(QK_EINVAL, "%s: the last checkpoint must be the whole program (%d gates), got %d", what, n_ops, (int)ckpt[n_ckpt - 1]);
  if ((flags & QK_BUILD_PARTIAL) && (n_ckpt > 1 || init))
    return qk_fail(QK_EINVAL, "%s: QK_BUILD_PARTIAL goes with one checkpoint and no initial snapshot (a dropped state has no snapshots)", what);
  if (!c || !op || !q0 || !alpha || !out) return qk_fail(QK_EINVAL, "%s: null argument", what);
  if (n_states <= 0 || n_qubits <= 0 || n_ops < 0) return qk_fail(QK_EINVAL, "%s: empty problem (%d states, %d qubits, %d gates)", what, n_states, n_qubits, n_ops);
  if (max_bond < 2 || max_bond > 1024) return qk_fail(QK_EINVAL, "%s: max_bond %d outside 2..1024", what, max_bond);
  if (qk_program_check(prog, &wrong) != QK_PROGRAM_OK) return qk_fail(QK_EINVAL, "%s: %s", what, wrong.c_str());
  const int n_codes = prog.n_mats > 0 ? N_OPS_MAT : N_OPS;
  const bool with_k1 = prog.n_channels > 0, with_k2 = prog.n_channels2 > 0, with_chan = with_k1 || with_k2;
  const int n_tables = prog.n_mats > 0 ? (prog.mats_state_stride ? n_states : 1) : 0;
  std::vector<int32_t> kgate((size_t)std::max(1, n_ops), 0);  // channel gates before gate i
  int n_kgates = 0, n_k2gates = 0;
  for (int i = 0; with_chan && i < n_ops; ++i) {
    kgate[i] = n_kgates;
    n_kgates += (op[i] == OP_K1 || op[i] == OP_K2);
    n_k2gates += (op[i] == OP_K2);
  }
  if (init) {  // a resumed build starts from snapshot init_j of `init`, which is only read
    if (init->ctx != c) return qk_fail(QK_EINVAL, "%s: the initial snapshot was built in another context", what);
    if (init_j < 0 || init_j >= init->n_snapshots()) return qk_fail(QK_EINVAL, "%s: initial snapshot %d outside 0..%d", what, init_j, init->n_snapshots() - 1);
    if (init->n_states != n_states || init->n_qubits != n_qubits)
      return qk_fail(QK_EINVAL, "%s: the initial snapshot holds %d states of %d qubits, the call has %d of %d", what, init->n_states, init->n_qubits, n_states, n_qubits);
    for (int s = 0; s < n_states; ++s)
      if (init->all_fidelity[(size_t)init_j * n_states + s] < 0) return qk_fail(QK_EINVAL, "%s: state %d of the initial snapshot was dropped (QK_BUILD_PARTIAL)", what, s);
    for (size_t e = 0; e < (size_t)n_states * (n_qubits + 1); ++e) {
      const int d = init->all_dims[(size_t)init_j * n_states * (n_qubits + 1) + e];
      if (d > max_bond) return qk_fail(QK_EINVAL, "%s: the initial snapshot has a bond of %d, beyond max_bond = %d", what, d, max_bond);
    }
  }
  *out = nullptr;
  QkRangeGuard range_("qk:build");
  HIP_TRY(hipSetDevice(c->device));
  const int cap = max_bond;
  size_t lds_meta = (size_t)2 * cap * sizeof(double) + (size_t)2 * cap * sizeof(int) + (size_t)(n_qubits + 1) * sizeof(int);
  lds_meta = (lds_meta + 15) / 16 * 16;
  if (lds_meta > 24 * 1024) return qk_fail(QK_EINVAL, "%s: %d qubits at max_bond %d need %zu bytes of LDS", what, n_qubits, cap, lds_meta);
  // Two workgroups per CU with 76 KiB of LDS each (what the bookkeeping leaves is the Jacobi working set: A and V of a
  // factorisation up to ~(p + q) q = 4500 complex numbers, e.g. 74 x 37; larger ones run from L2) -- or, when the caller
  // bounds the bonds by 32, four with 38 KiB and half the registers each: more latency hiding for small factorisations
  // (cfg5-shaped: 8.0 instead of 10.4 s), worse as soon as many of them spill to the L2 path.  QK_BUILD_WGS=2|4 overrides.
  // Workgroup shape: 256 threads, four workgroups per CU (bonds <= 32) or two -- or, for bonds beyond 64, 512 threads and ONE
  // workgroup per CU with 152 KiB of LDS (qk_build_kernels.h): a heterogeneous data set ends with its few heaviest states, whose
  // block factorisations run one visit per wavefront.  QK_BUILD_WGS=1|2|4 overrides.
  int wgs_variant = (cap <= 32) ? 4 : (cap <= 64 ? 2 : 1);
  // a share with a workgroup slot per state even in the 512-thread shape (<= one state per CU) ends with its slowest state either
  // way, and a state is built faster by 512 threads with the whole CU's LDS: 96 states of 100 qubits x 10 layers cut at bond 64,
  // 60.7 s in the 256-thread shape, 46.8 s in this one (profiles/r03/builder_capped_cfg5_gamma0.5_chi64.txt)
  // -- but not for a program of trajectories (a channel table, or a snapshot of such a build): the two shapes add the channel
  // step's sums and run the factorisations in different orders, and a trajectory's bits must not depend on how many states
  // share its launch (alone, in a set, in one rank's share of many).  Its shape follows from max_bond alone.
  const bool noisy = with_chan || (init && init->noisy);
  if (wgs_variant == 2 && n_states <= c->num_cus && !noisy) wgs_variant = 1;
  if (const char* v = std::getenv("QK_BUILD_WGS")) wgs_variant = (std::atoi(v) >= 4) ? 4 : (std::atoi(v) <= 1 ? 1 : 2);
  const int bt = wgs_variant == 1 ? 512 : 256;
  size_t lds_total = (wgs_variant == 4 ? 38 : wgs_variant == 2 ? 76 : 152) * 1024;
  if (const char* v = std::getenv("QK_BUILD_LDS_KB")) lds_total = (size_t)std::max(32, std::min(wgs_variant == 4 ? 38 : 156, std::atoi(v))) * 1024;
  const int jl_elems = (int)((lds_total - lds_meta) / sizeof(cd));
  if (n_kgates > n_k2gates && jl_elems < 16 + (5 * bt + 6) / 2)  // wg_channel: the staged matrices and five partial sums per thread
    return qk_fail(QK_EINVAL, "%s: the channel step needs %d complex numbers of LDS working set, this shape leaves %d", what, 16 + (5 * bt + 6) / 2, jl_elems);
  // wg_channel_2q: four staged 4x4 matrices, five partial sums per thread, N and the sixteen p_k
  if (n_k2gates > 0 && jl_elems < 64 + (5 * bt + 18) / 2)
    return qk_fail(QK_EINVAL, "%s: the two-qubit channel step needs %d complex numbers of LDS working set, this shape leaves %d", what, 64 + (5 * bt + 18) / 2, jl_elems);
  const size_t lds = lds_total;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb256::qk_build_kernel<2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb256::qk_build_kernel<4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 38 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb512::qk_build_kernel<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
  if (n_kgates > 0) {  // the instantiations with the channel step: a program without channel gates never launches them
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb256::qk_build_kernel<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb256::qk_build_kernel<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 38 * 1024));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb512::qk_build_kernel<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
  }
  const int wgs_per_cu = std::min(wgs_variant, (int)((160 * 1024) / (lds_total + 1024)));  // + the static LDS of the kernel
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t wslot = (size_t)(2 * cap + 32) * (2 * cap + 32);
  const size_t wtab = (((size_t)(2 * cap + 32) / 8) * ((size_t)(2 * cap + 32) / 8) + 3) / 4;
  const size_t per_wg = ((size_t)n_qubits * 2 * cap * cap + 4 * wslot + wtab) * sizeof(cd);
  long long grid = std::min<long long>(n_states, (long long)wgs_per_cu * c->num_cus);
  grid = std::min<long long>(grid, (long long)(0.35 * (double)free_b / (double)per_wg));
  if (grid < 1) return qk_fail(QK_EDEVICE, "%s: not enough device memory for one workgroup's arena (%zu bytes)", what, per_wg);
  // heap: every snapshot of every state, packed; bounded by the arena size of all states and by the free memory
  // (worst case = every bond at the cap; real data sets need a few per cent of that, and allocating -- and freeing -- a hundred GB
  // costs seconds: a twelfth of the free memory unless QK_BUILD_HEAP_GB says otherwise; a heap that turns out too small fails loudly)
  const double heap_want = (double)n_ckpt * (double)n_states * (double)n_qubits * 2.0 * cap * cap;
  double heap_lim = 0.08 * (double)free_b / (double)sizeof(cd);
  if (const char* v = std::getenv("QK_BUILD_HEAP_GB")) heap_lim = std::min(0.45 * (double)free_b, std::atof(v) * 1073741824.0) / (double)sizeof(cd);
  const size_t heap_cap = (size_t)std::max(1024.0, std::min(heap_want, heap_lim));
  const double t_host0 = (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() * 1e-6;
  // the per-workgroup arena and workspace (tens of GB at large bond caps: allocating and releasing them costs seconds) stay with
  // the context between calls -- build_kernel_matrix builds the X and the Y share one after the other -- and go with it
  HIP_TRY_AS(what, c->build_arena.ensure((size_t)grid * n_qubits * 2 * cap * cap * sizeof(cd)));
  HIP_TRY_AS(what, c->build_work.ensure((size_t)grid * (4 * wslot + wtab) * sizeof(cd)));
  QkDevBuf heap, d_op, d_q0, d_alpha, d_fid, d_secs, d_dims, d_offs, d_ctr, d_err, d_order;  // d_ctr: [0] state counter, [1] heap top
  QkDevBuf d_ckpt, d_centre, d_ioffs, d_idims, d_ifid, d_icentre, d_mats, d_mat;
  QkDevBuf d_logw, d_ilogw, d_kraus, d_nkraus, d_kraus2, d_nkraus2, d_channel, d_branch, d_kgate, d_sidx, d_traj, d_bout, d_chan, d_ccol, d_cmask;
  const size_t n_rec = (size_t)n_ckpt * n_states;  // (snapshot, state) records
  HIP_TRY_AS(what, heap.alloc(heap_cap * sizeof(cd)));
  HIP_TRY_AS(what, d_op.alloc(std::max(1, n_ops)));
  HIP_TRY_AS(what, d_q0.alloc((size_t)std::max(1, n_ops) * sizeof(int32_t)));
  HIP_TRY_AS(what, d_alpha.alloc((size_t)n_states * std::max(1, n_ops) * sizeof(double)));
  HIP_TRY_AS(what, d_fid.alloc(n_rec * sizeof(double)));
  HIP_TRY_AS(what, d_secs.alloc((size_t)n_states * sizeof(double)));
  HIP_TRY_AS(what, d_dims.alloc(n_rec * (n_qubits + 1) * sizeof(int32_t)));
  HIP_TRY_AS(what, d_offs.alloc(n_rec * sizeof(long long)));
  HIP_TRY_AS(what, d_centre.alloc(n_rec * sizeof(int32_t)));
  HIP_TRY_AS(what, d_ckpt.alloc((size_t)n_ckpt * sizeof(int32_t)));
  HIP_TRY_AS(what, hipMemcpy(d_ckpt.get(), ckpt, (size_t)n_ckpt * sizeof(int32_t), hipMemcpyHostToDevice));
  if (init) {
    const size_t r0 = (size_t)init_j * n_states;
    std::vector<long long> ioffs(init->all_offsets.begin() + r0, init->all_offsets.begin() + r0 + n_states);
    HIP_TRY_AS(what, d_ioffs.alloc((size_t)n_states * sizeof(long long)));
    HIP_TRY_AS(what, d_idims.alloc((size_t)n_states * (n_qubits + 1) * sizeof(int32_t)));
    HIP_TRY_AS(what, d_ifid.alloc((size_t)n_states * sizeof(double)));
    HIP_TRY_AS(what, d_icentre.alloc((size_t)n_states * sizeof(int32_t)));
    HIP_TRY_AS(what, hipMemcpy(d_ioffs.get(), ioffs.data(), (size_t)n_states * sizeof(long long), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemcpy(d_idims.get(), init->all_dims.data() + r0 * (n_qubits + 1), (size_t)n_states * (n_qubits + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemcpy(d_ifid.get(), init->all_fidelity.data() + r0, (size_t)n_states * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemcpy(d_icentre.get(), init->all_centre.data() + r0, (size_t)n_states * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_kgates > 0) {
      HIP_TRY_AS(what, d_ilogw.alloc((size_t)n_states * sizeof(double)));
      HIP_TRY_AS(what, hipMemcpy(d_ilogw.get(), init->all_logw.data() + r0, (size_t)n_states * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  if (n_kgates > 0) {  // the channel table, the branch rows and the names of the trajectories
    const size_t rows = prog.branch_state_stride ? (size_t)n_states : 1;
    std::vector<uint32_t> sidx(n_states), traj(n_states, 0u);
    for (int s = 0; s < n_states; ++s) sidx[s] = prog.state_index ? prog.state_index[s] : (uint32_t)s;
    if (prog.trajectory) traj.assign(prog.trajectory, prog.trajectory + n_states);
    HIP_TRY_AS(what, d_kraus.alloc(std::max<size_t>(1, prog.n_channels) * 16 * sizeof(cd)));
    HIP_TRY_AS(what, d_nkraus.alloc(std::max<size_t>(1, prog.n_channels) * sizeof(int32_t)));
    if (with_k2) {
      HIP_TRY_AS(what, d_kraus2.alloc((size_t)prog.n_channels2 * 256 * sizeof(cd)));
      HIP_TRY_AS(what, d_nkraus2.alloc((size_t)prog.n_channels2 * sizeof(int32_t)));
      HIP_TRY_AS(what, hipMemcpy(d_kraus2.get(), prog.kraus2, (size_t)prog.n_channels2 * 256 * sizeof(cd), hipMemcpyHostToDevice));
      HIP_TRY_AS(what, hipMemcpy(d_nkraus2.get(), prog.n_kraus2, (size_t)prog.n_channels2 * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    HIP_TRY_AS(what, d_channel.alloc((size_t)n_ops * sizeof(int32_t)));
    HIP_TRY_AS(what, d_branch.alloc(rows * n_ops * sizeof(int32_t)));
    HIP_TRY_AS(what, d_kgate.alloc((size_t)n_ops * sizeof(int32_t)));
    HIP_TRY_AS(what, d_sidx.alloc((size_t)n_states * sizeof(uint32_t)));
    HIP_TRY_AS(what, d_traj.alloc((size_t)n_states * sizeof(uint32_t)));
    HIP_TRY_AS(what, d_bout.alloc((size_t)n_states * n_kgates));
    if (with_k1) {
      HIP_TRY_AS(what, hipMemcpy(d_kraus.get(), prog.kraus, (size_t)prog.n_channels * 16 * sizeof(cd), hipMemcpyHostToDevice));
      HIP_TRY_AS(what, hipMemcpy(d_nkraus.get(), prog.n_kraus, (size_t)prog.n_channels * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    HIP_TRY_AS(what, hipMemcpy(d_channel.get(), prog.channel, (size_t)n_ops * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemcpy(d_branch.get(), prog.branch, rows * n_ops * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemcpy(d_kgate.get(), kgate.data(), (size_t)n_ops * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemcpy(d_sidx.get(), sidx.data(), (size_t)n_states * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemcpy(d_traj.get(), traj.data(), (size_t)n_states * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(what, hipMemset(d_bout.get(), 0xFF, (size_t)n_states * n_kgates));  // -1: not reached
    HIP_TRY_AS(what, d_logw.alloc(n_rec * sizeof(double)));
    ChanArgs ca;
    ca.kraus2 = with_k2 ? d_kraus2.get<cd>() : nullptr, ca.n_kraus2 = with_k2 ? d_nkraus2.get<int32_t>() : nullptr;
    ca.kraus = d_kraus.get<cd>(), ca.n_kraus = d_nkraus.get<int32_t>(), ca.channel = d_channel.get<int32_t>(), ca.branch = d_branch.get<int32_t>();
    ca.cond_col = nullptr, ca.cond_mask = nullptr;
    bool conditional = false;
    for (int i = 0; prog.cond_gate && i < n_ops; ++i) conditional = conditional || prog.cond_gate[i] >= 0;
    if (conditional) {  // rows whose gates are all unconditional are no rows: the kernel then does what it does without them
      std::vector<int32_t> ccol((size_t)n_ops);
      for (int i = 0; i < n_ops; ++i) ccol[i] = prog.cond_gate[i] >= 0 ? kgate[prog.cond_gate[i]] : -1;
      HIP_TRY_AS(what, d_ccol.alloc((size_t)n_ops * sizeof(int32_t)));
      HIP_TRY_AS(what, d_cmask.alloc((size_t)n_ops * sizeof(uint32_t)));
      HIP_TRY_AS(what, hipMemcpy(d_ccol.get(), ccol.data(), (size_t)n_ops * sizeof(int32_t), hipMemcpyHostToDevice));
      HIP_TRY_AS(what, hipMemcpy(d_cmask.get(), prog.cond_mask, (size_t)n_ops * sizeof(uint32_t), hipMemcpyHostToDevice));
      ca.cond_col = d_ccol.get<int32_t>(), ca.cond_mask = d_cmask.get<uint32_t>();
    }
    ca.kgate = d_kgate.get<int32_t>(), ca.branch_stride = prog.branch_state_stride ? n_ops : 0, ca.n_kgates = n_kgates;
    ca.seed_lo = (unsigned)prog.seed, ca.seed_hi = (unsigned)(prog.seed >> 32), ca.first_gate = prog.first_gate;
    ca.state_index = d_sidx.get<uint32_t>(), ca.trajectory = d_traj.get<uint32_t>(), ca.branch_out = d_bout.get<int8_t>();
    ca.logw_out = d_logw.get<double>(), ca.init_logw = d_ilogw.get<double>();
    HIP_TRY_AS(what, d_chan.alloc(sizeof(ChanArgs)));
    HIP_TRY_AS(what, hipMemcpy(d_chan.get(), &ca, sizeof(ChanArgs), hipMemcpyHostToDevice));
  }
  if (n_tables) {
    const size_t mats_bytes = (size_t)n_tables * prog.n_mats * 16 * sizeof(cd);
    HIP_TRY_AS(what, d_mats.alloc(mats_bytes));
    HIP_TRY_AS(what, d_mat.alloc((size_t)std::max(1, n_ops) * sizeof(int32_t)));
    HIP_TRY_AS(what, hipMemcpy(d_mats.get(), prog.mats, mats_bytes, hipMemcpyHostToDevice));
    if (n_ops > 0) HIP_TRY_AS(what, hipMemcpy(d_mat.get(), prog.mat, (size_t)n_ops * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  HIP_TRY_AS(what, d_ctr.alloc(2 * sizeof(unsigned long long)));
  HIP_TRY_AS(what, d_err.alloc(32 * sizeof(int)));
  if (n_ops > 0) {
    HIP_TRY_AS(what, hipMemcpyAsync(d_op.get(), op, n_ops, hipMemcpyHostToDevice, c->stream));
    HIP_TRY_AS(what, hipMemcpyAsync(d_q0.get(), q0, (size_t)n_ops * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY_AS(what, hipMemcpyAsync(d_alpha.get(), alpha, (size_t)n_states * n_ops * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY_AS(what, hipMemsetAsync(d_ctr.get(), 0, 2 * sizeof(unsigned long long), c->stream));
  HIP_TRY_AS(what, hipMemsetAsync(d_err.get(), 0, 32 * sizeof(int), c->stream));
  // Queue order: longest expected first.  The cost of a state grows with its bonds, and those with the entangling power
  // of its XXPhase / YYPhase / ZZPhase gates, sin^2(pi alpha) summed over the gates -- a cheap proxy that keeps the tail of the launch short.
  // Matrix gates (op codes 8 and 9) add nothing to it: a shared table costs every state the same, and the entangling power of a
  // per-state 4x4 is not worth a factorisation on the host.
  std::vector<int32_t> order(n_states);
  {
    std::vector<double> proxy(n_states, 0.0);
    for (int s = 0; s < n_states; ++s)
      for (int i = 0; i < n_ops; ++i)
        if (op[i] == OP_XX || op[i] == OP_YY || op[i] == OP_ZZ) {
          const double sn = std::sin(M_PI * alpha[(size_t)s * n_ops + i]);
          proxy[s] += sn * sn;
        }
    for (int s = 0; s < n_states; ++s) order[s] = s;
    if (!std::getenv("QK_BUILD_NO_ORDER")) std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return proxy[x] > proxy[y]; });
  }
  HIP_TRY_AS(what, d_order.alloc((size_t)n_states * sizeof(int32_t)));
  HIP_TRY_AS(what, hipMemcpyAsync(d_order.get(), order.data(), (size_t)n_states * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  BuildArgs a;
  a.order = d_order.get<int32_t>();
  a.n_states = n_states, a.n_qubits = n_qubits, a.n_ops = n_ops, a.cap = cap;
  a.op = d_op.get<int8_t>(), a.q0 = d_q0.get<int32_t>(), a.alpha = d_alpha.get<double>();
  a.mats = n_tables ? d_mats.get<cd>() : nullptr, a.mat = n_tables ? d_mat.get<int32_t>() : nullptr, a.mats_stride = n_tables > 1 ? prog.n_mats : 0;
  a.chan = n_kgates ? d_chan.get<ChanArgs>() : nullptr;
  a.budget = trunc_budget, a.zero = value_of_zero;
  a.arena = c->build_arena.get<cd>(), a.work = c->build_work.get<cd>(), a.heap = heap.get<cd>(), a.heap_cap = heap_cap;
  a.counter = d_ctr.get<unsigned long long>(), a.heap_top = a.counter + 1;
  a.dims_out = d_dims.get<int32_t>(), a.fid_out = d_fid.get<double>(), a.secs_out = d_secs.get<double>(), a.offs_out = d_offs.get<long long>(), a.error = d_err.get<int>();
  a.jl_offset = (int)(lds_meta / sizeof(double)), a.jl_elems = jl_elems;
  a.n_ckpt = n_ckpt, a.ckpt = d_ckpt.get<int32_t>(), a.centre_out = d_centre.get<int32_t>();
  a.init_heap = init ? init->heap.get<cd>() : nullptr;
  a.init_offs = d_ioffs.get<long long>(), a.init_dims = d_idims.get<int32_t>(), a.init_fid = d_ifid.get<double>(), a.init_centre = d_icentre.get<int32_t>();
  a.partial = (flags & QK_BUILD_PARTIAL) ? 1 : 0;
  a.truncate = (flags & QK_BUILD_TRUNCATE) ? 1 : 0;
  a.block = 1;
  if (const char* v = std::getenv("QK_BUILD_BLOCK")) a.block = std::atoi(v) != 0;
  HIP_TRY_AS(what, hipEventRecord(c->ev0, c->stream));
  if (n_kgates > 0) {
    if (wgs_variant == 4) qkb256::qk_build_kernel<4, true><<<dim3((unsigned)grid), dim3(bt), lds, c->stream>>>(a);
    else if (wgs_variant == 2) qkb256::qk_build_kernel<2, true><<<dim3((unsigned)grid), dim3(bt), lds, c->stream>>>(a);
    else qkb512::qk_build_kernel<1, true><<<dim3((unsigned)grid), dim3(bt), lds, c->stream>>>(a);
  } else if (wgs_variant == 4) qkb256::qk_build_kernel<4, false><<<dim3((unsigned)grid), dim3(bt), lds, c->stream>>>(a);
  else if (wgs_variant == 2) qkb256::qk_build_kernel<2, false><<<dim3((unsigned)grid), dim3(bt), lds, c->stream>>>(a);
  else qkb512::qk_build_kernel<1, false><<<dim3((unsigned)grid), dim3(bt), lds, c->stream>>>(a);
  HIP_TRY_AS(what, hipGetLastError());
  HIP_TRY_AS(what, hipEventRecord(c->ev1, c->stream));
  std::unique_ptr<qk_built> b(new (std::nothrow) qk_built);
  if (!b) return qk_fail(QK_ENOMEM, "%s: out of memory", what);
  b->ctx = c, b->n_states = n_states, b->n_qubits = n_qubits;
  b->checkpoints.assign(ckpt, ckpt + n_ckpt);
  b->all_dims.resize(n_rec * (n_qubits + 1));
  b->all_fidelity.resize(n_rec);
  b->all_offsets.resize(n_rec);
  b->all_centre.resize(n_rec);
  b->all_logw.assign(n_rec, 0.0);
  if (init && n_kgates == 0)  // a resumed tail without channel gates: every record keeps the log-weight of the snapshot
    for (size_t r = 0; r < n_rec; ++r) b->all_logw[r] = init->all_logw[(size_t)init_j * n_states + r % n_states];
  b->n_kgates = n_kgates;
  b->noisy = noisy;
  b->branches.assign((size_t)n_states * n_kgates, (int8_t)-1);
  std::vector<long long> offs(n_rec);
  int errv[32] = {0};
  unsigned long long ctr[2] = {0, 0};
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(b->all_dims.data(), d_dims.get(), b->all_dims.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(b->all_fidelity.data(), d_fid.get(), n_rec * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(b->all_centre.data(), d_centre.get(), n_rec * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && n_kgates > 0) e = hipMemcpy(b->all_logw.data(), d_logw.get(), n_rec * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && n_kgates > 0) e = hipMemcpy(b->branches.data(), d_bout.get(), b->branches.size(), hipMemcpyDeviceToHost);
  b->secs.resize(n_states);
  if (e == hipSuccess) e = hipMemcpy(b->secs.data(), d_secs.get(), (size_t)n_states * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(offs.data(), d_offs.get(), n_rec * sizeof(long long), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(errv, d_err.get(), sizeof(errv), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ctr, d_ctr.get(), sizeof(ctr), hipMemcpyDeviceToHost);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
  if (std::getenv("QK_BUILD_DEBUG")) {
    const double t_host1 = (double)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() * 1e-6;
    std::fprintf(stderr, "[qk_build_mps] host wall %.2f s for a %.2f s launch (arena %.1f GB, heap %.1f GB: allocation, upload, download)\n", t_host1 - t_host0, ms / 1e3,
                 (double)grid * (double)per_wg / 1e9, (double)heap_cap * sizeof(cd) / 1e9);
  }
  if (e != hipSuccess) return qk_fail(QK_EDEVICE, "%s: %s", what, hipGetErrorString(e));
  const int err = errv[0];
  if (std::getenv("QK_BUILD_DEBUG"))
    std::fprintf(stderr, "[qk_build_mps] %d states, grid %lld x %d threads, %.1f ms; Jacobi: %d factorisations, %.2f sweeps on average, %d at most, %d unconverged, %d in LDS / %d from L2; error bits %d\n",
                 n_states, grid, bt, ms, errv[1], errv[1] ? (double)errv[2] / errv[1] : 0.0, errv[3], errv[4], errv[5], errv[6], err);
  if (std::getenv("QK_BUILD_DEBUG") && errv[7]) {
    unsigned long long tk[5];
    for (int i = 0; i < 5; ++i) std::memcpy(&tk[i], errv + 14 + 2 * i, 8);
    std::fprintf(stderr, "[qk_build_mps] %d centre moves of large sites by Gram-Schmidt twice (no sweeps)\n", errv[24]);
    std::fprintf(stderr, "[qk_build_mps] %d preconditioned block factorisations: %.3f s of workgroup time (sort+copy %.1f %%, Gram-Schmidt %.1f %%, sweeps %.1f %%, V and W = A V %.1f %%)\n", errv[7],
                 (double)tk[0] / 1e8, 100.0 * tk[1] / std::max(1ull, tk[0]), 100.0 * tk[2] / std::max(1ull, tk[0]), 100.0 * tk[3] / std::max(1ull, tk[0]), 100.0 * tk[4] / std::max(1ull, tk[0]));
  }
  if (std::getenv("QK_BUILD_DEBUG")) {
    std::vector<double> t(b->secs);
    std::sort(t.begin(), t.end());
    double sum = 0;
    for (double x : t) sum += x;
    std::fprintf(stderr, "[qk_build_mps] workgroup time per state: median %.3f s, 90 %% %.3f s, the three longest %.3f %.3f %.3f s; sum %.1f s = %.2f s per workgroup slot\n", t[t.size() / 2], t[(size_t)(0.9 * (t.size() - 1))],
                 t[t.size() >= 3 ? t.size() - 3 : 0], t[t.size() >= 2 ? t.size() - 2 : 0], t.back(), sum, sum / (double)grid);
  }
  if (std::getenv("QK_BUILD_DEBUG")) {
    unsigned long long ticks = 0, steps = 0;
    std::memcpy(&ticks, errv + 8, 8), std::memcpy(&steps, errv + 10, 8);
    unsigned long long busy = 0;
    std::memcpy(&busy, errv + 12, 8);
    std::fprintf(stderr, "[qk_build_mps] workgroups busy %.1f %% of the launch (%.3f s of workgroup time per state); sweeps are %.1f %% of the busy time (%.2f us per step, %llu steps)\n",
                 100.0 * (double)busy / 1e8 / ((double)grid * ms / 1e3), (double)busy / 1e8 / n_states, 100.0 * (double)ticks / (double)std::max(1ull, busy),
                 steps ? (double)ticks / 100.0 / (double)steps : 0.0, steps);
  }
  if (err) {
    if (err & ERR_OP) return qk_fail(QK_EINVAL, "%s: unknown gate op code (valid: 0..%d)", what, n_codes - 1);
    if (err & ERR_CHANNEL)
      return qk_fail(QK_EDEVICE, "%s: state %d (state_index %u), gate %u: the branch of the channel has probability 0 or one that is not finite (an impossible outcome was post-selected?)",
                     what, errv[26] - 1, prog.state_index ? prog.state_index[std::max(0, errv[26] - 1)] : (uint32_t)std::max(0, errv[26] - 1), prog.first_gate + (unsigned)errv[27]);
    if (err & ERR_GATE) return qk_fail(QK_EINVAL, "%s: gate on a qubit outside the register", what);
    if (err & ERR_BOND) return qk_fail(QK_EINVAL, "%s: a bond grew beyond max_bond = %d", what, cap);
    if (err & ERR_HEAP) return qk_fail(QK_EDEVICE, "%s: the packed states (%d snapshots each) need %llu complex numbers, the heap holds %zu", what, n_ckpt, ctr[1], heap_cap);
    return qk_fail(QK_EDEVICE, "%s: a Jacobi factorisation did not converge in %d sweeps", what, MAX_SWEEPS);
  }
  for (size_t r = 0; r < n_rec; ++r) b->all_offsets[r] = offs[r];
  const size_t last = (size_t)(n_ckpt - 1) * n_states;
  b->dims.assign(b->all_dims.begin() + last * (n_qubits + 1), b->all_dims.end());
  b->fidelity.assign(b->all_fidelity.begin() + last, b->all_fidelity.end());
  b->offsets.assign(b->all_offsets.begin() + last, b->all_offsets.end());
  b->heap = std::move(heap);
  b->total = (int64_t)ctr[1];
  b->kernel_ms = ms;
  b->grid = (int32_t)grid, b->threads = bt, b->slots = (int32_t)std::min<long long>(INT32_MAX, (long long)wgs_per_cu * c->num_cus);
  *out = b.release();
  return QK_OK;
}

extern "C" uint32_t qk_program_size(void) { return (uint32_t)sizeof(qk_program); }
extern "C" uint32_t qk_build_run_size(void) { return (uint32_t)sizeof(qk_build_run); }

extern "C" int qk_build_program(qk_ctx* c, const qk_program* prog, const qk_build_run* run, qk_built** out) {
  if (!prog || !run) return qk_fail(QK_EINVAL, "%s: null argument", what);
  if (prog->size != sizeof(qk_program)) return qk_fail(QK_EINVAL, "%s: qk_program.size is %u, this library's is %zu", what, prog->size, sizeof(qk_program));
  if (run->size != sizeof(qk_build_run)) return qk_fail(QK_EINVAL, "%s: qk_build_run.size is %u, this library's is %zu", what, run->size, sizeof(qk_build_run));
  return build_impl(c, *prog, *run, out);
}

// ---- the entries from before qk_program: each fills the two structs, calls qk_build_program and puts its own name in front of an error
static qk_program plain_program(int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha) {
  qk_program p{};
  p.size = sizeof p, p.n_states = n_states, p.n_qubits = n_qubits, p.n_ops = n_ops, p.op = op, p.q0 = q0, p.alpha = alpha;
  return p;
}

static qk_build_run plain_run(double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags) {
  qk_build_run r{};
  r.size = sizeof r, r.trunc_budget = trunc_budget, r.value_of_zero = value_of_zero, r.max_bond = max_bond, r.flags = flags;
  return r;
}

// plain_run with the checkpoints these entries insist on (a negative count is refused as "no checkpoints") and the snapshot to resume
static qk_build_run scan_run(double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const int32_t* checkpoints, const qk_built* initial,
                             int32_t initial_snapshot) {
  qk_build_run r = plain_run(trunc_budget, value_of_zero, max_bond, flags);
  r.n_checkpoints = checkpoints && n_checkpoints >= 1 ? n_checkpoints : -1, r.checkpoints = checkpoints, r.initial = initial, r.initial_snapshot = initial_snapshot;
  return r;
}

static void set_mats(qk_program& p, int32_t n_mats, const double* mats, int32_t mats_state_stride, const int32_t* mat) {
  p.n_mats = n_mats, p.mats = mats, p.mats_state_stride = mats_state_stride, p.mat = mat;
}

static void set_channels(qk_program& p, int32_t n_channels, const double* kraus, const int32_t* n_kraus, const int32_t* channel, const int32_t* branch, int32_t branch_state_stride,
                         uint64_t seed, const uint32_t* state_index, const uint32_t* trajectory, uint32_t first_gate) {
  p.n_channels = n_channels, p.kraus = kraus, p.n_kraus = n_kraus, p.channel = channel, p.branch = branch, p.branch_state_stride = branch_state_stride;
  p.seed = seed, p.state_index = state_index, p.trajectory = trajectory, p.first_gate = first_gate;
}

static int as_entry(const char* name, int rc) {  // rc of qk_build_program, its message under the name of the entry the caller came through
  const std::string msg = qk_last_error();
  return rc != QK_OK && msg.rfind(what, 0) == 0 ? qk_fail(rc, "%s%s", name, msg.c_str() + std::strlen(what)) : rc;
}

extern "C" int qk_build_mps(qk_ctx* c, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0,
                            const double* alpha, double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, qk_built** out) {
  const qk_program p = plain_program(n_states, n_qubits, n_ops, op, q0, alpha);
  const qk_build_run r = plain_run(trunc_budget, value_of_zero, max_bond, flags);
  return as_entry("qk_build_mps", qk_build_program(c, &p, &r, out));
}

extern "C" int qk_build_mps_scan(qk_ctx* c, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget,
                                 double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const int32_t* checkpoints, const qk_built* initial,
                                 int32_t initial_snapshot, qk_built** out) {
  const qk_program p = plain_program(n_states, n_qubits, n_ops, op, q0, alpha);
  const qk_build_run r = scan_run(trunc_budget, value_of_zero, max_bond, flags, n_checkpoints, checkpoints, initial, initial_snapshot);
  return as_entry("qk_build_mps_scan", qk_build_program(c, &p, &r, out));
}

extern "C" int qk_build_mps_gates(qk_ctx* c, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget,
                                  double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const int32_t* checkpoints, const qk_built* initial,
                                  int32_t initial_snapshot, int32_t n_mats, const double* mats, int32_t mats_state_stride, const int32_t* mat, qk_built** out) {
  qk_program p = plain_program(n_states, n_qubits, n_ops, op, q0, alpha);
  set_mats(p, n_mats, mats, mats_state_stride, mat);
  const qk_build_run r = scan_run(trunc_budget, value_of_zero, max_bond, flags, n_checkpoints, checkpoints, initial, initial_snapshot);
  return as_entry("qk_build_mps_gates", qk_build_program(c, &p, &r, out));
}

extern "C" int qk_build_mps_channels(qk_ctx* c, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget,
                                     double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const int32_t* checkpoints, const qk_built* initial,
                                     int32_t initial_snapshot, int32_t n_mats, const double* mats, int32_t mats_state_stride, const int32_t* mat, int32_t n_channels,
                                     const double* kraus, const int32_t* n_kraus, const int32_t* channel, const int32_t* branch, int32_t branch_state_stride, uint64_t seed,
                                     const uint32_t* state_index, const uint32_t* trajectory, uint32_t first_gate, qk_built** out) {
  qk_program p = plain_program(n_states, n_qubits, n_ops, op, q0, alpha);
  set_mats(p, n_mats, mats, mats_state_stride, mat);
  set_channels(p, n_channels, kraus, n_kraus, channel, branch, branch_state_stride, seed, state_index, trajectory, first_gate);
  const qk_build_run r = scan_run(trunc_budget, value_of_zero, max_bond, flags, n_checkpoints, checkpoints, initial, initial_snapshot);
  return as_entry("qk_build_mps_channels", qk_build_program(c, &p, &r, out));
}

extern "C" int qk_build_mps_channels2(qk_ctx* c, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget,
                                      double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const int32_t* checkpoints, const qk_built* initial,
                                      int32_t initial_snapshot, int32_t n_mats, const double* mats, int32_t mats_state_stride, const int32_t* mat, int32_t n_channels,
                                      const double* kraus, const int32_t* n_kraus, const int32_t* channel, const int32_t* branch, int32_t branch_state_stride, uint64_t seed,
                                      const uint32_t* state_index, const uint32_t* trajectory, uint32_t first_gate, int32_t n_channels2, const double* kraus2,
                                      const int32_t* n_kraus2, qk_built** out) {
  qk_program p = plain_program(n_states, n_qubits, n_ops, op, q0, alpha);
  set_mats(p, n_mats, mats, mats_state_stride, mat);
  set_channels(p, n_channels, kraus, n_kraus, channel, branch, branch_state_stride, seed, state_index, trajectory, first_gate);
  p.n_channels2 = n_channels2, p.kraus2 = kraus2, p.n_kraus2 = n_kraus2;
  const qk_build_run r = scan_run(trunc_budget, value_of_zero, max_bond, flags, n_checkpoints, checkpoints, initial, initial_snapshot);
  return as_entry("qk_build_mps_channels2", qk_build_program(c, &p, &r, out));
}

extern "C" int qk_build_mps_conditions(qk_ctx* c, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget,
                                       double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const int32_t* checkpoints, const qk_built* initial,
                                       int32_t initial_snapshot, int32_t n_mats, const double* mats, int32_t mats_state_stride, const int32_t* mat, int32_t n_channels,
                                       const double* kraus, const int32_t* n_kraus, const int32_t* channel, const int32_t* branch, int32_t branch_state_stride, uint64_t seed,
                                       const uint32_t* state_index, const uint32_t* trajectory, uint32_t first_gate, int32_t n_channels2, const double* kraus2,
                                       const int32_t* n_kraus2, const int32_t* cond_gate, const uint32_t* cond_mask, qk_built** out) {
  qk_program p = plain_program(n_states, n_qubits, n_ops, op, q0, alpha);
  set_mats(p, n_mats, mats, mats_state_stride, mat);
  set_channels(p, n_channels, kraus, n_kraus, channel, branch, branch_state_stride, seed, state_index, trajectory, first_gate);
  p.n_channels2 = n_channels2, p.kraus2 = kraus2, p.n_kraus2 = n_kraus2, p.cond_gate = cond_gate, p.cond_mask = cond_mask;
  const qk_build_run r = scan_run(trunc_budget, value_of_zero, max_bond, flags, n_checkpoints, checkpoints, initial, initial_snapshot);
  return as_entry("qk_build_mps_conditions", qk_build_program(c, &p, &r, out));
}

extern "C" int qk_built_info(const qk_built* b, int32_t* dims, double* fidelity, int64_t* offsets, int64_t* total_complex, double* kernel_ms) {
  if (!b) return qk_fail(QK_EINVAL, "qk_built_info: null handle");
  if (dims) std::copy(b->dims.begin(), b->dims.end(), dims);
  if (fidelity) std::copy(b->fidelity.begin(), b->fidelity.end(), fidelity);
  if (offsets) std::copy(b->offsets.begin(), b->offsets.end(), offsets);
  if (total_complex) *total_complex = b->total;
  if (kernel_ms) *kernel_ms = b->kernel_ms;
  return QK_OK;
}

extern "C" int qk_built_launch(const qk_built* b, int32_t* grid, int32_t* threads, int32_t* slots) {
  if (!b) return qk_fail(QK_EINVAL, "qk_built_launch: null handle");
  if (grid) *grid = b->grid;
  if (threads) *threads = b->threads;
  if (slots) *slots = b->slots;
  return QK_OK;
}

extern "C" int qk_built_download(const qk_built* b, double* host) {
  if (!b || !host) return qk_fail(QK_EINVAL, "qk_built_download: null argument");
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipMemcpy(host, b->heap.get(), (size_t)b->total * sizeof(cd), hipMemcpyDeviceToHost));
  return QK_OK;
}

extern "C" int qk_built_num_snapshots(const qk_built* b) { return b ? b->n_snapshots() : 0; }

extern "C" int qk_built_checkpoints(const qk_built* b, int32_t* checkpoints) {
  if (!b || !checkpoints) return qk_fail(QK_EINVAL, "qk_built_checkpoints: null argument");
  std::copy(b->checkpoints.begin(), b->checkpoints.end(), checkpoints);
  return QK_OK;
}

static int snapshot_index(const qk_built* b, int32_t j, const char* what) {
  if (!b) return qk_fail(QK_EINVAL, "%s: null handle", what);
  if (j < 0 || j >= b->n_snapshots()) return qk_fail(QK_EINVAL, "%s: snapshot %d outside 0..%d", what, j, b->n_snapshots() - 1);
  return QK_OK;
}

static int64_t state_elems(const qk_built* b, int32_t j, int s) {  // complex elements of state s in snapshot j (0 for a dropped state)
  const size_t r = (size_t)j * b->n_states + s;
  if (b->all_fidelity[r] < 0) return 0;
  const int32_t* d = b->all_dims.data() + r * (b->n_qubits + 1);
  int64_t t = 0;
  for (int k = 0; k < b->n_qubits; ++k) t += 2ll * d[k] * d[k + 1];
  return t;
}

extern "C" int qk_built_info_at(const qk_built* b, int32_t j, int32_t* dims, double* fidelity, int64_t* offsets, int32_t* centre, int64_t* total_complex) {
  if (const int rc = snapshot_index(b, j, "qk_built_info_at")) return rc;
  const size_t ns = b->n_states, n1 = b->n_qubits + 1, r0 = (size_t)j * ns;
  if (dims) std::copy(b->all_dims.begin() + r0 * n1, b->all_dims.begin() + (r0 + ns) * n1, dims);
  if (fidelity) std::copy(b->all_fidelity.begin() + r0, b->all_fidelity.begin() + r0 + ns, fidelity);
  if (offsets) std::copy(b->all_offsets.begin() + r0, b->all_offsets.begin() + r0 + ns, offsets);
  if (centre) std::copy(b->all_centre.begin() + r0, b->all_centre.begin() + r0 + ns, centre);
  if (total_complex) {
    int64_t t = 0;
    for (int s = 0; s < b->n_states; ++s) t += state_elems(b, j, s);
    *total_complex = t;
  }
  return QK_OK;
}

extern "C" int qk_built_logw_at(const qk_built* b, int32_t j, double* logw) {
  if (const int rc = snapshot_index(b, j, "qk_built_logw_at")) return rc;
  if (!logw) return qk_fail(QK_EINVAL, "qk_built_logw_at: null argument");
  std::copy(b->all_logw.begin() + (size_t)j * b->n_states, b->all_logw.begin() + (size_t)(j + 1) * b->n_states, logw);
  return QK_OK;
}

extern "C" int qk_built_num_channel_gates(const qk_built* b) { return b ? b->n_kgates : 0; }

extern "C" int qk_built_branches(const qk_built* b, int8_t* branches) {
  if (!b) return qk_fail(QK_EINVAL, "qk_built_branches: null handle");
  if (b->n_kgates > 0 && !branches) return qk_fail(QK_EINVAL, "qk_built_branches: null argument");
  std::copy(b->branches.begin(), b->branches.end(), branches);
  return QK_OK;
}

extern "C" int qk_built_download_at(const qk_built* b, int32_t j, double* host) {
  if (const int rc = snapshot_index(b, j, "qk_built_download_at")) return rc;
  if (!host) return qk_fail(QK_EINVAL, "qk_built_download_at: null argument");
  HIP_TRY(hipSetDevice(b->ctx->device));
  cd* dst = reinterpret_cast<cd*>(host);
  for (int s = 0; s < b->n_states; ++s) {  // a snapshot's states lie where their workgroups' bumps put them: one copy each, packed in state order
    const int64_t cnt = state_elems(b, j, s), off = b->all_offsets[(size_t)j * b->n_states + s];
    if (cnt == 0) continue;
    if (off < 0 || off + cnt > b->total) return qk_fail(QK_EDEVICE, "qk_built_download_at: state %d of snapshot %d lies outside the heap", s, j);
    HIP_TRY(hipMemcpy(dst, b->heap.get<cd>() + off, (size_t)cnt * sizeof(cd), hipMemcpyDeviceToHost));
    dst += cnt;
  }
  return QK_OK;
}

static int set_from_snapshot(qk_ctx* c, const qk_built* b, int32_t j, qk_mps_set** out, const char* what);

extern "C" int qk_mps_set_from_built(qk_ctx* c, const qk_built* b, qk_mps_set** out) {
  if (!c || !b || !out) return qk_fail(QK_EINVAL, "qk_mps_set_from_built: null argument");
  return set_from_snapshot(c, b, b->n_snapshots() - 1, out, "qk_mps_set_from_built");
}

extern "C" int qk_mps_set_from_built_at(qk_ctx* c, const qk_built* b, int32_t j, qk_mps_set** out) {
  if (!c || !b || !out) return qk_fail(QK_EINVAL, "qk_mps_set_from_built_at: null argument");
  if (const int rc = snapshot_index(b, j, "qk_mps_set_from_built_at")) return rc;
  return set_from_snapshot(c, b, j, out, "qk_mps_set_from_built_at");
}

// qk_pack_built_kernel with the offsets and bond tables of snapshot j
static int set_from_snapshot(qk_ctx* c, const qk_built* b, const int32_t j, qk_mps_set** out, const char* what) {
  if (b->ctx != c) return qk_fail(QK_EINVAL, "%s: the states were built in another context", what);
  const size_t r0 = (size_t)j * b->n_states;
  const int32_t* const bdims = b->all_dims.data() + r0 * (b->n_qubits + 1);
  const int64_t* const boffs = b->all_offsets.data() + r0;
  for (int s = 0; s < b->n_states; ++s)
    if (b->all_fidelity[r0 + s] < 0) return qk_fail(QK_EINVAL, "%s: state %d outgrew max_bond and was dropped (QK_BUILD_PARTIAL)", what, s);
  HIP_TRY(hipSetDevice(c->device));
  const int ns = b->n_states, n = b->n_qubits, stride = n + 1;
  auto pad16 = [](int x) { return (x + 15) / 16 * 16; };
  std::vector<int32_t> pad((size_t)ns * stride);
  std::vector<long long> src((size_t)ns * n), dst((size_t)ns * n);
  long long total = 0;
  int max_pad = 0;
  for (int s = 0; s < ns; ++s) {
    long long pos = boffs[s];
    for (int k = 0; k <= n; ++k) {
      pad[(size_t)s * stride + k] = pad16(bdims[(size_t)s * stride + k]);
      max_pad = std::max(max_pad, pad[(size_t)s * stride + k]);
    }
    for (int k = 0; k < n; ++k) {
      src[(size_t)s * n + k] = pos;
      dst[(size_t)s * n + k] = total;
      pos += 2ll * bdims[(size_t)s * stride + k] * bdims[(size_t)s * stride + k + 1];
      total += 2ll * pad[(size_t)s * stride + k] * 2 * pad[(size_t)s * stride + k + 1];
    }
  }
  qk_mps_set* m = nullptr;
  const int rc = qk_mps_set_alloc(c, ns, n, total * (long long)sizeof(double), 64, &m, what);
  if (rc != QK_OK) return rc;
  m->max_pad = max_pad;
  m->dims_true.assign(bdims, bdims + (size_t)ns * stride);
  m->centre = b->all_centre[r0];  // the states of a snapshot share their centre unless conditional gates moved it apart: then the gauge counts as unknown
  for (int s = 1; s < ns; ++s)
    if (b->all_centre[r0 + s] != m->centre) m->centre = -1;
  QkDevBuf d_src;
  hipError_t e = hipMemsetAsync(m->d_data.get(), 0, (size_t)m->bytes, c->stream);
  if (e == hipSuccess) e = d_src.alloc(src.size() * sizeof(long long));
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_dims.get(), pad.data(), pad.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_true.get(), bdims, pad.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_offs.get(), dst.data(), dst.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_src.get(), src.data(), src.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    qk_pack_built_kernel<<<dim3((unsigned)(ns * n)), dim3(256), 0, c->stream>>>(b->heap.get<cd>(), d_src.get<long long>(), m->d_offs.get<long long>(), m->d_true.get<int32_t>(),
                                                                              m->d_dims.get<int32_t>(), n, m->d_data.get<double>());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    qk_mps_set_destroy(m);
    return qk_fail(QK_EDEVICE, "%s: %s", what, hipGetErrorString(e));
  }
  *out = m;
  return QK_OK;
}

extern "C" int qk_mps_set_centre(const qk_mps_set* m) { return m ? m->centre : -1; }

// ---- building from given states (qk_built_from_set) ---------------------------------------------------------------------------------
// A set becomes a qk_built with ONE snapshot of zero gates; every build entry resumes from it through initial, initial_snapshot.
// The heap holds each set state once; the per-state tables repeat by `index`, so one state may start many builds.
//   verbatim (the set records its centre, QK_SEED_SWEEP not set): qk_unpack_set_kernel copies the true-bond corners, bit for bit;
//   sweep (everything else): finite check, qk_compress_kernel with cap 0 and budget 0 (left-canonical, centre on the last site, bonds
//   shrunk to their ranks), then qk_seed_gather_kernel packs the batch's staging slots into the heap, polishes the isometries
//   and normalises the centre.
extern "C" int qk_built_from_set(qk_ctx* c, const qk_mps_set* set, int32_t n_states, const int32_t* index, double value_of_zero, uint32_t flags, qk_built** out, double* norms,
                                 double* fidelity) {
  static const char* what = "qk_built_from_set";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!set) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!out) return qk_fail(QK_EINVAL, "%s: out is null", what);
  *out = nullptr;
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; building from a set needs an fp64 set", what);
  if (n_states < 1) return qk_fail(QK_EINVAL, "%s: n_states must be >= 1, got %d", what, (int)n_states);
  if (!(value_of_zero >= 0.0) || !std::isfinite(value_of_zero)) return qk_fail(QK_EINVAL, "%s: value_of_zero must be >= 0 and finite (got %g)", what, value_of_zero);
  if (flags & ~(uint32_t)QK_SEED_SWEEP) return qk_fail(QK_EINVAL, "%s: unknown flags 0x%x (valid: QK_SEED_SWEEP)", what, (unsigned)flags);
  const int ns = set->n_states, n = set->n_sites, n1 = n + 1;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  if (!index && n_states != ns) return qk_fail(QK_EINVAL, "%s: without an index n_states must be the set's %d, got %d", what, ns, (int)n_states);
  for (int s = 0; index && s < n_states; ++s)
    if (index[s] < 0 || index[s] >= ns) return qk_fail(QK_EINVAL, "%s: index[%d] = %d outside the set's 0..%d", what, s, (int)index[s], ns - 1);
  const bool sweep = (flags & QK_SEED_SWEEP) || set->centre < 0;
  const int32_t* tru = set->dims_true.data();
  int qall = 1;
  for (size_t e = 0; e < (size_t)ns * n1; ++e) qall = std::max(qall, (int)tru[e]);
  if (sweep && qall > SPEC_QMAX) return qk_fail(QK_EINVAL, "%s: a bond of %d is beyond the %d the factorisation's LDS bookkeeping holds", what, qall, SPEC_QMAX);
  QkRangeGuard range_("qk:seed");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  std::vector<long long> need(ns, 0);  // complex elements of a state at its input bonds
  long long heap_elems = 0;
  for (int s = 0; s < ns; ++s) {
    for (int k = 0; k < n; ++k) need[s] += 2ll * tru[(size_t)s * n1 + k] * tru[(size_t)s * n1 + k + 1];
    heap_elems += need[s];
  }
  // what the set's states become: bond tables, offsets into the heap, fidelity, centre, norm
  std::vector<int32_t> sdims(set->dims_true), scentre(ns, sweep ? n - 1 : set->centre);
  std::vector<long long> soffs(ns, 0);
  std::vector<double> sfid(ns, 1.0), snorm(ns, 1.0);
  QkDevBuf heap;
  HIP_TRY_AS(what, heap.alloc((size_t)heap_elems * sizeof(cd)));  // no bond grows: the input sizes bound the heap
  long long top = 0;
  float ms = 0;
  int launch_grid = 0;
  if (!sweep) {
    std::vector<long long> dst((size_t)ns * n);
    for (int s = 0; s < ns; ++s) {
      soffs[s] = top;
      for (int k = 0; k < n; ++k) {
        dst[(size_t)s * n + k] = top;
        top += 2ll * tru[(size_t)s * n1 + k] * tru[(size_t)s * n1 + k + 1];
      }
    }
    QkDevBuf d_dst;
    HIP_TRY_AS(what, d_dst.alloc(dst.size() * sizeof(long long)));
    HIP_TRY_AS(what, hipMemcpyAsync(d_dst.get(), dst.data(), dst.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    qk_unpack_set_kernel<<<dim3((unsigned)(ns * n)), dim3(256), 0, c->stream>>>(set->d_data.get<double>(), set->d_offs.get<long long>(), d_dst.get<long long>(), set->d_true.get<int32_t>(),
                                                                              set->d_dims.get<int32_t>(), n, heap.get<cd>());
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  } else {
    // 1. the finite check: one flag per state, no factorisation is launched on a state that holds a NaN or an infinity
    {
      QkDevBuf d_flags;
      std::vector<int32_t> flg(ns, 0);
      HIP_TRY_AS(what, d_flags.alloc((size_t)ns * sizeof(int32_t)));
      HIP_TRY_AS(what, hipMemsetAsync(d_flags.get(), 0, (size_t)ns * sizeof(int32_t), c->stream));
      qk_seed_finite_kernel<<<dim3((unsigned)(ns * n)), dim3(256), 0, c->stream>>>(set->d_data.get<double>(), set->d_offs.get<long long>(), set->d_true.get<int32_t>(),
                                                                                 set->d_dims.get<int32_t>(), n, d_flags.get<int32_t>());
      HIP_TRY_AS(what, hipGetLastError());
      HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
      HIP_TRY_AS(what, hipMemcpy(flg.data(), d_flags.get(), (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int s = 0; s < ns; ++s)
        if (flg[s]) return qk_fail(QK_EDEVICE, "%s: state %d holds an element that is not finite", what, s);
    }
    // 2. the canonical sweep, in the batches of qk_mps_set_compress (the quarter-of-free-memory rule), 3. the gather of each batch
    size_t free_b = 0, total_b = 0;
    HIP_TRY_AS(what, hipMemGetInfo(&free_b, &total_b));
    const long long budget = (long long)(free_b / 4);
    std::vector<int> bstart{0};
    for (long long acc = 0, s = 0; s < ns; ++s) {
      const long long w = need[s] * (long long)sizeof(cd);
      if (acc > 0 && acc + w > budget / 2) bstart.push_back((int)s), acc = 0;
      acc += w;
    }
    bstart.push_back(ns);
    QkDevBuf d_new, d_fid, d_disc, d_err, d_so, d_ho, d_norm;
    const size_t n_disc = std::max<size_t>(1, (size_t)ns * (n - 1));
    HIP_TRY_AS(what, d_new.alloc((size_t)ns * n1 * sizeof(int32_t)));
    HIP_TRY_AS(what, d_fid.alloc((size_t)ns * sizeof(double)));
    HIP_TRY_AS(what, d_disc.alloc(n_disc * sizeof(double)));
    HIP_TRY_AS(what, d_err.alloc(32 * sizeof(int)));
    HIP_TRY_AS(what, d_so.alloc((size_t)ns * n * sizeof(long long)));
    HIP_TRY_AS(what, d_ho.alloc((size_t)ns * sizeof(long long)));
    HIP_TRY_AS(what, d_norm.alloc((size_t)ns * sizeof(double)));
    std::vector<long long> so((size_t)ns * n);
    HIP_TRY_AS(what, hipEventRecord(c->ev0, c->stream));
    for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
      const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
      long long stage_elems = 0;
      int qmax = 1;
      for (int s = s0; s < s0 + nb; ++s)
        for (int k = 0; k < n; ++k) {
          so[(size_t)s * n + k] = stage_elems;
          stage_elems += 2ll * tru[(size_t)s * n1 + k] * tru[(size_t)s * n1 + k + 1];
          qmax = std::max(qmax, (int)tru[(size_t)s * n1 + k]);
        }
      const size_t per_wg = qk_compress_work_bytes(qmax);
      const long long room = budget - stage_elems * (long long)sizeof(cd);
      const int grid = (int)std::max<long long>(1, std::min<long long>({(long long)nb, 2ll * c->num_cus, room / (long long)per_wg}));
      launch_grid = std::max(launch_grid, grid);
      QkDevBuf stage, work;
      HIP_TRY_AS(what, stage.alloc((size_t)stage_elems * sizeof(cd)));
      HIP_TRY_AS(what, work.alloc((size_t)grid * per_wg));
      HIP_TRY_AS(what, hipMemcpyAsync(d_so.get<long long>() + (size_t)s0 * n, so.data() + (size_t)s0 * n, (size_t)nb * n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
      QkCompressArgs a{};
      a.planes = set->d_data.get<double>(), a.pad = set->d_dims.get<int32_t>(), a.tru = set->d_true.get<int32_t>(), a.offs = set->d_offs.get<int64_t>();
      a.s0 = s0, a.n_batch = nb, a.n_sites = n;
      a.stage = stage.get<double>(), a.stage_offs = d_so.get<long long>() + (size_t)s0 * n;
      a.dims_new = d_new.get<int32_t>(), a.fidelity = d_fid.get<double>(), a.discarded = d_disc.get<double>();
      a.cap = 0, a.budget = 0.0, a.zero = value_of_zero;
      a.work = work.get<char>(), a.work_bytes = (long long)per_wg, a.qmax = qmax, a.error = d_err.get<int>();
      if (const int rc = qk_compress_launch(c, a, grid, what)) return rc;  // synchronises; a state of norm 0 is named there
      HIP_TRY_AS(what, hipMemcpy(sdims.data() + (size_t)s0 * n1, d_new.get<int32_t>() + (size_t)s0 * n1, (size_t)nb * n1 * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int s = s0; s < s0 + nb; ++s) {
        for (int k = 0; k <= n; ++k) {
          const int32_t x = sdims[(size_t)s * n1 + k];
          if (x < 1 || x > tru[(size_t)s * n1 + k]) return qk_fail(QK_EDEVICE, "%s: state %d came back with bond %d of %d (was %d)", what, s, k, (int)x, (int)tru[(size_t)s * n1 + k]);
        }
        soffs[s] = top;
        for (int k = 0; k < n; ++k) top += 2ll * sdims[(size_t)s * n1 + k] * sdims[(size_t)s * n1 + k + 1];
      }
      // the polish's scratch of a state: E (the largest bond squared) and one product (the largest site), at the new bonds
      std::vector<long long> po(nb);
      long long polish_elems = 0;
      for (int s = s0; s < s0 + nb; ++s) {
        long long r2 = 1, site = 1;
        for (int k = 0; k < n; ++k) {
          const long long l = sdims[(size_t)s * n1 + k], r = sdims[(size_t)s * n1 + k + 1];
          r2 = std::max(r2, r * r), site = std::max(site, 2 * l * r);
        }
        po[s - s0] = polish_elems;
        polish_elems += r2 + site;
      }
      QkDevBuf polish, d_po;
      HIP_TRY_AS(what, polish.alloc((size_t)polish_elems * sizeof(cd)));
      HIP_TRY_AS(what, d_po.alloc((size_t)nb * sizeof(long long)));
      HIP_TRY_AS(what, hipMemcpyAsync(d_po.get(), po.data(), (size_t)nb * sizeof(long long), hipMemcpyHostToDevice, c->stream));
      HIP_TRY_AS(what, hipMemcpyAsync(d_ho.get<long long>() + s0, soffs.data() + s0, (size_t)nb * sizeof(long long), hipMemcpyHostToDevice, c->stream));
      qk_seed_gather_kernel<<<dim3((unsigned)nb), dim3(256), 0, c->stream>>>(stage.get<cd>(), d_so.get<long long>() + (size_t)s0 * n, d_new.get<int32_t>(), d_ho.get<long long>(), s0, n,
                                                                           heap.get<cd>(), d_norm.get<double>(), polish.get<cd>(), d_po.get<long long>());
      HIP_TRY_AS(what, hipGetLastError());
      HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the staging buffer and the workspaces go before the next batch
    }
    HIP_TRY_AS(what, hipEventRecord(c->ev1, c->stream));
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
    HIP_TRY_AS(what, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    HIP_TRY_AS(what, hipMemcpy(sfid.data(), d_fid.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY_AS(what, hipMemcpy(snorm.data(), d_norm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = 0; s < ns; ++s)
      if (!(snorm[s] > 0.0) || !std::isfinite(snorm[s])) return qk_fail(QK_EDEVICE, "%s: state %d has a norm of %g after the sweep: nothing to build from", what, s, snorm[s]);
  }
  std::unique_ptr<qk_built> b(new (std::nothrow) qk_built);
  if (!b) return qk_fail(QK_ENOMEM, "%s: out of memory", what);
  b->ctx = c, b->n_states = n_states, b->n_qubits = n;
  b->checkpoints.assign(1, 0);
  b->all_dims.resize((size_t)n_states * n1);
  b->all_fidelity.resize(n_states);
  b->all_offsets.resize(n_states);
  b->all_centre.resize(n_states);
  b->all_logw.assign(n_states, 0.0);
  for (int s = 0; s < n_states; ++s) {
    const int src = index ? index[s] : s;
    std::copy(sdims.begin() + (size_t)src * n1, sdims.begin() + (size_t)(src + 1) * n1, b->all_dims.begin() + (size_t)s * n1);
    b->all_fidelity[s] = sfid[src], b->all_offsets[s] = soffs[src], b->all_centre[s] = scentre[src];
  }
  b->dims = b->all_dims, b->fidelity = b->all_fidelity, b->offsets = b->all_offsets;
  b->secs.assign(n_states, 0.0);
  b->heap = std::move(heap);
  b->total = top;
  b->kernel_ms = ms;
  if (sweep) b->grid = launch_grid, b->threads = 256, b->slots = 2 * c->num_cus;
  if (norms) std::copy(snorm.begin(), snorm.end(), norms);
  if (fidelity) std::copy(sfid.begin(), sfid.end(), fidelity);
  *out = b.release();
  return QK_OK;
}

extern "C" int qk_built_destroy(qk_built* b) {
  if (!b) return QK_OK;
  delete b;
  return QK_OK;
}

extern "C" int qk_debug_jacobi_precond(qk_ctx* c, int32_t p, int32_t q, double* a_inout, double* v_out, double* sig_out, int32_t* ord_out, int32_t* stats_out) {
  if (!c || !a_inout || !v_out || !sig_out || !ord_out) return qk_fail(QK_EINVAL, "qk_debug_jacobi_precond: null argument");
  if (p < 1 || q < 16 || q > 1024 || p > 64 * qkb256::MGS_R) return qk_fail(QK_EINVAL, "qk_debug_jacobi_precond: bad shape %d x %d (16 <= q <= 1024, p <= %d)", p, q, 64 * qkb256::MGS_R);
  HIP_TRY(hipSetDevice(c->device));
  QkDevBuf dA, dV, dS, dL, dSig, dO, dE, dC;  // cd: A, V, S, L; double: Sig; int: O, E, C
  const size_t lrows = (size_t)(q + 31) / 32 * 32, qpad = (size_t)(q + 15) / 16 * 16;
  HIP_TRY(dA.alloc((size_t)p * q * sizeof(cd)));
  HIP_TRY(dV.alloc((size_t)q * q * sizeof(cd)));
  HIP_TRY(dS.alloc((size_t)p * q * sizeof(cd)));
  HIP_TRY(dL.alloc(lrows * qpad * sizeof(cd)));
  HIP_TRY(dSig.alloc((size_t)q * sizeof(double)));
  HIP_TRY(dO.alloc((size_t)q * sizeof(int)));
  HIP_TRY(dE.alloc(32 * sizeof(int)));
  HIP_TRY(dC.alloc((qpad / 8) * (qpad / 8) * sizeof(int)));
  HIP_TRY(hipMemset(dE.get(), 0, 32 * sizeof(int)));
  HIP_TRY(hipMemcpy(dA.get(), a_inout, (size_t)p * q * sizeof(cd), hipMemcpyHostToDevice));
  const size_t lds_head = (size_t)(((q * 12 + 15) / 16) * 2 + 2) * sizeof(double);
  const bool wide = std::getenv("QK_BUILD_WGS") && std::atoi(std::getenv("QK_BUILD_WGS")) <= 1;  // the 512-thread variant of the builder
  const size_t lds = (wide ? 152 : 72) * 1024;
  const int lds_elems = (int)((lds - lds_head) / sizeof(cd));
  const size_t need = lds_head + (size_t)(wide ? qkb512::NWV * qkb512::BLK_LDS : qkb256::NWV * qkb256::BLK_LDS) * sizeof(cd);
  if (need > lds) return qk_fail(QK_EINVAL, "qk_debug_jacobi_precond: q = %d needs %zu bytes of LDS", q, need);
  int* const chk = std::getenv("QK_BUILD_NO_SKIP") ? nullptr : dC.get<int>();
  if (wide) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb512::qk_jacobi_precond_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
    qkb512::qk_jacobi_precond_kernel<<<dim3(1), dim3(512), lds, c->stream>>>(dA.get<cd>(), p, q, dV.get<cd>(), dSig.get<double>(), dO.get<int>(), dE.get<int>(), dS.get<cd>(), dL.get<cd>(), lds_elems, chk);
  } else {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(qkb256::qk_jacobi_precond_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 76 * 1024));
    qkb256::qk_jacobi_precond_kernel<<<dim3(1), dim3(256), lds, c->stream>>>(dA.get<cd>(), p, q, dV.get<cd>(), dSig.get<double>(), dO.get<int>(), dE.get<int>(), dS.get<cd>(), dL.get<cd>(), lds_elems, chk);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(a_inout, dA.get(), (size_t)p * q * sizeof(cd), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(v_out, dV.get(), (size_t)q * q * sizeof(cd), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sig_out, dSig.get(), (size_t)q * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ord_out, dO.get(), (size_t)q * sizeof(int), hipMemcpyDeviceToHost));
  int errv[32] = {0};
  HIP_TRY(hipMemcpy(errv, dE.get(), sizeof errv, hipMemcpyDeviceToHost));
  if (stats_out) {  // [0] sweeps, then 100 MHz ticks (low words): [1] all, [2] sort + copy, [3] Gram-Schmidt, [4] sweeps, [5] V and W = A V
    stats_out[0] = errv[2];
    stats_out[1] = errv[14], stats_out[2] = errv[16], stats_out[3] = errv[18], stats_out[4] = errv[20], stats_out[5] = errv[22];
  }
  if (errv[0]) return qk_fail(QK_EDEVICE, "qk_debug_jacobi_precond: no convergence in %d sweeps", MAX_SWEEPS);
  return QK_OK;
}

extern "C" int qk_debug_jacobi(qk_ctx* c, int32_t p, int32_t q, double* a_inout, double* v_out, double* sig_out, int32_t* ord_out) {
  if (!c || !a_inout || !v_out || !sig_out || !ord_out) return qk_fail(QK_EINVAL, "qk_debug_jacobi: null argument");
  if (p < 1 || q < 1 || q > 2048) return qk_fail(QK_EINVAL, "qk_debug_jacobi: bad shape %d x %d", p, q);
  HIP_TRY(hipSetDevice(c->device));
  QkDevBuf dA, dV, dS, dO, dE;  // cd: A, V; double: S; int: O, E
  HIP_TRY(dA.alloc((size_t)p * q * sizeof(cd)));
  HIP_TRY(dV.alloc((size_t)q * q * sizeof(cd)));
  HIP_TRY(dS.alloc((size_t)q * sizeof(double)));
  HIP_TRY(dO.alloc((size_t)q * sizeof(int)));
  HIP_TRY(dE.alloc(32 * sizeof(int)));
  HIP_TRY(hipMemset(dE.get(), 0, 32 * sizeof(int)));
  HIP_TRY(hipMemcpy(dA.get(), a_inout, (size_t)p * q * sizeof(cd), hipMemcpyHostToDevice));
  qkb256::qk_jacobi_kernel<<<dim3(1), dim3(256), (size_t)q * (sizeof(double) + sizeof(int)) + 16, c->stream>>>(dA.get<cd>(), p, q, dV.get<cd>(), dS.get<double>(), dO.get<int>(), dE.get<int>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(a_inout, dA.get(), (size_t)p * q * sizeof(cd), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(v_out, dV.get(), (size_t)q * q * sizeof(cd), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sig_out, dS.get(), (size_t)q * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ord_out, dO.get(), (size_t)q * sizeof(int), hipMemcpyDeviceToHost));
  int err = 0;
  HIP_TRY(hipMemcpy(&err, dE.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (err) return qk_fail(QK_EDEVICE, "qk_debug_jacobi: no convergence in %d sweeps", MAX_SWEEPS);
  return QK_OK;
}
