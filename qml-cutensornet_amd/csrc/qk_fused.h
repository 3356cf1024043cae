// qk_fused.h -- the site-fused sweep (qk_sweep_fused_kernel): the shipped fp64 hot path for sets with a bond > 32.
//
// One overlap <x|y> (reference: MPS.vdot, gpu_backend/kernel_state_ansatz.py:380; KernelPkg.jl:106) is the chain
//     X_0 = 1,   T[a, p, b'] = sum_b X[b, a] B_k[b, p, b'],   X'[b', a'] = sum_{a, p} T[a, p, b'] conj(A_k[a, p, a'])
// The ring sweep (qk_ring.h) runs it as two GEMMs per site with X and T in an L2-resident scratch: 40 % of its fabric
// traffic is the T round trip and every GEMM starts with a write->read stall.  Here T never exists in memory:
//
//   * X lives in LDS (complex128 interleaved, [b][a] row-major = "k-major" for the next site) whenever it fits the
//     workgroup's X buffer (98.7 % of the sites and 88 % of the matrix work of the 60-qubit x 6-layer headline workload
//     at 8192 elements).  Where X' is built and which part of X stays in LDS through a step is ONE rule (qk_plan.h: qk_resident; the step
//     table carries its answer).  X sits at one end of the buffer and X' is built at the other end whenever that keeps panels of X alive:
//     when the two fit side by side every panel stays (X' zeroed while the previous site's result is consumed, one barrier between the
//     phases); when each fits but not both, only the panels of X that X' overlaps are copied to the global buffer, the units of those row
//     blocks run phase 1 in its global-X form and all the others in its LDS form -- a unit with row block ta reads only panel ta (the form
//     is chosen per unit, not per step); a step that is LDS-resident by its single round alone overwrites X from element 0 behind a
//     barrier.  The 12-wave shapes give the rule more elements than the segmentation counts on (QKF_RCAP_ONE against QKF_XCAP_ONE: the LDS
//     the CU has beyond the buffer and the launch's tables), so more steps are side by side at the same plan, masks and step table;
//   * the unit of work is an ITEM (ta, tb, p): one 16 x 16 tile T[ta, p, tb], dealt to the waves in rounds of consecutive indices.
//     The order of the indices (qk_unit_decode, qk_plan.h: p slowest, ta fastest) decides what the waves of a round share: a round
//     lies inside one p and covers a few column blocks tb with all their ta, so an A block (ta, p) is used by the tb of the round at
//     the same time and a B block (p, tb) by its ta.  With p fastest (the order of the DET forms and of the dual kernel) a round takes
//     ONE tb with all (ta, p): each A block has one user per round and comes back a whole round later, once per tb.  Operand blocks
//     asked for per round, summed over a step of 4 x 4 tiles at 8 waves: 24 against 40, of 16 distinct ones (tests/host_san/
//     units_main.cpp holds the model for every shape).  Measured on the small-site launch of the headline set: - 7 % (lab/NOTES_r05.md);
//     the same order in the dual kernel: + 2 %, so that kernel keeps p fastest.
//     Phase 1: the wave computes its tile (K = b) and KEEPS it in registers -- the C/D layout of v_mfma_f64_16x16x4_f64
//     (register r of lane (q, j) = C[q + 4r][j]) is the A-operand layout of a k-major operand with k-step r, so the
//     tile is fed straight back as the A operand of phase 2:
//         X'[tb rows, tn cols] += T^T conj(A_k[ta rows, p, tn cols])     for every column block tn of a',
//     added into LDS with ds_add_f64 (the sum over ta and p is taken by the LDS);
//   * site tensors are read straight from the set image into B-operand fragments: one 16-byte load per lane and k-step
//     (complex128 interleaved image, rows of 16 elements = 256 contiguous bytes), four k-steps in flight per wave.  The
//     stream never drains: the last group of a tile loads the first group of the wave's next tile, of its first
//     phase-2 group, or of its first tile of the NEXT site, across the barriers.  In the one-tile kernel rows of zero padding are not
//     fetched: the k-steps of a group at or above the true bond ask for the address of the last k-step below it (QkfStream: - 5 % on
//     the small-site launch; the dual kernel, where it measured nothing, loads whole groups).  No staging ring, no per-K-tile
//     barrier: a wave runs its items autonomously and the workgroup meets at two or three barriers per site.  The
//     fragments that several items share are re-read through the caches (which catch a fifth to a quarter of them: the rest comes
//     back over the fabric -- DESIGN.md, cache counters);
//   * K is walked in units of 4 up to the TRUE bond; the complex product is the 3M form of the ring kernel.  In phase 2 of the plain
//     forms the three partial products are not re-combined by vector additions: with S = Ar + Ai, k1 = sum ti S is formed first and the
//     chains of re = k1 + sum (tr - ti) Ar and im = k1 + sum (-tr - ti) Ai START on it (the C operand of their first matrix instruction),
//     so a column block ends in its ds_add_f64 with no v_add_f64 behind the matrix instructions and forms ONE operand sum per fragment
//     element (qkf_p2_onesum; lab/NOTES_r07.md, lab/NOTES_r10.md);
//   * sites whose X or X' is too large for the LDS run in STRIPS: X is read whole from a per-workgroup global buffer (A-operand
//     fragments loaded like the site tensors), X' is accumulated a block of b' rows at a time (as many as fit the LDS), items in
//     rounds of (waves x slots), and written to the other global buffer;
//   * the chain is walked in STEPS: the first and last k sites of both states come as edge blocks (one product each), a step in
//     between is one site or two neighbouring sites contracted into one tensor of physical dimension 4 (merged image of the set),
//     as the pair's segmentation mask says (qk_plan.h: qk_segment_chain, made once per plan by qk_segment_kernel); per-step control
//     is a 48-byte record, the step table of the pair, built by all threads at pair set-up (qkf_step_table);
//   * every step has an ORIENTATION, chosen with the segmentation: 0 = as written above ("B first"), 1 = the two states exchanged, the
//     same code working on W = X^H ("A first").  A step that is followed by one of the other orientation ends with a SWITCH: its phase 2
//     runs with the source operands of the matrix instructions exchanged and leaves X'^H (qkf_p2_switch; plain forms only).
// Two launch shapes (chosen per launch -- or per run of pairs of a split plan -- in qkgram.hip): one 12-wave workgroup per CU
// (three waves per SIMD at 168 VGPRs, two tiles per wave) with an 8192-element X buffer -- by default in its DUAL form
// (qk_sweep_fused_dual_kernel below: the two tiles of a wave share the rows of X and of A, so every A and X fragment feeds
// two tiles), with independent single tiles in this kernel (QK_FUSED_DUAL=0) -- or two 8-wave workgroups (128 VGPRs, one tile
// per wave) with 4608 elements each -- the second workgroup fills the first one's barriers and per-site set-up, which pays
// while most of the work sits in sites that fit the smaller buffer.  A wave issues in order, so its tails, set-up and load waits
// stall its own matrix stream: the more waves share a SIMD, the better the matrix pipe is fed (8 waves x 4 slots: 482 ms
// on the headline set, 12 x 2: 452 ms, 16 x 1: 455 ms with a few spilled registers).
// Both kernels come in a DET form (template parameter; QK_DETERMINISTIC=1): the contributions to a block of X' are then added in a fixed
// order (qkf_turn_add) and a Gram is bit-reproducible, at 1.03 x the time on the headline set.
// fp64 only: the f32 MFMA's C layout (C[4q + r][j]) is not an operand layout (the complex64 sweep stays on qk_ring.h).
#pragma once
#include "qk_device.h"
#include "qk_plan.h"  // the order of a step's units (qk_unit_decode)

#include <cstddef>
#include <type_traits>

// Wave priority: a wave that is NOT in a matrix block (tile tails with their adds and LDS atomics, item set-up, barriers)
// runs at raised priority, so that it gets the issue slots ahead of the other wave's matrix stream and is back at its own
// MFMAs sooner: 481.4 against 490.5 ms on the 60-qubit x 6-layer set, same box, twice (the opposite rule: 489.6).
#define QKF_PRIO_LO() __builtin_amdgcn_s_setprio(0)
#define QKF_PRIO_HI() __builtin_amdgcn_s_setprio(2)
typedef double v2d __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) v2d lds_v2d;
// X (b rows x a columns, LDS or the global buffers) is kept in PANELS of 16 columns: element (row, col) sits at
//     (col / 16) * (rows * 16) + row * 16 + col % 16
// so that everything a lane adds to its address inside the loops is a constant: a k-step of phase 1 (4 rows) is 64 elements, the four rows
// q + 4 r of a tile in phase 2 are 64 elements apart, the second tile of a pair (16 rows down) 256 -- immediate offsets of the LDS and
// global instructions instead of vector additions, which on gfx950 take time from the matrix pipe (lab/tools/mfma_rate.hip).  A row-major
// X (stride a) costs four additions per group of k-steps in phase 1 and eight per column block in phase 2.
static constexpr int QKF_XSTEP = 4 * TILE;        // elements between two k-steps of X (phase 1) and between the rows q + 4 r of a tile (phase 2)
static constexpr int QKF_XBLOCK = TILE * TILE;    // elements of a block of 16 rows of a panel

// Two shapes are shipped (qkgram.hip picks one per launch from the plan's work profile):
//   <12 waves, 2 slots, 8192-element X buffer, 3 waves per SIMD>: one workgroup per CU -- large bonds (more sites stay LDS-resident)
//   <8 waves, 1 slot, 4608-element X buffer, 4 waves per SIMD>: two workgroups per CU -- small / medium bonds (the second workgroup
//                                              fills the first one's barriers and per-site set-up)

// experiment switches (lab builds only: -DQKF_EXPERIMENT -D...; all default to the shipped code)
#ifndef QKF_LDS3M
#define QKF_LDS3M 0
#endif
#ifndef QKF_P2_PROBE
#define QKF_P2_PROBE 0
#endif
// ABLATION builds of the dual kernel (timing only, WRONG results; lab/tools/r04_run18.sh): bit 0 = no operand sums inside the matrix loops, bit 1 = no global
// loads inside them, bit 2 = no s_barrier in the step loop, bit 3 = no LDS reads of X inside the loops of phase 1; one-wave sweep (qk_sweep_wave2_kernel): bit 4 = no LDS-DMA, bit 5 = no LDS reads of the fragments, bit 6 = no additions behind a T tile; one-tile kernel (qk_sweep_fused_kernel): bits 0-3 as in the dual kernel (bits 7 and 8, the tail of a block of phase 2, went with that tail)
#ifndef QKF_ABL
#define QKF_ABL 0
#endif
#define QKF_STEP_BARRIER()                            \
  do {                                                \
    if (QKF_ABL & 4) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    else qk_lds_barrier();                            \
  } while (0)
#define QKF_SUM(a, b) ((QKF_ABL & 1) ? (a) : (a) + (b))
#define QKF_DIF(a, b) ((QKF_ABL & 1) ? (b) : (a) - (b))
// one complex k-step, 3M form: (ar + i ai) * (br + i s bi), s = +1 | -1 (CONJB)
template <bool CONJB>
__device__ __forceinline__ void qkf_kstep(v4d& p1, v4d& p2, v4d& p3, const double ar, const double ai, const double br, const double bi) {
  const double sa = QKF_SUM(ar, ai), sb = CONJB ? QKF_DIF(br, bi) : QKF_SUM(br, bi);
  p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, p1, 0, 0, 0);
  p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, p2, 0, 0, 0);
  p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, sb, p3, 0, 0, 0);
}

struct QkfTile {  // a 16 x 16 complex tile in the C/D register layout: 16 VGPRs
  v4d re, im;
};

// 16-byte fragment load from a wave-uniform base and a 32-bit lane offset (in elements): the addressing form
// global_load_dwordx4 v, v_off, s[base:base+1] -- one VGPR of address state per stream
__device__ __forceinline__ v2d qkf_ldg(const v2d* __restrict__ base, const unsigned off) {
  return *reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(base) + (size_t)(off * 16u));
}
// experiment builds (-DQKF_EXPERIMENT -DQKF_NT_A=1 / -DQKF_NT_B=1): the phase-2 (A) / phase-1 (B) fragment stream with non-temporal loads
#ifndef QKF_NT_A
#define QKF_NT_A 0
#endif
#ifndef QKF_NT_B
#define QKF_NT_B 0
#endif
__device__ __forceinline__ v2d qkf_ldg_nt(const v2d* __restrict__ base, const unsigned off) {
  return __builtin_nontemporal_load(reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(base) + (size_t)(off * 16u)));
}
__device__ __forceinline__ v2d qkf_ldg_a(const v2d* __restrict__ base, const unsigned off) { return QKF_NT_A ? qkf_ldg_nt(base, off) : qkf_ldg(base, off); }
__device__ __forceinline__ v2d qkf_ldg_b(const v2d* __restrict__ base, const unsigned off) { return QKF_NT_B ? qkf_ldg_nt(base, off) : qkf_ldg(base, off); }
__device__ __forceinline__ v2d qkf_ldx(const v2d* __restrict__ base, const unsigned off) { return qkf_ldg(base, off); }
__device__ __forceinline__ v2d qkf_ldx(const lds_v2d* base, const unsigned off) { return base[off]; }

// A fragment stream: k-step i of the current group is element base + off + i * step (base wave-uniform, off this lane's).
// No row of padding is fetched: of a group that holds the end of the true bond only `lim` k-steps are needed (the matrix instructions of the
// others are not issued), and the others are asked for at the address of the last one needed -- the same cache lines, so the request ends in
// the L1 and costs no byte over the fabric (a bond of 84 is padded to 96 rows: an eighth of both streams).  The four addresses of a group are
// wave-uniform bases (qkf_kbase: scalar min / multiply / add where a stream starts or changes), the lane offset is shared, so the matrix
// blocks hold the same vector instructions as with unconditional loads.  `lim` of a stream is that of its FIRST group: min(4, k-steps of b)
// for a B stream, the k-steps below the true bond of its block of rows for an A stream (whose groups all cover the same rows).  The
// streams of the dual kernel leave it at 4: they load whole groups (rows up to the padded bond exist and are zero).  X from the global
// buffer (strip path) is loaded whole as well: its four k-steps are immediate offsets of ONE vector address, and an address per k-step
// would cost the steady block a vector instruction each.
struct QkfStream {
  const v2d* base;
  unsigned off;
  int step;
  int lim = 4;
};
__device__ __forceinline__ const v2d* qkf_kbase(const v2d* const base, const int step, const int i, const int lim) { return base + max(min(i, lim - 1), 0) * step; }
__device__ __forceinline__ void qkf_load4(v2d (&fr)[4], const QkfStream& st) {
#pragma unroll
  for (int i = 0; i < 4; ++i) fr[i] = qkf_ldg(qkf_kbase(st.base, st.step, i, st.lim), st.off);
}
// ... with the lane offset in BYTES (phase 1 keeps its two running offsets in the unit the instructions take: one addition per group each)
__device__ __forceinline__ v2d qkf_ldgb(const v2d* __restrict__ base, const unsigned boff) {
  const v2d* const at = reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(base) + (size_t)boff);
  return QKF_NT_B ? __builtin_nontemporal_load(at) : *at;  // (the phase-1 B stream: the QKF_NT_B experiment applies)
}
// this lane's running position in the X operand of phase 1: an LDS address, or a byte offset on the (wave-uniform) global buffer -- one
// addition per group of k-steps either way, the four k-steps of a group are immediate offsets
struct QkfXLds {
  const lds_v2d* p;
  __device__ __forceinline__ void advance() { p += 4 * QKF_XSTEP; }
  __device__ __forceinline__ v2d kstep(const int i) const { return p[i * QKF_XSTEP]; }
};
struct QkfXGlobal {
  const v2d* base;
  unsigned bo;
  __device__ __forceinline__ void advance() { bo += 4 * QKF_XSTEP * 16u; }
  __device__ __forceinline__ v2d kstep(const int i) const { return *reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(base + i * QKF_XSTEP) + (size_t)bo); }
};
__device__ __forceinline__ QkfXLds qkf_xcursor(const lds_v2d* xp, const unsigned xoff) { return QkfXLds{xp + xoff}; }
__device__ __forceinline__ QkfXGlobal qkf_xcursor(const v2d* xp, const unsigned xoff) { return QkfXGlobal{xp, xoff * 16u}; }

// Phase 1, one tile (= one item): T[ta, p, tb] = sum_{l < 4 nks} X[l][16 ta + .] * B[l][p][16 tb + .].
//   B operand: stream `cur` (step = one k-step = 4 rows of b); its first group is already in `fr` when `primed`;
//   A operand: X element (xp + xoff + 64 i) of the panel of columns 16 ta .. (k-step i: rows 4 i + q), X in LDS or in the global buffer.
// Four k-steps of fragments are in flight: the registers of a k-step are reloaded for k-step + 4 right after its
// MFMAs (sched_barrier keeps that order); in the LAST group they are reloaded with the first group of stream `nxt`
// -- the wave's next tile, or its first phase-2 group -- so the stream never drains between tiles or across the
// barriers.  MFMAs are issued only for the k-steps below the true bond, and the rows of padding above it are not
// fetched: the group that holds the end of the bond (`last` k-steps) is loaded from bases of its own (QkfStream), which
// the steady loop takes over for its final trip -- the loop runs in two passes over ONE body, the bases change between them.
template <typename XPtr>
__device__ __forceinline__ void qkf_p1_tile(QkfTile& t, v2d (&fr)[4], const bool primed, QkfStream cur, XPtr xp, unsigned xoff, const int nks, const QkfStream nxt) {
  v4d p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0};
  v2d fx[4];
  const int ng = (nks + 3) >> 2, last = nks - 4 * (ng - 1);  // k-steps of the last group: 1..4
  if (!primed) qkf_load4(fr, cur);
#pragma unroll
  for (int i = 0; i < 4; ++i) fx[i] = qkf_ldx(xp + i * QKF_XSTEP, xoff);
  // the bases the NEXT group is loaded from: whole groups, but the last group only up to the bond
  const v2d* cb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) cb[i] = qkf_kbase(cur.base, cur.step, i, ng == 2 ? last : 4);
  unsigned bo = cur.off * 16u;  // this lane's byte offset into the B stream, and its X address: the two running values of the loops
  const unsigned bs = (unsigned)(4 * cur.step) * 16u;
  auto xq = qkf_xcursor(xp, xoff);
  QKF_PRIO_LO();
  int gq = 0;
  // the first k-step of a chain of more than four k-steps STARTS the accumulators (literal zero as the C operand): no register moves to zero
  // them -- on gfx950 every vector instruction takes time from the matrix pipe (lab/tools/mfma_rate.hip)
  if (ng >= 2) {
    gq = 1;
    bo += bs, xq.advance();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i == 0) {
        const v4d z = {0, 0, 0, 0};
        p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(fx[0].x, fr[0].x, z, 0, 0, 0);
        p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fx[0].y, fr[0].y, z, 0, 0, 0);
        p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(QKF_SUM(fx[0].x, fx[0].y), QKF_SUM(fr[0].x, fr[0].y), z, 0, 0, 0);
      } else {
        qkf_kstep<false>(p1, p2, p3, fx[i].x, fx[i].y, fr[i].x, fr[i].y);
      }
      if (!(QKF_ABL & 2)) fr[i] = qkf_ldgb(cb[i], bo);
      if (!(QKF_ABL & 8)) fx[i] = xq.kstep(i);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // pass 0: the groups that are followed by a whole group; pass 1: the one trip that loads the last group, from its own bases
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int end = ng - 2 + pass;
#pragma unroll 1
    for (; gq < end; ++gq) {
      bo += bs, xq.advance();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        qkf_kstep<false>(p1, p2, p3, fx[i].x, fx[i].y, fr[i].x, fr[i].y);
        if (!(QKF_ABL & 2)) fr[i] = qkf_ldgb(cb[i], bo);
        if (!(QKF_ABL & 8)) fx[i] = xq.kstep(i);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cb[i] = qkf_kbase(cur.base, cur.step, i, last);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < last) qkf_kstep<false>(p1, p2, p3, fx[i].x, fx[i].y, fr[i].x, fr[i].y);
    if (!(QKF_ABL & 2)) fr[i] = qkf_ldg(qkf_kbase(nxt.base, nxt.step, i, nxt.lim), nxt.off);
    __builtin_amdgcn_sched_barrier(0);
  }
  QKF_PRIO_HI();
  t.re = p1 - p2;
  t.im = p3 - p1 - p2;
}

// ORDERED accumulation (the DET forms of the kernels: bit-reproducible sweeps).  The contributions to one 16 x 16 block of X' -- one per
// (ta, p) -- are added in the order of their index i = pd ta + p instead of in arrival order: the block has a turn counter in LDS, the
// contribution of index 0 STORES (so X' needs no zeroing pass, and an LDS-resident site with X and X' side by side needs no barrier between
// its phases), index i waits until the counter reads i, adds and passes the turn on.  Waits always go to a lower index, and a wave takes
// its units in increasing order, so the chain cannot lock; waves that keep pace wait a few cycles per block (the LDS unit serialises adds
// to one block anyway).  The counters of a step are zeroed during the step before (two sets, alternating).
typedef __attribute__((address_space(3))) int lds_int;
struct QkfTurn {
  lds_int* at;                 // the turn counters of this contribution's block of rows, one per column block tn
  int idx;                     // its place in the order
  lds_int* broken;             // sticky flag of the workgroup: a wait ran out (a bug, never seen) -- every later wait is skipped, the launch ends
  unsigned long long* gerr;    // ... and is reported through this word (qk_get_stats fails the call)
};
__device__ __forceinline__ void qkf_turn_add(__attribute__((address_space(3))) double* const d, const long rs, const v4d& re, const v4d& im, const QkfTurn& t, const int tn) {
  lds_int* const turn = t.at + tn;
  if (t.idx > 0) {
    int spins = 0;
#ifdef QKF_FIRST_STORE  // experiment: only the FIRST contribution is ordered (it stores: no zeroing, no barrier between the phases); the others add in arrival order
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0) {
#else
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != t.idx) {
#endif
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 20) || __builtin_amdgcn_readfirstlane(__hip_atomic_load(t.broken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 0) {  // never a hung GPU
        __hip_atomic_store(t.broken, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (t.gerr) *t.gerr = 1ull;
        break;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      __hip_atomic_fetch_add(d + r * rs, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(d + r * rs + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) *(lds_v2d*)(d + r * rs) = (v2d){re[r], im[r]};
  }
#ifdef QKF_FIRST_STORE
  if (t.idx > 0) return;
#endif
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's adds have left the LDS queue before the turn moves on
  __hip_atomic_store(turn, t.idx + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- Phase 2 of the plain forms: ONE column block for both kinds of step, one operand sum per fragment element (lab/NOTES_r10.md).
// With S = Ar + Ai the products are
//     ordinary (X' += T^T conj(A)):   k1 = sum ti S,   re = k1 + sum (tr - ti) Ar,   im = k1 + sum (-tr - ti) Ai
//     switch   (X'^H = conj(T)^T A):  k1 = sum S tr,   re = k1 + sum Ai (ti - tr),   im = k1 + sum Ar (-tr - ti)
// (tests/host_san/onesum_main.cpp), so the chains of re and im run on the RAW parts of the fragment and a column block forms one sum
// per fragment element and k-step -- 4 v_add_f64 -- where the first tuned form (qkf_p2_block) has 8 and the simple switch loop
// (qkf_p2_switch_simple) 4 and 16 additions behind its matrix instructions.  Everything else rides on the T side: three register sets per
// tile as before, QkfTSet: k (feeds k1), a (feeds re), b (feeds im), taken once per unit (qkf_tset) from the tile phase 1 left.  The two
// kinds of step differ only in which part of T is in which set, in which raw part of the fragment a chain reads, and in the order of the
// two source operands of every matrix instruction (SWITCH: the fragment is the A operand and the accumulators hold the tile of X'^T --
// the A and the B operand of v_mfma_f64_16x16x4_f64 have the same lane layout).
// As in the first tuned form k1 of the block's k-steps is formed first (k-step 0 starts the chain on the literal zero; the sum of k-step
// i + 1 is taken while the matrix instruction of k-step i runs) and the chains of re and im START on it: the first matrix instruction of
// `re` reads k1 as its C operand and writes other registers, `im` goes on in k1's, and the block ends in its ds_add_f64 with no addition
// behind the matrix instructions.
// The reload: the chains read the raw fragment, so the registers of a k-step cannot be reloaded behind its k1 as in the first tuned form.
// fr[i] is reloaded LATE, behind the last chain instruction that reads it (in a pair of tiles: the second tile's): one set, one block
// body, 6 - 12 matrix instructions between a load and its first use instead of a whole block -- the other waves of the SIMD cover it:
// cfg4, one box, parent against this form twice each: dual launch 277.7 / 278.3 -> 273.3 / 273.3 ms, 8-wave launch 46.93 / 46.94 ->
// 46.29 / 46.27 ms.  (A ping-pong form -- the next block's loads into a second set behind k1_i, a whole block ahead -- needed eight
// registers more than the dual kernel has and lost 11 ms: lab/dropped/r10_p2_pingpong.patch.)
// QKF_P2_FORM_* = 1 selects this block per launch shape (the shipped setting for all three); 0 keeps the first tuned form (qkf_p2_block /
// the plain loop of qkf_p2_item) and the simple switch loop, for A/B builds.
#ifndef QKF_P2_FORM_DUAL  // the 12-wave dual kernel
#define QKF_P2_FORM_DUAL 1
#endif
#ifndef QKF_P2_FORM_ONE   // the 12-wave one-tile kernel (two slots, 168 registers)
#define QKF_P2_FORM_ONE 1
#endif
#ifndef QKF_P2_FORM_TWO   // the 8-wave one-tile kernel (128 registers)
#define QKF_P2_FORM_TWO 1
#endif
typedef __attribute__((address_space(3))) double lds_double;
struct QkfTSet {
  v4d k, a, b;
};
template <bool SWITCH>
__device__ __forceinline__ QkfTSet qkf_tset(const QkfTile& t) {
  return SWITCH ? QkfTSet{t.re, t.im - t.re, -t.re - t.im} : QkfTSet{t.im, t.re - t.im, -t.re - t.im};
}
// one matrix instruction of the block: the T-side value first, the fragment's second; SWITCH exchanges them
template <bool SWITCH>
__device__ __forceinline__ v4d qkf_p2_mma(const double t, const double f, const v4d& c) {
  return SWITCH ? __builtin_amdgcn_mfma_f64_16x16x4f64(f, t, c, 0, 0, 0) : __builtin_amdgcn_mfma_f64_16x16x4f64(t, f, c, 0, 0, 0);
}
// (Late reload: a matrix builtin carries no order against a load, and the compiler, left alone, issues the reload of a k-step ahead of the chain
// instructions that still read it and pays with eight register copies per block.  So the chains' results pass through an empty statement
// -- no instruction -- that the load cannot cross.)
#define QKF_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b) : : "memory")
// One column block: the chains on the fragment in `fa`, whose k-step i is reloaded from (b_i, off) behind its last reader; then the results
// are added to X' at d (and d1 for the second tile), the rows q + 4 r of a tile 2 QKF_XSTEP doubles apart.
template <bool FULL, bool HAS1, bool SWITCH>
__device__ __forceinline__ void qkf_p2_onesum(const QkfTSet& u0, const QkfTSet& u1, v2d (&fa)[4], const int kmax, const v2d* const b0, const v2d* const b1, const v2d* const b2,
                                              const v2d* const b3, const unsigned off, lds_double* const d, lds_double* const d1) {
  constexpr long rs = 2 * QKF_XSTEP;
  const v4d z = {0, 0, 0, 0};
  v4d p1 = z, r1 = z, re, im, re1, im1;
  QKF_PRIO_LO();
  double s = QKF_SUM(fa[0].x, fa[0].y);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (FULL || i == 0 || i < kmax) {
      p1 = qkf_p2_mma<SWITCH>(u0.k[i], s, i == 0 ? z : p1);
      if (HAS1) r1 = qkf_p2_mma<SWITCH>(u1.k[i], s, i == 0 ? z : r1);
    }
    if (i < 3) s = QKF_SUM(fa[i + 1].x, fa[i + 1].y);  // (a k-step at or above the bond: loaded from the last one's address, the sum is not used)
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (FULL || i == 0 || i < kmax) {
      const double fre = SWITCH ? fa[i].y : fa[i].x, fim = SWITCH ? fa[i].x : fa[i].y;  // the raw part the chain of re / of im reads
      re = qkf_p2_mma<SWITCH>(u0.a[i], fre, i == 0 ? p1 : re);
      im = qkf_p2_mma<SWITCH>(u0.b[i], fim, i == 0 ? p1 : im);
    }
    if (!HAS1 && !(QKF_ABL & 2)) {
      QKF_PIN2(re, im);
      fa[i] = qkf_ldg_a(i == 0 ? b0 : i == 1 ? b1 : i == 2 ? b2 : b3, off);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (HAS1) {  // the second tile's chains stand behind the first tile's (whose ds_add_f64 then run beside them); they are the last to read fr[i]
    QKF_PIN2(re, im);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (FULL || i == 0 || i < kmax) {
        const double fre = SWITCH ? fa[i].y : fa[i].x, fim = SWITCH ? fa[i].x : fa[i].y;
        re1 = qkf_p2_mma<SWITCH>(u1.a[i], fre, i == 0 ? r1 : re1);
        im1 = qkf_p2_mma<SWITCH>(u1.b[i], fim, i == 0 ? r1 : im1);
      }
      if (!(QKF_ABL & 2)) {
        QKF_PIN2(re1, im1);
        fa[i] = qkf_ldg_a(i == 0 ? b0 : i == 1 ? b1 : i == 2 ? b2 : b3, off);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  QKF_PRIO_HI();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    __hip_atomic_fetch_add(d + r * rs, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(d + r * rs + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (HAS1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      __hip_atomic_fetch_add(d1 + r * rs, re1[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(d1 + r * rs + 1, im1[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}
// The column blocks of a unit: `fr` holds the first group of stream `cur` (k-steps of it below `lim` are fetched, qkf_kbase) and leaves
// with the first group of `nxt`; block tn adds to d + tn * dstep, the second tile of a pair d1off further on (a constant in the ordinary
// step: an immediate offset).  The bases of a stream are wave-uniform and do not change, so the loop runs over the blocks that are
// followed by another block of the stream, and the last block, which reloads from `nxt`, stands behind it.
template <bool FULL, bool HAS1, bool SWITCH>
__device__ __forceinline__ void qkf_p2_blocks(const QkfTile& t0, const QkfTile& t1, v2d (&fr)[4], const QkfStream cur, const int lim, const QkfStream nxt, const int nn, const int kmax,
                                              lds_double* d, const int d1off, const int dstep) {
  const QkfTSet u0 = qkf_tset<SWITCH>(t0), u1 = HAS1 ? qkf_tset<SWITCH>(t1) : u0;
  const v2d *const c0 = qkf_kbase(cur.base, cur.step, 0, lim), *const c1 = qkf_kbase(cur.base, cur.step, 1, lim), *const c2 = qkf_kbase(cur.base, cur.step, 2, lim),
            *const c3 = qkf_kbase(cur.base, cur.step, 3, lim);
  unsigned off = cur.off;
#pragma unroll 1
  for (int tn = 0; tn + 1 < nn; ++tn) {
    off += TILE;
    qkf_p2_onesum<FULL, HAS1, SWITCH>(u0, u1, fr, kmax, c0, c1, c2, c3, off, d, d + d1off);
    d += dstep;
  }
  qkf_p2_onesum<FULL, HAS1, SWITCH>(u0, u1, fr, kmax, qkf_kbase(nxt.base, nxt.step, 0, nxt.lim), qkf_kbase(nxt.base, nxt.step, 1, nxt.lim), qkf_kbase(nxt.base, nxt.step, 2, nxt.lim),
                                    qkf_kbase(nxt.base, nxt.step, 3, nxt.lim), nxt.off, d, d + d1off);
}

// Phase 2, one item: X'[tb rows, tn cols] += T^T conj(A[16 ta + ., p, 16 tn + .]) for every column block tn, added into
// the LDS image `xo` (row stride a2, this item's 16 rows start at xo) with ds_add_f64.  A operand: stream `cur` (group
// = column block tn: off advances by 16 per group; step = one k-step = 4 rows of a).  FULL: all four k-steps of this ta
// block lie below the true bond (every block but the last one of a ragged bond); otherwise kmax of them do.  The last
// group reloads the registers with the first group of `nxt` (the wave's next item, or its first tile of the next site).
// The plain form is the single-tile instantiation of the one-sum block (FORM 1, shipped), or the first tuned form's loop (FORM 0); the
// ordered form (DET) keeps the product's first 3M form, its additions and its bits.
template <bool FULL, bool DET = false, int FORM = 0>
__device__ __forceinline__ void qkf_p2_item(const QkfTile& t, v2d (&fr)[4], const bool primed, QkfStream cur, const int ps, const int nn, const int kmax, lds_v2d* xo, const int q,
                                            const int j, const QkfStream nxt, const QkfTurn turn = QkfTurn{nullptr, 0, nullptr, nullptr}) {
  if (!primed) qkf_load4(fr, cur);
  __attribute__((address_space(3))) double* d = (__attribute__((address_space(3))) double*)(xo + q * TILE + j);
  if constexpr (!DET && FORM != 0) {  // the one-sum block (above), single tile
    qkf_p2_blocks<FULL, false, false>(t, t, fr, cur, FULL ? 4 : kmax, nxt, nn, kmax, d, 0, 2 * ps);
    return;
  }
  if constexpr (!DET) {
    // (FORM 0, A/B builds: the first tuned form)  k1 = sum (tr + ti) Ar first, then the chains of re = k1 + sum ti (Ai - Ar) and im = k1 - sum tr (Ar + Ai) START on it
    // (qkf_p2_block has the reasoning): 8 v_add_f64 per column block -- the operand sums, formed while k1 runs so that the registers of a
    // k-step are reloaded right behind its k1 -- instead of 17; the sums tr + ti are taken once per item (the register allocator of the
    // 128-register shape keeps seven of the eight registers and forms the last sum again per block: 9 per block there).
    const v4d z = {0, 0, 0, 0};
    const v4d s = t.re + t.im;
#pragma unroll 1
    for (int tn = 0; tn < nn; ++tn) {
      v4d p1 = z, re, im;
      double sp[4], sm[4];
      const bool fin = tn + 1 == nn;
      const v2d* const rb = fin ? nxt.base : cur.base;
      const int rs = fin ? nxt.step : cur.step, rl = fin ? nxt.lim : FULL ? 4 : kmax;  // (the k-steps at or above the bond: the address of the last one below it)
      cur.off = fin ? nxt.off : cur.off + TILE;
      QKF_PRIO_LO();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (FULL || i == 0 || i < kmax) {
          p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(s[i], fr[i].x, i == 0 ? z : p1, 0, 0, 0);
          sp[i] = QKF_DIF(-fr[i].x, fr[i].y), sm[i] = QKF_DIF(fr[i].y, fr[i].x);
        }
        if (!(QKF_ABL & 2)) fr[i] = qkf_ldg_a(qkf_kbase(rb, rs, i, rl), cur.off);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (FULL || i == 0 || i < kmax) {
          re = __builtin_amdgcn_mfma_f64_16x16x4f64(t.im[i], sm[i], i == 0 ? p1 : re, 0, 0, 0);
          im = __builtin_amdgcn_mfma_f64_16x16x4f64(t.re[i], sp[i], i == 0 ? p1 : im, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      QKF_PRIO_HI();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        __hip_atomic_fetch_add(d + r * 2 * QKF_XSTEP, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(d + r * 2 * QKF_XSTEP + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      d += 2 * ps;  // the next panel
    }
    return;
  }
  // the ordered form keeps the product's first 3M form and its additions: deterministic Grams keep their bits
#pragma unroll 1
  for (int tn = 0; tn < nn; ++tn) {
    v4d p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0};
    const bool fin = tn + 1 == nn;
    const v2d* const rb = fin ? nxt.base : cur.base;
    const int rs = fin ? nxt.step : cur.step, rl = fin ? nxt.lim : FULL ? 4 : kmax;  // (the k-steps at or above the bond: the address of the last one below it)
    cur.off = fin ? nxt.off : cur.off + TILE;
    QKF_PRIO_LO();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (FULL || i < kmax) qkf_kstep<true>(p1, p2, p3, t.re[i], t.im[i], fr[i].x, fr[i].y);
      if (!(QKF_ABL & 2)) fr[i] = qkf_ldg_a(qkf_kbase(rb, rs, i, rl), cur.off);
      __builtin_amdgcn_sched_barrier(0);
    }
    QKF_PRIO_HI();
    const v4d re = p1 + p2, im = p3 - p1 + p2;
    qkf_turn_add(d, (long)2 * QKF_XSTEP, re, im, turn, tn);
    d += 2 * ps;  // the next panel
  }
}

// Phase 2 of a SWITCH step (qk_plan.h: the association of a step): the chain goes on in the other orientation, so the step leaves
// X'^H instead of X'.  On v_mfma_f64_16x16x4_f64 the A and the B operand have the same lane layout (lane (q, j) holds [k = q][m or n = j]),
// so the two source operands of every matrix instruction are EXCHANGED -- the fragment of A_k is the A operand, the T tile the B operand --
// and the accumulators hold the tile [a' of block tn][b' of block tb] of X'^T in the usual C layout.  It goes to block (tn, tb) of the
// output in the other orientation's panels (16 columns of b', a2 rows: the caller's `d` points at block tb's panel, a block of rows tn is
// QKF_XBLOCK elements further on, the second tile of a pair `d1off` doubles = one panel) with the ordinary in-tile lane pattern.  The
// conjugation moves from A to T and rides on the per-tile sums of T:  X'^H = conj(T)^T A,
//     k1 = sum tr (Ar + Ai),   re = k1 + sum (ti - tr) Ai,   im = k1 + sum (-tr - ti) Ar
// -- one operand sum per fragment element, the registers of T's imaginary part and of tr + ti become ti - tr and -tr - ti.  The shipped
// form is the SWITCH instantiation of the one-sum block (qkf_p2_onesum above: chains started on k1, a specialisation for full blocks, the
// reload of the kernel's form); `lim` as in qkf_p2_item (4 in the dual kernel, whose streams load whole groups).  It hands fr to the next
// unit exactly as the ordinary blocks do.  On the headline set a fifth of the steps take it.
// FORM 0 is the simple loop round 9 shipped (kept for the A/B): that of the ordered forms -- three chains per tile and k-step, the registers
// of a k-step reloaded behind them, the sums k1 + . taken behind the block, no specialisation for full blocks.
template <bool HAS1>
__device__ __forceinline__ void qkf_p2_switch_simple(const QkfTile& t0, const QkfTile& t1, v2d (&fr)[4], QkfStream cur, const int lim, const int nn, const int kmax,
                                                     __attribute__((address_space(3))) double* d, const int d1off, const QkfStream nxt) {
  const v4d dm0 = t0.im - t0.re, ng0 = -t0.re - t0.im, dm1 = HAS1 ? t1.im - t1.re : dm0, ng1 = HAS1 ? -t1.re - t1.im : ng0;
#pragma unroll 1
  for (int tn = 0; tn < nn; ++tn) {
    v4d p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0}, r2 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
    const bool fin = tn + 1 == nn;
    const v2d* const rb = fin ? nxt.base : cur.base;
    const int rs = fin ? nxt.step : cur.step, rl = fin ? nxt.lim : lim;
    cur.off = fin ? nxt.off : cur.off + TILE;
    QKF_PRIO_LO();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < kmax) {
        const double sa = QKF_SUM(fr[i].x, fr[i].y);
        p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, t0.re[i], p1, 0, 0, 0);
        p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[i].y, dm0[i], p2, 0, 0, 0);
        p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[i].x, ng0[i], p3, 0, 0, 0);
        if (HAS1) {
          r1 = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, t1.re[i], r1, 0, 0, 0);
          r2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[i].y, dm1[i], r2, 0, 0, 0);
          r3 = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[i].x, ng1[i], r3, 0, 0, 0);
        }
      }
      fr[i] = qkf_ldg_a(qkf_kbase(rb, rs, i, rl), cur.off);
      __builtin_amdgcn_sched_barrier(0);
    }
    QKF_PRIO_HI();
    {
      const v4d re = p1 + p2, im = p1 + p3;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        __hip_atomic_fetch_add(d + r * 2 * QKF_XSTEP, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(d + r * 2 * QKF_XSTEP + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    if (HAS1) {
      const v4d re = r1 + r2, im = r1 + r3;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        __hip_atomic_fetch_add(d + d1off + r * 2 * QKF_XSTEP, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(d + d1off + r * 2 * QKF_XSTEP + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    d += 2 * QKF_XBLOCK;  // the next block of rows of a'
  }
}
template <bool FULL, bool HAS1, int FORM>
__device__ __forceinline__ void qkf_p2_switch(const QkfTile& t0, const QkfTile& t1, v2d (&fr)[4], const bool primed, const QkfStream cur, const int lim, const int nn, const int kmax,
                                              lds_double* const d, const int d1off, const QkfStream nxt) {
  if (!primed) qkf_load4(fr, cur);
  if constexpr (FORM == 0) qkf_p2_switch_simple<HAS1>(t0, t1, fr, cur, lim, nn, kmax, d, d1off, nxt);
  else qkf_p2_blocks<FULL, HAS1, true>(t0, t1, fr, cur, lim, nxt, nn, kmax, d, d1off, 2 * QKF_XBLOCK);  // (tn: the next block of rows of a')
}

// The T tiles of a wave live in registers, S slots.  The slot loops are NOT unrolled (unrolled, every slot drags ~50
// VGPRs of hoisted address state through the whole sweep) and the working slot is always T[S-1]: when a round gives
// the waves up to L > 1 items each, the last L slots are turned by one before each item (phase 1 makes all L turns, so
// that item s ends in slot S-L+s; phase 2 turns once per item, which brings item s to slot S-1).  S <= 4.
template <int S>
__device__ __forceinline__ void qkf_rotate(QkfTile (&T)[S], const int L) {  // turn the last L <= S slots by one: T[S-L] goes to T[S-1]
  if constexpr (S >= 2) {
    if (L == 2) {
      const QkfTile t = T[S - 2];
      T[S - 2] = T[S - 1], T[S - 1] = t;
    }
  }
  if constexpr (S >= 3) {
    if (L == 3) {
      const QkfTile t = T[S - 3];
      T[S - 3] = T[S - 2], T[S - 2] = T[S - 1], T[S - 1] = t;
    }
  }
  if constexpr (S >= 4) {
    if (L >= 4) {
      const QkfTile t0 = T[0];
#pragma unroll
      for (int e = 0; e + 1 < S; ++e) T[e] = T[e + 1];
      T[S - 1] = t0;
    }
  }
}

// ----------------------------------------------------------------------------------------
// Edge blocks (SweepArgs.edge_k): the contraction order chosen on the host for the ENDS of the chain.  While the bonds still grow
// like 2^k, contracting the first k sites of each state into one matrix L[s][a] and taking X = Ly^T conj(Lx) -- one product with
// K = 2^k -- is cheaper than k sites of the chain, and it saves their per-site costs (two barriers, set-up, load latencies: 3-5 us
// each, as much as the matrix work of a 64 x 64 site); likewise at the right end, where the overlap is sum_{b,a} X[b][a] R[b][a]
// with R = Ry^T conj(Rx).  On the 60-qubit x 6-layer set the model picks k = 8: 16 of 60 sites go.
// ----------------------------------------------------------------------------------------
// An edge product is streamed like the site loops (qkf_edge_unit): the two blocks are addressed from WAVE-UNIFORM bases, one per k-step of a
// trip, and a lane byte offset that advances once per trip -- no address arithmetic inside a k-step (the earlier form built
// (long)(4 * k-step) * ld per k-step in 64-bit vector arithmetic) --, and SETS register sets of one group (four k-steps) each are in flight:
// the registers of a k-step are reloaded for k-step + 4 SETS right behind its matrix instructions.  Measured per launch of the 60-qubit x
// 6-layer Gram, parent's library against builds of this code alternating in one call (lab/NOTES_r06.md, profiles/r06/):
//   12-wave dual launch, 298.4 ms (the two forms below with the dual kernel's pull-ahead loop; single tiles with the parent's loop: 292.2):
//                                   single tiles, two sets (8 k-steps in flight)  288.2   <- shipped in the 168-register shapes
//                                   PAIRS of tiles (a unit = two neighbouring column blocks of the y block: the x fragment and its operand sum
//                                   feed both, 3 loads per 6 matrix instructions), one set  290.5 -- the two sets of a pair (96 fragment
//                                   registers + 48 of accumulators) do not fit beside the kernel's live state: they spill INSIDE the loop
//   8-wave launch, 50.0 ms:         single tiles, two sets  49.9 (a tie)  <- NOT shipped: the 128-register shape keeps one set, the depth it had
//                                   single tiles, one set  49.15   <- shipped there
// The pair form stays in the source for experiment builds (-DQKF_EDGE_PAIRS_V=1; its units: qk_edge_unit, qk_plan.h).
#ifdef QKF_EDGE_PAIRS_V
#define QKF_EDGE_PAIRS(WPS) (QKF_EDGE_PAIRS_V != 0)
#else
#define QKF_EDGE_PAIRS(WPS) false
#endif
// register sets of a SINGLE tile's streams, by the kernel's waves per SIMD; a pair always runs one set (experiment builds: -DQKF_EDGE_SETS_V=1 | 2)
#ifdef QKF_EDGE_SETS_V
#define QKF_EDGE_SETS(WPS) (QKF_EDGE_SETS_V)
#else
#define QKF_EDGE_SETS(WPS) ((WPS) <= 3 ? 2 : 1)
#endif
// One UNIT of  Ay^T conj(Ax)  (K = 16 ng rows, ng a power of two): the tile of column block `oy` of Ay and, with HAS1, of the column block
// behind it, against ONE column block of Ax.  Ay / Ax are wave-uniform, oy / ox this lane's element of k-step 0 (row q, column 16 t + j),
// ldy / ldx = elements per row.  K = 16 is one group (a second set is never loaded), K = 32 one group per set: the steady loop runs for neither.
__device__ __forceinline__ v2d qkf_lde(const v2d* __restrict__ base, const unsigned boff, const int col = 0) {
  return reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(base) + (size_t)boff)[col];
}
template <bool HAS1, bool MORE>
__device__ __forceinline__ void qkf_edge_group(v4d (&acc)[6], v2d (&fy)[4], v2d (&fz)[4], v2d (&fx)[4], const v2d* const* const by, const v2d* const* const bx, const unsigned boy,
                                               const unsigned box) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double sb = QKF_DIF(fx[i].x, fx[i].y);  // (conjugated operand)
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fy[i].x, fx[i].x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fy[i].y, fx[i].y, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(QKF_SUM(fy[i].x, fy[i].y), sb, acc[2], 0, 0, 0);
    if (HAS1) {
      acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz[i].x, fx[i].x, acc[3], 0, 0, 0);
      acc[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz[i].y, fx[i].y, acc[4], 0, 0, 0);
      acc[5] = __builtin_amdgcn_mfma_f64_16x16x4f64(QKF_SUM(fz[i].x, fz[i].y), sb, acc[5], 0, 0, 0);
    }
    if (MORE) {
      fy[i] = qkf_lde(by[i], boy);
      if (HAS1) fz[i] = qkf_lde(by[i], boy, TILE);
      fx[i] = qkf_lde(bx[i], box);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <bool HAS1, int SETS>
__device__ __forceinline__ void qkf_edge_unit(QkfTile& t0, QkfTile& t1, const v2d* __restrict__ Ay, const unsigned oy, const int ldy, const v2d* __restrict__ Ax, const unsigned ox, const int ldx,
                                              const int ng) {
  static_assert(SETS == 1 || SETS == 2, "one or two groups of k-steps in flight");
  v4d acc[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) acc[e] = (v4d){0, 0, 0, 0};
  v2d fy[SETS][4], fz[SETS][4], fx[SETS][4];
  const v2d *by[4 * SETS], *bx[4 * SETS];  // k-step i of a trip: rows 4 i + q
#pragma unroll
  for (int i = 0; i < 4 * SETS; ++i) by[i] = Ay + 4 * i * ldy, bx[i] = Ax + 4 * i * ldx;
  unsigned boy = oy * 16u, box = ox * 16u;  // this lane's byte offsets: the two running values of the loop
  const unsigned sy = (unsigned)(SETS * TILE * ldy) * 16u, sx = (unsigned)(SETS * TILE * ldx) * 16u;
  const bool two = SETS == 2 && ng > 1;
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    if (s == 0 || two) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fy[s][i] = qkf_lde(by[4 * s + i], boy);
        if (HAS1) fz[s][i] = qkf_lde(by[4 * s + i], boy, TILE);
        fx[s][i] = qkf_lde(bx[4 * s + i], box);
      }
    }
  }
  QKF_PRIO_LO();
#pragma unroll 1
  for (int g = SETS; g < ng; g += SETS) {  // the trips that are followed by another one
    boy += sy, box += sx;
#pragma unroll
    for (int s = 0; s < SETS; ++s) qkf_edge_group<HAS1, true>(acc, fy[s], fz[s], fx[s], by + 4 * s, bx + 4 * s, boy, box);
  }
  qkf_edge_group<HAS1, false>(acc, fy[0], fz[0], fx[0], by, bx, boy, box);
  if constexpr (SETS == 2) {
    if (two) qkf_edge_group<HAS1, false>(acc, fy[1], fz[1], fx[1], by + 4, bx + 4, boy, box);
  }
  QKF_PRIO_HI();
  t0.re = acc[0] + acc[1], t0.im = acc[2] - acc[0] + acc[1];
  if (HAS1) t1.re = acc[3] + acc[4], t1.im = acc[5] - acc[3] + acc[4];
}
// a 64-bit value that is the same in every lane, moved to scalar registers (the bases of the edge streams)
__device__ __forceinline__ long long qkf_uniform(const long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// unit u of a product of mt x nt tiles: single tiles with ta fastest (the shipped kernels), or pairs (qk_edge_unit, qk_plan.h)
template <int NW, bool PAIRS>
__device__ __forceinline__ QkEdgeUnit qkf_edge_unit_of(const int u, const int mt, const int nt, const int inv) {
  if constexpr (PAIRS) return qk_edge_unit(u, mt, nt, NW, inv);
  const int tb = (u * inv) >> 20;
  return QkEdgeUnit{u - tb * mt, tb, false, true};
}
// The environment behind the left edge: X[b][a] = sum_s Ly[s][b] conj(Lx[s][a]), b x a (padded bonds of site edge_k), written in panels of
// 16 columns to LDS (`xl`) or, when it does not fit, to the global X buffer (`xg`); units dealt round-robin to the NW wavefronts.
template <int NW, bool PAIRS, int SETS>
__device__ __forceinline__ void qkf_edge_prefix(const SweepArgs& g, const int xi, const int yj, const int a, const int b, lds_v2d* const xl, v2d* const xg, const bool to_global, const int wave,
                                                const int q, const int j, const bool swap = false) {
  // (swap: a chain that starts in orientation 1 -- xi is then a state of the y set and yj one of the x set, a / b their bonds)
  const v2d* const Lx = reinterpret_cast<const v2d*>(swap ? g.yedge : g.xedge) + qkf_uniform((swap ? g.yedge_offs : g.xedge_offs)[2 * (long long)xi]);
  const v2d* const Ly = reinterpret_cast<const v2d*>(swap ? g.xedge : g.yedge) + qkf_uniform((swap ? g.xedge_offs : g.yedge_offs)[2 * (long long)yj]);
  const int mt = a / TILE, nt = b / TILE, ng = (1 << g.edge_k) >> 4, inv = qk_recip20(mt), units = PAIRS ? qk_edge_units(mt, nt, NW) : mt * nt;  // (K = 2^k >= 16)
  for (int u = wave; u < units; u += NW) {
    const QkEdgeUnit un = qkf_edge_unit_of<NW, PAIRS>(u, mt, nt, inv);
    if (!un.mine) continue;
    QkfTile T0, T1;
    const unsigned oy = (unsigned)(q * b + un.tb0 * TILE + j), ox = (unsigned)(q * a + un.ta * TILE + j);
    if (un.has1) qkf_edge_unit<true, 1>(T0, T1, Ly, oy, b, Lx, ox, a, ng);
    else qkf_edge_unit<false, SETS>(T0, T1, Ly, oy, b, Lx, ox, a, ng);
    const int at = un.ta * (b * TILE) + (un.tb0 * TILE + q) * TILE + j;  // (panels of 16 columns)
    if (to_global) {
#pragma unroll
      for (int r = 0; r < 4; ++r) xg[at + r * QKF_XSTEP] = (v2d){T0.re[r], T0.im[r]};
      if (un.has1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) xg[at + QKF_XBLOCK + r * QKF_XSTEP] = (v2d){T1.re[r], T1.im[r]};
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) xl[at + r * QKF_XSTEP] = (v2d){T0.re[r], T0.im[r]};
      if (un.has1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) xl[at + QKF_XBLOCK + r * QKF_XSTEP] = (v2d){T1.re[r], T1.im[r]};
      }
    }
  }
}

// The overlap at the right edge: z = sum_{b,a} X[b][a] R[b][a], R = Ry^T conj(Rx); X in panels of 16 columns in LDS (`xl`) or in the global
// buffer (`xg`).  Every wavefront leaves its units' share in its own two doubles of `zacc` (LDS, [NW][2]); the caller adds them up in
// wavefront order behind a barrier.  Which tiles a wavefront takes is a pure function of the shape (qk_edge_unit), so the sum is reproducible.
template <int NW, bool PAIRS, int SETS>
__device__ __forceinline__ void qkf_edge_suffix(const SweepArgs& g, const int xi, const int yj, const int a, const int b, const lds_v2d* const xl, const v2d* const xg, const bool from_global,
                                                __attribute__((address_space(3))) double* zacc, const int wave, const int q, const int j, const bool swap = false) {
  // (swap: a chain that ends in orientation 1, as in qkf_edge_prefix; the sum is then conj(z))
  const v2d* const Rx = reinterpret_cast<const v2d*>(swap ? g.yedge : g.xedge) + qkf_uniform((swap ? g.yedge_offs : g.xedge_offs)[2 * (long long)xi + 1]);
  const v2d* const Ry = reinterpret_cast<const v2d*>(swap ? g.xedge : g.yedge) + qkf_uniform((swap ? g.xedge_offs : g.yedge_offs)[2 * (long long)yj + 1]);
  const int mt = a / TILE, nt = b / TILE, ng = (1 << g.edge_k) >> 4, inv = qk_recip20(mt), units = PAIRS ? qk_edge_units(mt, nt, NW) : mt * nt;
  double zr = 0, zi = 0;
  for (int u = wave; u < units; u += NW) {
    const QkEdgeUnit un = qkf_edge_unit_of<NW, PAIRS>(u, mt, nt, inv);
    if (!un.mine) continue;
    QkfTile T0, T1;
    const unsigned oy = (unsigned)(q * b + un.tb0 * TILE + j), ox = (unsigned)(q * a + un.ta * TILE + j);
    if (un.has1) qkf_edge_unit<true, 1>(T0, T1, Ry, oy, b, Rx, ox, a, ng);
    else qkf_edge_unit<false, SETS>(T0, T1, Ry, oy, b, Rx, ox, a, ng);
    const int at = un.ta * (b * TILE) + (un.tb0 * TILE + q) * TILE + j;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const v2d x = from_global ? xg[at + r * QKF_XSTEP] : (v2d)xl[at + r * QKF_XSTEP];
      zr += x.x * T0.re[r] - x.y * T0.im[r], zi += x.x * T0.im[r] + x.y * T0.re[r];
    }
    if (un.has1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const v2d x = from_global ? xg[at + QKF_XBLOCK + r * QKF_XSTEP] : (v2d)xl[at + QKF_XBLOCK + r * QKF_XSTEP];
        zr += x.x * T1.re[r] - x.y * T1.im[r], zi += x.x * T1.im[r] + x.y * T1.re[r];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) zr += __shfl_xor(zr, o), zi += __shfl_xor(zi, o);
  if ((q | j) == 0) zacc[2 * wave] = zr, zacc[2 * wave + 1] = zi;  // one slot per wavefront: the caller adds them up in wavefront order (reproducible)
}

// What a site needs: bonds, tile counts, where its X / X' live and how its items are cut into strips.
struct QkfSite {
  int a, a2, b, b2, at, nks, mt, nt, nn, W, inv, inv2, pd, ps, next;  // inv2 = the two reciprocals of the strips' column units (qk_unit_recips); next = the table entry of the step after this one; pd = physical dimension of the step (2, or 4 for two merged sites), ps = log2 pd; inv = ceil(2^20 / mt): u / mt == (u * inv) >> 20 for u < 2048, mt <= 32 (checked exhaustively)
  int flags;  // word [7] of the record: LDS-resident, orientation, switch, and the residency of X (qk_plan.h: qk_rec_resident)
  bool small, sw;  // sw: the step ends with a switch of orientation (qkf_p2_switch)
  const v2d *Ak, *Bk;
};
typedef int v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i lds_v4i;

// The step table of a pair, built by all threads at pair set-up: per step 12 ints (48 bytes)
//   [0] a  [1] a2  [2] b  [3] b2  [4] true a  [5] k-steps of b  [6] W  [7] small | orientation << 1 | switch << 2 | the residency of X (qk_plan.h: qk_rec_resident)  [8] ceil(2^20 / mt)  [9] log2 pd  [10] next step
//   [11] ITEM_RECIPS (the one-tile kernel's order of items): ceil(2^15 / column blocks) of a full strip | of the last strip << 16 (qk_unit_recips)
// and the addresses of the step's two tensors ([a][pd][a2] of x, [b][pd][b2] of y) in a second table.  A step is one site (pd = 2,
// entry = the site's index, next = + 1) or, with a merged image, two sites contracted into one tensor of physical dimension 4 (entry =
// the first site's index, next = + 2).  The merged step does the same matrix work as its two sites when the bond between them is as
// large as the bonds around them, with half the barriers, set-ups and stream turn-arounds, and less where the true middle bond would
// have been padded.  Which steps are merged is the pair's segmentation mask (SweepArgs.seg; qk_plan.h: qk_segment_chain, where the rule
// lives): one thread per site, a site whose bit is set writes the merged entry, any other site the plain one (the second site of a
// merged step is then never visited).  `rule`: the launch's shape, as the mask was made with -- here it tells the LDS-resident steps.
// The pair's second mask holds the ORIENTATION of every step (qk_plan.h: the association of a step): a step in orientation 1 gets the
// record of the exchanged states (qk_step_record) and its two tensor offsets exchanged -- still offsets from xdata and ydata --, and a
// step whose successor has the other orientation is flagged as a switch step (qkf_p2_switch).
template <int XCAP, int NT, bool ITEM_RECIPS = false>
__device__ __forceinline__ void qkf_step_table(const SweepArgs& g, const int xi, const int yj, const long long pair, lds_v4i* const rec, long long* const m_off, const int tid, const QkSegRule rule) {
  const int ns = g.n_sites, n1 = ns + 1;
  const int32_t* const xd = g.xdims + (long long)xi * n1;
  const int32_t* const yd = g.ydims + (long long)yj * n1;
  const int32_t* const xt = g.xtrue + (long long)xi * n1;
  const int32_t* const yt = g.ytrue + (long long)yj * n1;
  const v2d* const xdata = reinterpret_cast<const v2d*>(g.xdata);
  const v2d* const ydata = reinterpret_cast<const v2d*>(g.ydata);
  // the record (qk_plan.h: qk_step_record) and the step's two tensors: X of the state that plays x, Y of the one that plays y -- exchanged in
  // orientation 1, where the first offset still counts from xdata and the second from ydata
  auto put = [&](const int e, const int len, const int o, const bool sw, const v2d* const X, const v2d* const Y) __attribute__((always_inline)) {
    const QkStepRec r = qk_step_record(xd, xt, yd, yt, e, len, o, sw, rule, ITEM_RECIPS);
    rec[3 * e] = (v4i){r.w[0], r.w[1], r.w[2], r.w[3]};
    rec[3 * e + 1] = (v4i){r.w[4], r.w[5], r.w[6], r.w[7]};
    rec[3 * e + 2] = (v4i){r.w[8], r.w[9], r.w[10], r.w[11]};
    // (as element offsets from the sets' plain images, whatever buffer the tensor lives in: the kernels add them to their pointer
    //  ARGUMENTS, which keeps the fragment loads global_load -- an address that comes out of the table as an integer makes them
    //  flat_load, whose waits cover the LDS counter as well)
    m_off[2 * e] = (long long)(((const char*)(o ? Y : X) - (const char*)xdata) / 16);
    m_off[2 * e + 1] = (long long)(((const char*)(o ? X : Y) - (const char*)ydata) / 16);
  };
  auto plain = [&](const int e, const int o, const bool sw) __attribute__((always_inline)) {
    put(e, 1, o, sw, xdata + (g.xoffs[(long long)xi * ns + e] >> 1), ydata + (g.yoffs[(long long)yj * ns + e] >> 1));
  };
  if (g.seg == nullptr) {
    for (int e = tid; e < ns; e += NT) plain(e, 0, false);
    return;
  }
  const int ek = g.edge_k, k_hi = ns - ek;
  // the pair's four words: the merges, then the orientations (all zero for a launch whose kernel has no switch step)
  const unsigned long long w0 = g.seg[4 * pair], w1 = g.seg[4 * pair + 1], o0 = g.seg[4 * pair + 2], o1 = g.seg[4 * pair + 3];
  for (int e = ek + tid; e < k_hi; e += NT) {
    const int i = e - ek;
    const bool merged = qk_seg_bit(w0, w1, i) && e + 1 < k_hi;
    const int len = merged ? 2 : 1, o = qk_seg_bit(o0, o1, i) ? 1 : 0;
    const bool sw = qk_seg_bit(o0, o1, i + len) != (o != 0);  // the successor (or the chain's end) has the other orientation
    if (merged)
      put(e, 2, o, sw, reinterpret_cast<const v2d*>(g.xmg) + (g.xmg_offs[(long long)xi * g.merge_steps + i] >> 1),
          reinterpret_cast<const v2d*>(g.ymg) + (g.ymg_offs[(long long)yj * g.merge_steps + i] >> 1));
    else plain(e, o, sw);
  }
}

// experiment builds only (-DQKF_PROF): cycle sums per section of a wave's life, added up over all waves into SweepArgs.prof[0..7]
// (lab/tools/fused_sections.py; printed by qk_get_stats of such a build)
#ifdef QKF_PROF
#define QKF_PROF_DECL() \
  unsigned long long pf[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt = __builtin_amdgcn_s_memtime(); \
  const unsigned long long pt0 = pt
#define QKF_STAMP(i)                                              \
  do {                                                            \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    pf[i] += now_ - pt;                                           \
    pt = now_;                                                    \
  } while (0)
#define QKF_PROF_FLUSH()                                             \
  do {                                                               \
    if (lane == 0) {                                                 \
      pf[7] = __builtin_amdgcn_s_memtime() - pt0;                    \
      for (int i_ = 0; i_ < 8; ++i_) atomicAdd(g.prof + i_, pf[i_]); \
    }                                                                \
  } while (0)
#else
#define QKF_PROF_DECL()
#define QKF_STAMP(i)
#define QKF_PROF_FLUSH()
#endif

// (dual kernel) The workgroup's next pair into a word of its queue slot: called by ONE lane -- lane 0 of the LAST wavefront, which has the fewest units of
// a ragged round of the right edge (units are dealt from wavefront 0 up), so the queue's atomic mostly waits while that wavefront would idle.
#define QKF_PULLER(NT) ((NT) - 64)
__device__ __forceinline__ void qkf_pull_next(const SweepArgs& g, const int xcc, int& gang_round, long long* const word) {
  const long long pp = qk_pull(g, xcc);  // this XCD's queue first: the workgroups that share an L2 stream the same few states
  qk_gang_sync(g, xcc, pp >= 0, gang_round);
  *word = pp;
}

template <int NW, int S, int XCAP, int WPS, bool DET = false, int RCAP = XCAP>  // waves per workgroup; T slots per wave (a round holds NW * S items); elements of the LDS X buffer as the segmentation sees it; waves per SIMD (register budget); ordered accumulation (bit-reproducible); elements the buffer really has (the residency of X: qk_plan.h, qk_resident)
__global__ __launch_bounds__(64 * NW, WPS) void qk_sweep_fused_kernel(const SweepArgs g) {
  constexpr int NT = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) double lds_raw[];
  lds_v2d* const XL = (lds_v2d*)lds_raw;  // (a C-style cast: the generic -> LDS address-space cast)
  static_assert(RCAP >= XCAP && RCAP % QKF_XBLOCK == 0, "the buffer holds what the segmentation counts on, in whole blocks");
  long long* const slot = reinterpret_cast<long long*>(lds_raw + 2 * RCAP);
  const v2d* const xdata = reinterpret_cast<const v2d*>(g.xdata);  // interleaved complex128 images
  const v2d* const ydata = reinterpret_cast<const v2d*>(g.ydata);
  v2d* const G0 = reinterpret_cast<v2d*>(g.scratch) + (long long)blockIdx.x * 2 * g.x_plane;  // two global X buffers of x_plane complex
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int ns = g.n_sites;
  // the step table of the current pair (qkf_step_table): 12 ints per step, and the addresses of the step's two tensors in a second table
  __attribute__((address_space(3))) double* const zacc = (__attribute__((address_space(3))) double*)(slot + 2);  // the overlap's partial sums (edge blocks): [16 wavefronts][2]
  lds_v4i* const rec = (lds_v4i*)(slot + 2 + 32);
  long long* const m_off = reinterpret_cast<long long*>(slot + 2 + 32) + 6 * (long long)ns;  // [ns][2]: A_k, B_k
  lds_int* const tbroken = (lds_int*)(m_off + 2 * (long long)ns);  // DET: the workgroup's sticky 'a wait ran out' flag, then
  lds_int* const turn0 = tbroken + 2;                              // two sets of g.turn_ints turn counters (qkf_turn_add)
  auto rfl = [&](const int v) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(v); };
  auto ldl = [&](const long long* p_) __attribute__((always_inline)) {
    const long long v = *p_;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
  };
  auto site = [&](const int k) __attribute__((always_inline)) {
    const v4i r0 = rec[3 * k], r1 = rec[3 * k + 1], r2 = rec[3 * k + 2];  // every lane reads the same 48 bytes
    QkfSite s;
    s.a = rfl(r0.x), s.a2 = rfl(r0.y), s.b = rfl(r0.z), s.b2 = rfl(r0.w);
    s.at = rfl(r1.x), s.nks = rfl(r1.y), s.W = rfl(r1.z), s.flags = rfl(r1.w), s.small = (s.flags & QK_REC_SMALL) != 0, s.sw = (s.flags & QK_REC_SWITCH) != 0;
    s.inv = rfl(r2.x), s.inv2 = rfl(r2.w);
    s.ps = rfl(r2.y), s.pd = 1 << s.ps, s.next = rfl(r2.z);
    s.mt = s.a / TILE, s.nt = s.b2 / TILE, s.nn = s.a2 / TILE;
    s.Ak = xdata + ldl(m_off + 2 * k);      // [a][pd][a2]
    s.Bk = ydata + ldl(m_off + 2 * k + 1);  // [b][pd][b2]
    return s;
  };
  // item `it` of a strip of w column blocks as (ta, tc = block of the strip, p): the order of qk_plan.h -- p slowest, so that the waves of a
  // round share both operands; the ordered form keeps p fastest (its turn index rises along `it`)
  auto item_of = [&](const QkfSite& s, const int w, const int it) __attribute__((always_inline)) {
    return DET ? qk_unit_decode_ordered(it, s.ps, s.mt, s.inv) : qk_unit_decode(it, s.mt, w, s.inv, qk_unit_recip_of(s.inv2, w == s.W));
  };
  // the streams of item `it` of a strip of w blocks starting at block s0
  auto b_stream = [&](const QkfSite& s, const int s0, const int w, const int it) __attribute__((always_inline)) {
    const QkUnit un = item_of(s, w, it);
    return QkfStream{s.Bk + un.p * s.b2, (unsigned)((q * s.pd) * s.b2 + (s0 + un.tc) * TILE + j), 4 * s.pd * s.b2, min(4, s.nks)};
  };
  auto a_stream = [&](const QkfSite& s, const int w, const int it) __attribute__((always_inline)) {
    const QkUnit un = item_of(s, w, it);
    return QkfStream{s.Ak + un.p * s.a2, (unsigned)(((un.ta * TILE + q) * s.pd) * s.a2 + j), 4 * s.pd * s.a2, min(4, (s.at - un.ta * TILE + 3) >> 2)};
  };
  QKF_PROF_DECL();
  const int xcc = qk_xcc_id();
  int gang_round = 0;  // (gang start: this workgroup's pairs so far)
  if (tid == 0) qk_tail_start(g);
  for (;;) {
    if (tid == 0) {
      const long long pp_ = qk_pull(g, xcc);
      qk_gang_sync(g, xcc, pp_ >= 0, gang_round);
      *slot = pp_;
    }  // this XCD's queue first: the workgroups that share an L2 stream the same few states
    __syncthreads();
    const long long p = *slot;
    __syncthreads();
    if (p < 0) break;
    const int xi = g.pairs[2 * p], yj = g.pairs[2 * p + 1];
    // an item is (ta, tb, p): pd mt nt of them.  LDS-resident step: X and X' fit the buffer and either ONE round holds all items
    // (X' may then overwrite X) or X and X' fit side by side (any number of rounds: X stays intact);
    // otherwise X' is built in strips of W blocks of b' (the strip's rows must fit the LDS), items in rounds of NW * S
    qkf_step_table<XCAP, NT, true>(g, xi, yj, p, rec, m_off, tid, QkSegRule{XCAP, NW * S, false, RCAP, QKF_RES_PARTIAL != 0});
    const int ek = g.edge_k, k_hi = ns - ek;  // the chain runs over the sites [ek, k_hi): the ends are in the edge blocks
    const bool edges = ek > 0;
    if (!edges)
      for (int e = tid; e < TILE * TILE; e += NT) XL[e] = (v2d){e == 0 ? 1.0 : 0.0, 0.0};  // X_0 = 1 in a 16 x 16 block
    if constexpr (DET)
      for (int e = tid; e < 2 * g.turn_ints + 2; e += NT) tbroken[e] = 0;
    int tsel = 0;  // DET: the set of turn counters in use (the other one is zeroed meanwhile for the next strip or step)
    __syncthreads();
    int cur = 0, xb = 0;  // where X lives: LDS (at element xb, in panels) while it fits the segmentation's buffer, else the global buffer G0 + cur * x_plane
    if (edges) {  // X behind the left edge: one product of the two left blocks
      const v4i r0 = rec[3 * ek];
      const int a_e = rfl(r0.x), b_e = rfl(r0.z);  // (of a chain that starts in orientation 1: the record of the exchanged states)
      const bool o1 = !DET && (rfl(rec[3 * ek + 1].w) & QK_REC_ORIENT) != 0;  // (the ordered forms run orientation 0 throughout)
      qkf_edge_prefix<NW, QKF_EDGE_PAIRS(WPS), QKF_EDGE_SETS(WPS)>(g, o1 ? yj : xi, o1 ? xi : yj, a_e, b_e, XL, G0, a_e * b_e > XCAP, wave, q, j, o1);
      __syncthreads();
    }
    QKF_STAMP(0);  // pair set-up
    QkfTile T[S];
    v2d fr[4];            // the fragment registers of the wave's global stream: they carry its next group across tiles and barriers
    bool primed = false;  // fr holds the first group of the wave's next tile
    QkfSite sn = site(ek);
    for (int k = ek; k < k_hi;) {
      const QkfSite sc = sn;
      k = sc.next;  // (from here on: the entry of the NEXT step)
      if (k < k_hi) sn = site(k);
      const int a = sc.a, a2 = sc.a2, b = sc.b, mt = sc.mt, nt = sc.nt, W = sc.W;
      const bool small = sc.small;
      v2d* const Gc = G0 + (long long)cur * g.x_plane;
      v2d* const Gn = G0 + (long long)(cur ^ 1) * g.x_plane;
      // ---- where X has to be for this site: the residency rule (qk_plan.h: qk_resident) says where X' is built and which panels of X
      // phase 1 reads from LDS -- [klo, khi), the others from the global buffer Gc
      const int n_out = sc.b2 * a2;
      // (X is in LDS exactly when it fits the segmentation's buffer: the left edge or the step before left it there whole, at xb; else it is in Gc, whole)
      const QkResident rs = qk_rec_resident(sc.flags, mt, n_out, RCAP, xb != 0);
      if (a * b <= XCAP && rs.khi - rs.klo < mt) {  // LDS -> global: the panels that X' (or its strips) will overlap -- all of them, or the ones outside [klo, khi)
        const int e0 = (rs.klo == 0 ? rs.khi : 0) * (b * TILE), e1 = (rs.klo == 0 ? mt : rs.klo) * (b * TILE);
        for (int e = e0 + tid; e < e1; e += NT) Gc[e] = XL[xb + e];
        __syncthreads();
      }
      const unsigned xgm = qk_res_global_mask(rs);  // bit ta: the units of row block ta read their panel of X from Gc
      // When X and X' fit the buffer side by side, X' goes to the other end and is zeroed right here
      // (that region held the X of the previous site, dead since its last barrier): one barrier between the phases
      // instead of barrier - zero - barrier.  A partially resident step builds X' at the other end too, in the manner of a single strip.
      // Otherwise X' overwrites X from element 0.
      const bool pingpong = rs.kind == QK_RES_SIDE;
      const int ob = rs.ob;  // where X' (or the strip of X') is built
      if (pingpong && !DET)
        for (int e = tid; e < n_out; e += NT) XL[ob + e] = (v2d){0.0, 0.0};
      QKF_STAMP(1);  // X moved between LDS and the global buffer
      for (int s0 = 0; s0 < nt; s0 += W) {
        const int w = min(W, nt - s0), items = sc.pd * mt * w;
        lds_int* const tcur = turn0 + tsel * g.turn_ints;
        if constexpr (DET) {  // (ordered accumulation: the first contribution to a block stores, nothing is zeroed but the next set of counters)
          for (int e = tid; e < g.turn_ints; e += NT) turn0[(tsel ^ 1) * g.turn_ints + e] = 0;
        } else if (!small && !pingpong) {  // zero this strip's X' rows (the in-place path zeroes after phase 1: X is still being read)
          for (int e = tid; e < w * TILE * a2; e += NT) XL[ob + e] = (v2d){0.0, 0.0};
          QKF_STEP_BARRIER();
        }
        QKF_STAMP(6);  // strip zeroing
        for (int r0 = 0; r0 < items; r0 += NW * S) {  // (LDS-resident sites: one round, or several when X and X' sit side by side)
          const int L = min(S, (items - r0 + NW - 1) / NW);  // slots in use this round (the same for every wave)
          const bool multi = L > 1;
          const int it0 = r0 + wave;          // this wave's items: it0, it0 + NW, ...
          // ---- phase 1: the T tile of each of this wave's items
          // (xbase: where this wave's items read X -- the LDS, the global buffer, or, with more than one slot, nullptr: per item by its panel)
          auto phase1 = [&](auto xbase) __attribute__((always_inline)) {
#pragma unroll 1
            for (int s = 0; s < L; ++s) {
              if (multi) qkf_rotate<S>(T, L);
              const int it = it0 + NW * s;
              if (it < items) {
                const int ta = item_of(sc, w, it).ta;
                const bool more = s + 1 < L && it + NW < items;  // another tile follows in this phase; else phase 2 starts with item it0
                const QkfStream nxt = more ? b_stream(sc, s0, w, it + NW) : a_stream(sc, w, it0);
                const unsigned xoff = (unsigned)(ta * (b * TILE) + q * TILE + j);
                if constexpr (std::is_same<decltype(xbase), std::nullptr_t>::value) {
                  if ((xgm >> ta) & 1u) qkf_p1_tile(T[S - 1], fr, primed, b_stream(sc, s0, w, it), (const v2d*)Gc, xoff, sc.nks, nxt);
                  else qkf_p1_tile(T[S - 1], fr, primed, b_stream(sc, s0, w, it), (const lds_v2d*)(XL + xb), xoff, sc.nks, nxt);
                } else {
                  qkf_p1_tile(T[S - 1], fr, primed, b_stream(sc, s0, w, it), xbase, xoff, sc.nks, nxt);
                }
                primed = true;
              }
            }
          };
          // one slot: the wave has one item per round, so its panel decides for the whole call (the loop then holds ONE form of the tile, as it
          // did when the choice was per step: with both forms in the loop the 128-register kernel spills twice as much)
          if constexpr (S == 1) {
            if (it0 < items && ((xgm >> item_of(sc, w, it0).ta) & 1u)) phase1((const v2d*)Gc);
            else phase1((const lds_v2d*)(XL + xb));
          } else {
            phase1(nullptr);
          }
          QKF_STAMP(2);  // phase 1
          if ((small || pingpong) && r0 == 0 && !(DET && pingpong)) {
            QKF_STEP_BARRIER();  // ping-pong: X' is zero everywhere; in place (one round): every wave has read X, it becomes X'
            if (!pingpong && !DET) {
              for (int e = tid; e < n_out; e += NT) XL[e] = (v2d){0.0, 0.0};
              QKF_STEP_BARRIER();
            }
          }
          QKF_STAMP(3);  // wait for the other waves' phase 1, zero X'
          // ---- phase 2: add the items' contributions to X'[strip rows]
          const bool last_round = s0 + W >= nt && r0 + NW * S >= items;
#pragma unroll 1
          for (int s = 0; s < S; ++s) {
            const int it = it0 + NW * s;
            if (it >= items) break;
            if (multi) qkf_rotate<S>(T, L);
            const QkUnit un = item_of(sc, w, it);
            const int ta = un.ta, tbl = un.tc;
            const int kmax = min(4, (sc.at - ta * TILE + 3) >> 2);
            const bool more = s + 1 < S && it + NW < items;
            // after the wave's last item of the site: its first tile of the next site (strip 0, round 0), if it has one
            const int wn = min(sn.W, sn.nt);
            const bool chain = !more && last_round && k < k_hi && wave < sn.pd * sn.mt * wn;
            const QkfStream nxt = more ? a_stream(sc, w, it + NW) : chain ? b_stream(sn, 0, wn, wave) : a_stream(sc, w, it);
            const int tix = sc.pd * ta + un.p;  // (ordered form) this contribution's place in the order of its block of rows
            const QkfTurn turn{tcur + tbl * sc.nn, tix, tbroken, g.err};
            constexpr int FORM = DET ? 0 : WPS >= 4 ? QKF_P2_FORM_TWO : QKF_P2_FORM_ONE;  // the form of the plain column blocks (qkf_p2_onesum)
            if (!DET && sc.sw) {  // the step ends with a switch: the tile of X'^H, to block tbl's panel of the other orientation (LDS-resident: w = nt)
              lds_double* const dsw = (lds_double*)(XL + ob + tbl * (a2 * TILE) + q * TILE + j);
              if (FORM != 0 && kmax == 4) qkf_p2_switch<true, false, FORM>(T[S - 1], T[S - 1], fr, primed, a_stream(sc, w, it), 4, sc.nn, 4, dsw, 0, nxt);
              else qkf_p2_switch<false, false, FORM>(T[S - 1], T[S - 1], fr, primed, a_stream(sc, w, it), kmax, sc.nn, kmax, dsw, 0, nxt);
            } else if (kmax == 4) qkf_p2_item<true, DET, FORM>(T[S - 1], fr, primed, a_stream(sc, w, it), w * QKF_XBLOCK, sc.nn, 4, XL + ob + tbl * QKF_XBLOCK, q, j, nxt, turn);
            else qkf_p2_item<false, DET, FORM>(T[S - 1], fr, primed, a_stream(sc, w, it), w * QKF_XBLOCK, sc.nn, kmax, XL + ob + tbl * QKF_XBLOCK, q, j, nxt, turn);
            primed = more || chain;
          }
          QKF_STAMP(4);  // phase 2
        }
        QKF_STEP_BARRIER();  // the strip of X' is complete
        tsel ^= 1;
        QKF_STAMP(5);      // wait for the other waves' phase 2
        if (!small && nt > W) {  // several strips: this one goes to the other global buffer
          for (int tn = 0; tn < sc.nn; ++tn)  // (panel by panel: the strip's rows of a panel are contiguous in both buffers)
            for (int e = tid; e < w * QKF_XBLOCK; e += NT) Gn[(long long)tn * (sc.b2 * TILE) + s0 * QKF_XBLOCK + e] = XL[tn * w * QKF_XBLOCK + e];
          __syncthreads();
          QKF_STAMP(1);
        }
      }
      if (nt > W) cur ^= 1, xb = 0;  // X' was written strip by strip to Gn
      else xb = ob;                  // X' is complete in LDS
    }
    // the orientation the chain ends in: that of its last step (whose second site, if it is a merged one, carries the same flags), switched once more if that step switches
    const int fl_end = DET ? 0 : rfl(rec[3 * (k_hi - 1) + 1].w);
    const bool sw_end = (fl_end & QK_REC_SWITCH) != 0, o_end = ((fl_end & QK_REC_ORIENT) != 0) != sw_end;
    if (edges) {  // the overlap: X against the product of the two right blocks
      const v4i r0 = rec[3 * (k_hi - 1)];
      const int a_l = rfl(r0.y), b_l = rfl(r0.w), a_e = sw_end ? b_l : a_l, b_e = sw_end ? a_l : b_l;  // (the last record is in the last step's orientation)
      qkf_edge_suffix<NW, QKF_EDGE_PAIRS(WPS), QKF_EDGE_SETS(WPS)>(g, o_end ? yj : xi, o_end ? xi : yj, a_e, b_e, (const lds_v2d*)(XL + xb), (const v2d*)(G0 + (long long)cur * g.x_plane), a_e * b_e > XCAP, zacc, wave,
                                                                   q, j, o_end);
      __syncthreads();
    }
    if (tid == 0) {
      v2d zz = {0.0, 0.0};
      if (edges)
        for (int w_ = 0; w_ < NW; ++w_) zz.x += zacc[2 * w_], zz.y += zacc[2 * w_ + 1];
      else zz = (v2d)XL[xb];  // (a chain without edge blocks ends in a 16 x 16 block: in LDS)
      if (o_end) zz.y = -zz.y;  // a chain that ends in orientation 1 yields conj(z)
      g.values[p] = zz.x * zz.x + zz.y * zz.y;
      if (g.z) {
        g.z[2 * p] = zz.x;
        g.z[2 * p + 1] = zz.y;
      }
    }
    __syncthreads();
  }
  if (tid == 0) qk_tail_exit(g);
  QKF_PROF_FLUSH();
}

// ----------------------------------------------------------------------------------------
// The DUAL form of the site-fused sweep: the unit of work is a pair of tiles T[ta, p, tb0], T[ta, p, tb0 + 1] (same rows
// of X and of A, neighbouring column blocks of B).  Phase 1 reads each X fragment once for both tiles; phase 2 reads each
// fragment of A once and feeds it to both tiles: half the A fragments, half the X fragments and half the per-item set-up
// of the single-tile form for the same matrix work.  One pair per wave and round, so there are no slots to rotate.
// ----------------------------------------------------------------------------------------
template <bool HAS1, typename XPtr>
__device__ __forceinline__ void qkf_p1_dual(QkfTile& t0, QkfTile& t1, v2d (&fr)[4], v2d (&fs)[4], const bool primed, QkfStream cur, XPtr xp, unsigned xoff, const int nks,
                                            const QkfStream nxt) {
  v4d p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0}, r2 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
  v2d fx[4];
  if (!primed) qkf_load4(fr, cur);
  if (HAS1) {  // (the second column block is not carried across units: 16 registers less through phase 2)
#pragma unroll
    for (int i = 0; i < 4; ++i) fs[i] = qkf_ldg(cur.base + i * cur.step, cur.off + TILE);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) fx[i] = qkf_ldx(xp + i * QKF_XSTEP, xoff);
  const int ng = (nks + 3) >> 2, last = nks - 4 * (ng - 1);  // k-steps of the last group: 1..4
  QKF_PRIO_LO();
  int gq = 0;
  // (the first k-step of a chain of more than four k-steps STARTS the accumulators -- literal zero as the C operand --: no register moves to zero them)
  if (ng >= 2) {
    gq = 1;
    cur.off += 4 * cur.step, xoff += 4 * QKF_XSTEP;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i == 0) {
        const v4d z = {0, 0, 0, 0};
        const double sa = QKF_SUM(fx[0].x, fx[0].y);
        p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(fx[0].x, fr[0].x, z, 0, 0, 0);
        p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fx[0].y, fr[0].y, z, 0, 0, 0);
        p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, QKF_SUM(fr[0].x, fr[0].y), z, 0, 0, 0);
        if (HAS1) {
          r1 = __builtin_amdgcn_mfma_f64_16x16x4f64(fx[0].x, fs[0].x, z, 0, 0, 0);
          r2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fx[0].y, fs[0].y, z, 0, 0, 0);
          r3 = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, QKF_SUM(fs[0].x, fs[0].y), z, 0, 0, 0);
        }
      } else {
        qkf_kstep<false>(p1, p2, p3, fx[i].x, fx[i].y, fr[i].x, fr[i].y);
        if (HAS1) qkf_kstep<false>(r1, r2, r3, fx[i].x, fx[i].y, fs[i].x, fs[i].y);
      }
      if (!(QKF_ABL & 2)) fr[i] = qkf_ldg_b(cur.base + i * cur.step, cur.off);
      if (HAS1 && !(QKF_ABL & 2)) fs[i] = qkf_ldg_b(cur.base + i * cur.step, cur.off + TILE);
      if (!(QKF_ABL & 8)) fx[i] = qkf_ldx(xp + i * QKF_XSTEP, xoff);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll 1
  for (; gq + 1 < ng; ++gq) {
    cur.off += 4 * cur.step, xoff += 4 * QKF_XSTEP;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qkf_kstep<false>(p1, p2, p3, fx[i].x, fx[i].y, fr[i].x, fr[i].y);
      if (HAS1) qkf_kstep<false>(r1, r2, r3, fx[i].x, fx[i].y, fs[i].x, fs[i].y);
      if (!(QKF_ABL & 2)) fr[i] = qkf_ldg_b(cur.base + i * cur.step, cur.off);
      if (HAS1 && !(QKF_ABL & 2)) fs[i] = qkf_ldg_b(cur.base + i * cur.step, cur.off + TILE);
      if (!(QKF_ABL & 8)) fx[i] = qkf_ldx(xp + i * QKF_XSTEP, xoff);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < last) {
      qkf_kstep<false>(p1, p2, p3, fx[i].x, fx[i].y, fr[i].x, fr[i].y);
      if (HAS1) qkf_kstep<false>(r1, r2, r3, fx[i].x, fx[i].y, fs[i].x, fs[i].y);
    }
    if (!(QKF_ABL & 2)) fr[i] = qkf_ldg(nxt.base + i * nxt.step, nxt.off);  // the first group of this pair's phase 2 (one stream: A)
    __builtin_amdgcn_sched_barrier(0);
  }
  QKF_PRIO_HI();
  t0.re = p1 - p2, t0.im = p3 - p1 - p2;
  if (HAS1) t1.re = r1 - r2, t1.im = r3 - r1 - r2;
}

// Phase 2 of a pair of tiles: X'[tb0 rows | tb0 + 1 rows, tn cols] += T0^T | T1^T conj(A[16 ta + ., p, 16 tn + .]).  `nxt` is the
// wave's next phase-1 stream (NXT_P1: both column blocks are loaded, the second one at + n1 elements) or a dummy.
// On gfx950 a vector-ALU instruction is not free beside the fp64 matrix instructions: whichever wave of the SIMD issues it, it takes 6 - 9
// cycles that the matrix pipe then stands still (lab/tools/mfma_rate.hip: 64.6 cycles per v_mfma_f64_16x16x4_f64 alone, + 6.6 per 32-bit and
// + 9.2 per 64-bit instruction put between them at two waves per SIMD).  So the loop over the column blocks is written for FEW instructions:
// the sums re + im of the T tiles' k-steps are taken once per unit, not once per block; the loop runs over the blocks that are followed by
// another block of this stream -- the four k-steps' addresses are then a lane offset on four wave-uniform bases that do not change -- and the
// last block, which reloads the registers with the first group of `nxt`, stands behind it; the product's second 3M form saves a third of
// the additions behind a block.  cfg4, one box, step by step: 374.4 -> 370.6 (this loop) -> 368.0 (3M form) -> 364.3 (phase 1 started by its
// first k-step) -> 363.9 ms (the same in the one-tile kernel).
// (What follows describes the FIRST tuned form, qkf_p2_block: round 7's, two operand sums per fragment element.  The shipped plain form is
// the one-sum block qkf_p2_onesum above, which keeps its order -- k1 first, the chains started on it -- and halves its additions;
// qkf_p2_block stays for A/B builds, -DQKF_P2_FORM_DUAL=0.)
// The additions BEHIND a block are gone altogether (lab/NOTES_r07.md): with  k1 = (tr + ti) Ar,  k2 = tr (Ar + Ai),  k3 = ti (Ar - Ai)  the
// product is re = k1 - k3, im = k1 - k2, and a matrix instruction adds its C operand for nothing.  So k1 of the block's k-steps is formed
// first (chain started on the literal zero), and the chains of re = k1 + sum ti (Ai - Ar) and im = k1 - sum tr (Ar + Ai) START on it: the
// first matrix instruction of `re` reads k1 as its C operand and writes other registers, `im` goes on in k1's registers -- three accumulator
// sets per tile, as before.  The signs ride on the operand sums (source modifiers of the v_add_f64), which are formed while k1 runs, so the
// registers of a k-step are reloaded right behind its k1: the loads keep their distance of a whole block.  Per block of a pair: 24 matrix
// instructions, 8 v_add_f64 (16 tail additions gone), 16 ds_add_f64.
// one column block: k1 of the k-steps in `fr`, each followed by the reload of its registers from (b_i, off); the chains of re and im; then the
// results added to X' at d (and d1 for the second tile)
template <bool FULL, bool HAS1>
__device__ __forceinline__ void qkf_p2_block(const QkfTile& t0, const QkfTile& t1, const v4d& s0, const v4d& s1, v2d (&fr)[4], const int kmax, const v2d* const b0, const v2d* const b1,
                                             const v2d* const b2, const v2d* const b3, const unsigned off, lds_double* const d, lds_double* const d1, const long rs) {
  const v4d z = {0, 0, 0, 0};
  v4d p1 = z, r1 = z, re, im, re1, im1;
  double sp[4], sm[4];
  QKF_PRIO_LO();
  // k1 of the block's k-steps (k-step 0 always lies below the bond and starts the chain on the literal zero)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (FULL || i == 0 || i < kmax) {
      p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(s0[i], fr[i].x, i == 0 ? z : p1, 0, 0, 0);
      if (HAS1) r1 = __builtin_amdgcn_mfma_f64_16x16x4f64(s1[i], fr[i].x, i == 0 ? z : r1, 0, 0, 0);
      sp[i] = QKF_DIF(-fr[i].x, fr[i].y), sm[i] = QKF_DIF(fr[i].y, fr[i].x);
    }
    if (!(QKF_ABL & 2)) fr[i] = qkf_ldg_a(i == 0 ? b0 : i == 1 ? b1 : i == 2 ? b2 : b3, off);
    __builtin_amdgcn_sched_barrier(0);
  }
  // re = k1 + sum ti (Ai - Ar), im = k1 - sum tr (Ar + Ai): both chains START on k1 (the first matrix instruction of `re` reads p1 as its C
  // operand and writes other registers, `im` goes on in p1's), the signs ride on the operand sums as source modifiers
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (FULL || i == 0 || i < kmax) {
      re = __builtin_amdgcn_mfma_f64_16x16x4f64(t0.im[i], sm[i], i == 0 ? p1 : re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f64_16x16x4f64(t0.re[i], sp[i], i == 0 ? p1 : im, 0, 0, 0);
      if (HAS1) {
        re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(t1.im[i], sm[i], i == 0 ? r1 : re1, 0, 0, 0);
        im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(t1.re[i], sp[i], i == 0 ? r1 : im1, 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  QKF_PRIO_HI();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    __hip_atomic_fetch_add(d + r * rs, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(d + r * rs + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (HAS1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      __hip_atomic_fetch_add(d1 + r * rs, re1[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(d1 + r * rs + 1, im1[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}
// the loop of the DET forms (ordered accumulation): one body for every column block, the last one selecting `nxt`, the product in its first 3M
// form (measured: the split loop of the plain form makes the ordered form 3.5 % slower)
template <bool FULL, bool HAS1, bool DET>
__device__ __forceinline__ void qkf_p2_dual_turn(const QkfTile& t0, const QkfTile& t1, v2d (&fr)[4], v2d (&fs)[4], QkfStream cur, const int ps, const int nn, const int kmax, lds_v2d* xo, const int q,
                                            const int j, const QkfStream nxt, const bool nxt_p1, const unsigned n1, const QkfTurn turn = QkfTurn{nullptr, 0, nullptr, nullptr}) {
  __attribute__((address_space(3))) double* d = (__attribute__((address_space(3))) double*)(xo + q * TILE + j);
#pragma unroll 1
  for (int tn = 0; tn < nn; ++tn) {
    v4d p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0}, r2 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
    const bool fin = tn + 1 == nn;
    const v2d* const rb = fin ? nxt.base : cur.base;
    const int rs = fin ? nxt.step : cur.step;
    cur.off = fin ? nxt.off : cur.off + TILE;
    QKF_PRIO_LO();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (FULL || i < kmax) {
        qkf_kstep<true>(p1, p2, p3, t0.re[i], t0.im[i], fr[i].x, fr[i].y);
        if (HAS1) qkf_kstep<true>(r1, r2, r3, t1.re[i], t1.im[i], fr[i].x, fr[i].y);
      }
      fr[i] = qkf_ldg_a(rb + i * rs, cur.off);
      __builtin_amdgcn_sched_barrier(0);
    }
    QKF_PRIO_HI();
    {
      const v4d re = p1 + p2, im = p3 - p1 + p2;
      if constexpr (DET) qkf_turn_add(d, (long)2 * QKF_XSTEP, re, im, turn, tn);
      else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          __hip_atomic_fetch_add(d + r * 2 * QKF_XSTEP, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(d + r * 2 * QKF_XSTEP + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
    if (HAS1) {
      const v4d re = r1 + r2, im = r3 - r1 + r2;
      __attribute__((address_space(3))) double* const d1 = d + 2 * QKF_XBLOCK;  // 16 rows further down
      if constexpr (DET) qkf_turn_add(d1, (long)2 * QKF_XSTEP, re, im, QkfTurn{turn.at + nn, turn.idx, turn.broken, turn.gerr}, tn);  // (the counters of the next block of rows follow)
      else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          __hip_atomic_fetch_add(d1 + r * 2 * QKF_XSTEP, re[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(d1 + r * 2 * QKF_XSTEP + 1, im[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
    d += 2 * ps;  // the next panel
  }
}

template <bool FULL, bool HAS1, bool DET = false>
__device__ __forceinline__ void qkf_p2_dual(const QkfTile& t0, const QkfTile& t1, v2d (&fr)[4], v2d (&fs)[4], QkfStream cur, const int ps, const int nn, const int kmax, lds_v2d* xo, const int q,
                                            const int j, const QkfStream nxt, const bool nxt_p1, const unsigned n1, const QkfTurn turn = QkfTurn{nullptr, 0, nullptr, nullptr}) {
  if constexpr (DET) {
    qkf_p2_dual_turn<FULL, HAS1, DET>(t0, t1, fr, fs, cur, ps, nn, kmax, xo, q, j, nxt, nxt_p1, n1, turn);
    return;
  }
  lds_double* d = (lds_double*)(xo + q * TILE + j);
  lds_double* d1 = d + 2 * QKF_XBLOCK;  // the second tile's rows: 16 rows further down
  if constexpr (QKF_P2_FORM_DUAL != 0) {  // the one-sum block
    qkf_p2_blocks<FULL, HAS1, false>(t0, t1, fr, cur, 4, nxt, nn, kmax, d, 2 * QKF_XBLOCK, 2 * ps);
    return;
  }
  constexpr long rs = 2 * QKF_XSTEP;
  const v4d s0 = t0.re + t0.im, s1 = HAS1 ? t1.re + t1.im : s0;
  const v2d *const c0 = cur.base, *const c1 = cur.base + cur.step, *const c2 = cur.base + 2 * cur.step, *const c3 = cur.base + 3 * cur.step;
  unsigned off = cur.off;
#pragma unroll 1
  for (int tn = 0; tn + 1 < nn; ++tn) {
    off += TILE;
    qkf_p2_block<FULL, HAS1>(t0, t1, s0, s1, fr, kmax, c0, c1, c2, c3, off, d, d1, rs);
    d += 2 * ps, d1 += 2 * ps;  // the next panel
  }
  qkf_p2_block<FULL, HAS1>(t0, t1, s0, s1, fr, kmax, nxt.base, nxt.base + nxt.step, nxt.base + 2 * nxt.step, nxt.base + 3 * nxt.step, nxt.off, d, d1, rs);
}

template <int NW, int XCAP, int WPS, bool DET = false, int RCAP = XCAP>  // waves per workgroup (a round holds NW pairs of tiles); elements of the LDS X buffer as the segmentation sees it; waves per SIMD (register budget); ordered accumulation (bit-reproducible); elements the buffer really has (the residency of X)
__global__ __launch_bounds__(64 * NW, WPS) void qk_sweep_fused_dual_kernel(const SweepArgs g) {
  constexpr int NT = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) double lds_raw[];
  lds_v2d* const XL = (lds_v2d*)lds_raw;
  static_assert(RCAP >= XCAP && RCAP % QKF_XBLOCK == 0, "the buffer holds what the segmentation counts on, in whole blocks");
  long long* const slot = reinterpret_cast<long long*>(lds_raw + 2 * RCAP);
  const v2d* const xdata = reinterpret_cast<const v2d*>(g.xdata);
  const v2d* const ydata = reinterpret_cast<const v2d*>(g.ydata);
  v2d* const G0 = reinterpret_cast<v2d*>(g.scratch) + (long long)blockIdx.x * 2 * g.x_plane;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int ns = g.n_sites;
  __attribute__((address_space(3))) double* const zacc = (__attribute__((address_space(3))) double*)(slot + 2);  // [16 wavefronts][2]
  lds_v4i* const rec = (lds_v4i*)(slot + 2 + 32);  // per-site records as in qk_sweep_fused_kernel
  long long* const m_off = reinterpret_cast<long long*>(slot + 2 + 32) + 6 * (long long)ns;
  lds_int* const tbroken = (lds_int*)(m_off + 2 * (long long)ns);  // DET: the workgroup's sticky 'a wait ran out' flag, then
  lds_int* const turn0 = tbroken + 2;                              // two sets of g.turn_ints turn counters (qkf_turn_add)
  auto rfl = [&](const int v) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(v); };
  auto ldl = [&](const long long* p_) __attribute__((always_inline)) {
    const long long v = *p_;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
  };
  auto site = [&](const int k) __attribute__((always_inline)) {
    const v4i r0 = rec[3 * k], r1 = rec[3 * k + 1], r2 = rec[3 * k + 2];
    QkfSite s;
    s.a = rfl(r0.x), s.a2 = rfl(r0.y), s.b = rfl(r0.z), s.b2 = rfl(r0.w);
    s.at = rfl(r1.x), s.nks = rfl(r1.y), s.W = rfl(r1.z), s.flags = rfl(r1.w), s.small = (s.flags & QK_REC_SMALL) != 0, s.sw = (s.flags & QK_REC_SWITCH) != 0;
    s.inv = rfl(r2.x);
    s.ps = rfl(r2.y), s.pd = 1 << s.ps, s.next = rfl(r2.z);
    s.mt = s.a / TILE, s.nt = s.b2 / TILE, s.nn = s.a2 / TILE;
    s.Ak = xdata + ldl(m_off + 2 * k);
    s.Bk = ydata + ldl(m_off + 2 * k + 1);
    return s;
  };
  // pair `v` of a strip as (ta, tc = tp: column blocks 2 tp, 2 tp + 1 of the strip, p).  This kernel keeps the order with p fastest in BOTH
  // its forms (qk_unit_decode_ordered, qk_plan.h): with p slowest -- the order of the one-tile kernel, fewer operand blocks per round -- it
  // measured 2 % SLOWER on the headline set (lab/NOTES_r05.md), and fetching no padding did not pay here either
  auto pair_of = [&](const QkfSite& s, const int v) __attribute__((always_inline)) { return qk_unit_decode_ordered(v, s.ps, s.mt, s.inv); };
  // the streams of pair `v` of a strip starting at block s0 (column blocks s0 + 2 tp, + 1)
  auto b_stream = [&](const QkfSite& s, const int s0, const int v, const int half) __attribute__((always_inline)) {
    const QkUnit un = pair_of(s, v);
    return QkfStream{s.Bk + un.p * s.b2, (unsigned)((q * s.pd) * s.b2 + (s0 + 2 * un.tc + half) * TILE + j), 4 * s.pd * s.b2};
  };
  // What this wave does in the round that starts at unit r0 of a strip of w blocks with `units` pairs of tiles: pair r0 + wave
  // -- or, when the units left fill at most half of the waves, ONE tile of a pair (column block 2 tp or 2 tp + 1):
  // the last round of a site then takes half as long (a site of 4 x 4 tiles has 16 pairs: 12 + 4, i.e. 12 pairs + 8 tiles).
  struct Unit {
    bool mine, has1;
    int v, half;
  };
  auto unit_of = [&](const QkfSite& s, const int w, const int units, const int r0) __attribute__((always_inline)) {
    Unit un;
    const int left = units - r0;
    const bool halves = 2 * left <= NW;
    // (first tiles to waves 0 .. left - 1, second tiles to the next `left` waves: consecutive waves sit on different SIMDs)
    un.half = (halves && wave >= left) ? 1 : 0;
    un.v = r0 + wave - (un.half ? left : 0);
    const int tp = pair_of(s, un.v).tc;
    const bool second = 2 * tp + 1 < w;  // the pair has a second tile
    un.mine = un.v < units && (un.half == 0 || second);
    un.has1 = !halves && second;
    return un;
  };
  auto a_stream = [&](const QkfSite& s, const int v) __attribute__((always_inline)) {
    const QkUnit un = pair_of(s, v);
    return QkfStream{s.Ak + un.p * s.a2, (unsigned)(((un.ta * TILE + q) * s.pd) * s.a2 + j), 4 * s.pd * s.a2};
  };
  QKF_PROF_DECL();
  const int xcc = qk_xcc_id();
  int gang_round = 0;  // (gang start: this workgroup's pairs so far)
  if (tid == 0) qk_tail_start(g);
  // The queue is pulled ONE PAIR AHEAD (qkf_pull_next): the pair after the current one while the waves run the current pair's right edge,
  // its step table behind that edge's barrier -- the table of the pair that just ended is dead by then, so one table serves.  The two
  // words of `slot` alternate per pair.  A workgroup still never pulls a pair it does not run.  Against the loop of the one-tile kernel
  // (pull, barrier, read, barrier, table in front of every pair, a barrier behind it): the atomic's latency leaves the critical path and
  // two barriers per pair go.  60-qubit x 6-layer Gram, this launch: 292.2 -> 288.4 ms; the 8-wave launch of the one-tile kernel measured
  // 49.15 -> 48.90 ms, inside its noise margin, so that kernel keeps its loop (lab/NOTES_r06.md).
  if (tid == QKF_PULLER(NT)) qkf_pull_next(g, xcc, gang_round, slot);
  __syncthreads();
  long long p = slot[0];
  int psel = 0;  // the word of `slot` that holds p
  auto table_of = [&](const long long pp) __attribute__((always_inline)) {
    if (pp < 0) return;
    const int xi_ = g.pairs[2 * pp], yj_ = g.pairs[2 * pp + 1];
    qkf_step_table<XCAP, NT>(g, xi_, yj_, pp, rec, m_off, tid, QkSegRule{XCAP, NW, true, RCAP, QKF_RES_PARTIAL != 0});
  };
  table_of(p);
  while (p >= 0) {
    const int xi = g.pairs[2 * p], yj = g.pairs[2 * p + 1];
    // a unit is (ta, tp, p): pd mt ceil(nt / 2) pairs of tiles.  LDS-resident step: X and X' fit the buffer and ONE round holds
    // all pairs, or they fit side by side; otherwise X' is built in strips of W blocks of b', pairs in rounds of NW
    const int ek = g.edge_k, k_hi = ns - ek;  // the chain runs over the sites [ek, k_hi): the ends are in the edge blocks
    const bool edges = ek > 0;
    if (!edges)
      for (int e = tid; e < TILE * TILE; e += NT) XL[e] = (v2d){e == 0 ? 1.0 : 0.0, 0.0};
    if constexpr (DET)
      for (int e = tid; e < 2 * g.turn_ints + 2; e += NT) tbroken[e] = 0;
    int tsel = 0;  // DET: the set of turn counters in use (the other one is zeroed meanwhile for the next strip or step)
    __syncthreads();
    int cur = 0, xb = 0;
    if (edges) {  // X behind the left edge: one product of the two left blocks
      const v4i r0 = rec[3 * ek];
      const int a_e = rfl(r0.x), b_e = rfl(r0.z);  // (of a chain that starts in orientation 1: the record of the exchanged states)
      const bool o1 = !DET && (rfl(rec[3 * ek + 1].w) & QK_REC_ORIENT) != 0;  // (the ordered form runs orientation 0 throughout)
      qkf_edge_prefix<NW, QKF_EDGE_PAIRS(WPS), QKF_EDGE_SETS(WPS)>(g, o1 ? yj : xi, o1 ? xi : yj, a_e, b_e, XL, G0, a_e * b_e > XCAP, wave, q, j, o1);
      __syncthreads();
    }
    QKF_STAMP(0);  // pair set-up (queue, step table, left edge)
    QkfTile T0, T1;
    v2d fr[4], fs[4];     // the fragment registers of the wave's global streams (fs: the second column block of phase 1)
    bool primed = false;  // fr / fs hold the first group of the wave's next pair of tiles
    QkfSite sn = site(ek);
    for (int k = ek; k < k_hi;) {
      const QkfSite sc = sn;
      k = sc.next;  // (from here on: the entry of the NEXT step)
      if (k < k_hi) sn = site(k);
      const int a = sc.a, a2 = sc.a2, b = sc.b, mt = sc.mt, nt = sc.nt, W = sc.W;
      const bool small = sc.small;
      v2d* const Gc = G0 + (long long)cur * g.x_plane;
      v2d* const Gn = G0 + (long long)(cur ^ 1) * g.x_plane;
      // the residency of X (qk_plan.h: qk_resident), as in qk_sweep_fused_kernel: where X' is built, the panels [klo, khi) phase 1 reads from LDS
      const int n_out = sc.b2 * a2;
      const QkResident rs = qk_rec_resident(sc.flags, mt, n_out, RCAP, xb != 0);
      if (a * b <= XCAP && rs.khi - rs.klo < mt) {  // (X is in LDS exactly when it fits the segmentation's buffer) the panels that X' or its strips will overlap go to the global buffer
        const int e0 = (rs.klo == 0 ? rs.khi : 0) * (b * TILE), e1 = (rs.klo == 0 ? mt : rs.klo) * (b * TILE);
        for (int e = e0 + tid; e < e1; e += NT) Gc[e] = XL[xb + e];
        __syncthreads();
      }
      const unsigned xgm = qk_res_global_mask(rs);  // bit ta: the units of row block ta read their panel of X from Gc
      const bool pingpong = rs.kind == QK_RES_SIDE;
      const int ob = rs.ob;
      if (pingpong && !DET)
        for (int e = tid; e < n_out; e += NT) XL[ob + e] = (v2d){0.0, 0.0};
      QKF_STAMP(1);  // step set-up: record decode, X moved between LDS and the global buffer, X' zeroed (ping-pong)
      for (int s0 = 0; s0 < nt; s0 += W) {
        const int w = min(W, nt - s0), units = sc.pd * mt * ((w + 1) >> 1);
        lds_int* const tcur = turn0 + tsel * g.turn_ints;
        if constexpr (DET) {  // (ordered accumulation: the first contribution to a block stores, nothing is zeroed but the next set of counters)
          for (int e = tid; e < g.turn_ints; e += NT) turn0[(tsel ^ 1) * g.turn_ints + e] = 0;
        } else if (!small && !pingpong) {
          for (int e = tid; e < w * TILE * a2; e += NT) XL[ob + e] = (v2d){0.0, 0.0};
          QKF_STEP_BARRIER();
        }
        for (int r0 = 0; r0 < units; r0 += NW) {  // (LDS-resident sites: one round, or several when X and X' sit side by side)
          const Unit un = unit_of(sc, w, units, r0);
          const int v = un.v;
          const bool mine = un.mine, has1 = un.has1;
          const QkUnit pr = pair_of(sc, v);
          const int tp = pr.tc, ta = pr.ta;
          if (mine) {
            const QkfStream bs = b_stream(sc, s0, v, un.half), as = a_stream(sc, v);
            const unsigned xoff = (unsigned)(ta * (b * TILE) + q * TILE + j);
            if ((xgm >> ta) & 1u) {  // this unit's panel of X is in the global buffer
              if (has1) qkf_p1_dual<true>(T0, T1, fr, fs, primed, bs, (const v2d*)Gc, xoff, sc.nks, as);
              else qkf_p1_dual<false>(T0, T1, fr, fs, primed, bs, (const v2d*)Gc, xoff, sc.nks, as);
            } else {
              if (has1) qkf_p1_dual<true>(T0, T1, fr, fs, primed, bs, (const lds_v2d*)(XL + xb), xoff, sc.nks, as);
              else qkf_p1_dual<false>(T0, T1, fr, fs, primed, bs, (const lds_v2d*)(XL + xb), xoff, sc.nks, as);
            }
          }
          QKF_STAMP(2);  // phase 1
          if ((small || pingpong) && r0 == 0 && !(DET && pingpong)) {
            QKF_STEP_BARRIER();  // ping-pong: X' is zero everywhere; in place (one round): every wave has read X, it becomes X'
            if (!pingpong && !DET) {
              for (int e = tid; e < n_out; e += NT) XL[e] = (v2d){0.0, 0.0};
              QKF_STEP_BARRIER();
            }
          }
          QKF_STAMP(3);  // wait for the other waves' phase 1 (LDS-resident steps), zero X'
          if (mine) {
            const int kmax = min(4, (sc.at - ta * TILE + 3) >> 2);
            // what the wave does next: its unit of the next round of this strip, of the first round of the next strip, or of
            // the next site (strip 0, round 0) -- if it has one there
            QkfStream nxt = a_stream(sc, v);
            bool np1 = false;
            if (r0 + NW < units) {
              const Unit nu = unit_of(sc, w, units, r0 + NW);
              if (nu.mine) nxt = b_stream(sc, s0, nu.v, nu.half), np1 = true;
            } else if (s0 + W < nt) {
              const int w2 = min(W, nt - s0 - W);
              const Unit nu = unit_of(sc, w2, sc.pd * mt * ((w2 + 1) >> 1), 0);
              if (nu.mine) nxt = b_stream(sc, s0 + W, nu.v, nu.half), np1 = true;
            } else if (k < k_hi) {
              const int w2 = min(sn.W, sn.nt);
              const Unit nu = unit_of(sn, w2, sn.pd * sn.mt * ((w2 + 1) >> 1), 0);
              if (nu.mine) nxt = b_stream(sn, 0, nu.v, nu.half), np1 = true;
            }
            const unsigned nd1 = 0;
            lds_v2d* const xo = XL + ob + (2 * tp + un.half) * QKF_XBLOCK;
            // the turn counters of this block of rows and this contribution's place in their order
            const QkfTurn tp_turn{tcur + (2 * tp + un.half) * sc.nn, sc.pd * ta + pr.p, tbroken, g.err};
            if (!DET && sc.sw) {  // the step ends with a switch: the tiles of X'^H, to the panels 2 tp (+ half), + 1 of the other orientation (LDS-resident: w = nt)
              lds_double* const dsw = (lds_double*)(XL + ob + (2 * tp + un.half) * (a2 * TILE) + q * TILE + j);
              constexpr int FORM = QKF_P2_FORM_DUAL;
              if (FORM != 0 && kmax == 4) {
                if (has1) qkf_p2_switch<true, true, FORM>(T0, T1, fr, true, a_stream(sc, v), 4, sc.nn, 4, dsw, 2 * a2 * TILE, nxt);
                else qkf_p2_switch<true, false, FORM>(T0, T1, fr, true, a_stream(sc, v), 4, sc.nn, 4, dsw, 0, nxt);
              } else {
                if (has1) qkf_p2_switch<false, true, FORM>(T0, T1, fr, true, a_stream(sc, v), 4, sc.nn, kmax, dsw, 2 * a2 * TILE, nxt);
                else qkf_p2_switch<false, false, FORM>(T0, T1, fr, true, a_stream(sc, v), 4, sc.nn, kmax, dsw, 0, nxt);
              }
            } else if (has1) {
              if (kmax == 4) qkf_p2_dual<true, true, DET>(T0, T1, fr, fs, a_stream(sc, v), w * QKF_XBLOCK, sc.nn, 4, xo, q, j, nxt, np1, nd1, tp_turn);
              else qkf_p2_dual<false, true, DET>(T0, T1, fr, fs, a_stream(sc, v), w * QKF_XBLOCK, sc.nn, kmax, xo, q, j, nxt, np1, nd1, tp_turn);
            } else {
              if (kmax == 4) qkf_p2_dual<true, false, DET>(T0, T1, fr, fs, a_stream(sc, v), w * QKF_XBLOCK, sc.nn, 4, xo, q, j, nxt, np1, nd1, tp_turn);
              else qkf_p2_dual<false, false, DET>(T0, T1, fr, fs, a_stream(sc, v), w * QKF_XBLOCK, sc.nn, kmax, xo, q, j, nxt, np1, nd1, tp_turn);
            }
            primed = np1;
          }
          QKF_STAMP(4);  // phase 2
        }
        QKF_STEP_BARRIER();  // the strip of X' is complete
        tsel ^= 1;
        QKF_STAMP(5);  // wait for the other waves' phase 2
        if (!small && nt > W) {
          for (int tn = 0; tn < sc.nn; ++tn)  // (panel by panel: the strip's rows of a panel are contiguous in both buffers)
            for (int e = tid; e < w * QKF_XBLOCK; e += NT) Gn[(long long)tn * (sc.b2 * TILE) + s0 * QKF_XBLOCK + e] = XL[tn * w * QKF_XBLOCK + e];
          __syncthreads();
        }
      }
      if (nt > W) cur ^= 1, xb = 0;
      else xb = ob;
    }
    if (tid == QKF_PULLER(NT)) qkf_pull_next(g, xcc, gang_round, slot + (psel ^ 1));  // the next pair, while the other wavefronts run the right edge
    // the orientation the chain ends in: that of its last step (whose second site, if it is a merged one, carries the same flags), switched once more if that step switches
    const int fl_end = DET ? 0 : rfl(rec[3 * (k_hi - 1) + 1].w);
    const bool sw_end = (fl_end & QK_REC_SWITCH) != 0, o_end = ((fl_end & QK_REC_ORIENT) != 0) != sw_end;
    if (edges) {  // the overlap: X against the product of the two right blocks
      const v4i r0 = rec[3 * (k_hi - 1)];
      const int a_l = rfl(r0.y), b_l = rfl(r0.w), a_e = sw_end ? b_l : a_l, b_e = sw_end ? a_l : b_l;  // (the last record is in the last step's orientation)
      qkf_edge_suffix<NW, QKF_EDGE_PAIRS(WPS), QKF_EDGE_SETS(WPS)>(g, o_end ? yj : xi, o_end ? xi : yj, a_e, b_e, (const lds_v2d*)(XL + xb), (const v2d*)(G0 + (long long)cur * g.x_plane), a_e * b_e > XCAP, zacc, wave,
                                                                   q, j, o_end);
    }
    __syncthreads();  // the partial sums and the next pair's index are in LDS; nobody reads this pair's step table any more
    const long long pn = slot[psel ^ 1];
    if (tid == 0) {
      v2d zz = {0.0, 0.0};
      if (edges)
        for (int w_ = 0; w_ < NW; ++w_) zz.x += zacc[2 * w_], zz.y += zacc[2 * w_ + 1];
      else zz = (v2d)XL[xb];  // (a chain without edge blocks ends in a 16 x 16 block: in LDS)
      if (o_end) zz.y = -zz.y;  // a chain that ends in orientation 1 yields conj(z)
      g.values[p] = zz.x * zz.x + zz.y * zz.y;
      if (g.z) {
        g.z[2 * p] = zz.x;
        g.z[2 * p + 1] = zz.y;
      }
    }
    table_of(pn);  // (the barrier that opens the next pair publishes it)
    if (!edges) __syncthreads();  // thread 0 has read the result from X: the next pair's X_0 may now be written
    p = pn, psel ^= 1;
    QKF_STAMP(6);  // right edge, result, the next pair's step table
  }
  if (tid == 0) qk_tail_exit(g);
  QKF_PROF_FLUSH();
}

// split planes (re | im) of a set image -> interleaved complex (complex128 for double, complex64 for float), same offsets;
// one workgroup per (state, site)
template <typename T>
__global__ void qk_interleave_kernel(const T* __restrict__ src, T* __restrict__ dst, const int32_t* __restrict__ dims, const int64_t* __restrict__ offs,
                                     const int n_sites, const long long n_tensors) {
  typedef T v2 __attribute__((ext_vector_type(2)));
  for (long long t = blockIdx.x; t < n_tensors; t += gridDim.x) {
    const long long s = t / n_sites;
    const int k = (int)(t - s * n_sites);
    const long long plane = (long long)dims[s * (n_sites + 1) + k] * 2 * dims[s * (n_sites + 1) + k + 1];
    const T* re = src + offs[t];
    const T* im = re + plane;
    v2* d = reinterpret_cast<v2*>(dst + offs[t]);
    for (long long e = threadIdx.x; e < plane; e += blockDim.x) d[e] = (v2){re[e], im[e]};
  }
}

// ----------------------------------------------------------------------------------------
// Wave sweep for bonds <= 32 (fp64): ONE pair per wavefront, the whole chain in registers -- no barrier, no atomics, no
// scratch.  The generalisation of qk_sweep_wave_kernel (bonds <= 16, qk_ring.h) to 2 x 2 tiles: X is held as up to four
// A-operand tiles XA[tk][ta] (tk: block of b, ta: block of a).  Per site, for every block tb of b':
//     for each (ta, p):  T = sum_tk XA[tk][ta]^T B_k[tk rows, p, tb cols]          (one tile, 16 VGPRs, never stored)
//                        N[tn] += T^T conj(A_k[ta rows, p, tn cols])   for tn = 0, 1 (raw 3M accumulators)
//     XN[tb][tn] = combine(N[tn])                                                  (C layout = next site's XA[tk = tb][ta = tn])
// This is the regime of the 100-qubit x 10-layer config at gamma = 0.1 (bonds <= 27) and of the reference's own runs at
// gamma <= 0.5: most sites have one or two blocks per bond, so a multi-wave workgroup would leave most of its waves idle.
// What bounds it is the stream of site tensors (8 waves per CU, each reading its own pair): with plain loads right before
// use a wave has 4 KiB in flight and the launch sits at the latency of HBM (219 ms on that config).  So the fragments reach
// the wave through a private 12-KiB LDS ring filled by LDS-DMA two k-step groups ahead of the matrix instructions, the per-pair
// tables come through the scalar cache, and only the k-steps below the TRUE bond are fetched (191 -> 170 ms: the rows of zero
// padding are a third of the image at bonds around 20).
// ----------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void qkw_wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// NG > 0: the k-step groups (4 fragments of 1 KiB) reach the wave through a private LDS ring of NG groups filled by LDS-DMA,
// NG - 1 .. NG groups ahead of the matrix instructions (the fetch side walks the same loop nest as a small scalar state
// machine, across site boundaries).  NG = 0: plain loads into registers right before use (4 KiB in flight per wave).
// SRC = float: the set image is complex64 (interleaved), the arithmetic stays fp64 -- the sweep is bound by the bytes it
// streams, so single-precision STORAGE halves its time while the only error left is the rounding of the inputs.  A group
// is then 16 rows x 16 columns x 8 bytes = 2 KiB, fetched as one or two 1-KiB pieces (8 rows each, 16 bytes per lane).
template <int NG, typename SRC>
__global__ __launch_bounds__(64, 2) void qk_sweep_wave2_kernel(const SweepArgs g) {
  constexpr bool F32 = sizeof(SRC) == 4;
  static_assert(!F32 || NG > 0, "complex64 images go through the LDS ring");
  constexpr int ES = F32 ? 8 : 16;  // bytes of a complex element of the image (addresses below are byte addresses: pointers to a
                                    // vector of the template's scalar make hipcc drop the host-side stub of the kernel without a word)
  constexpr int GROUP = F32 ? 128 : 256;  // v2d-sized (16-byte) units of LDS per group
  __shared__ long long slot;
  __shared__ v2d ring[NG > 0 ? NG * GROUP : 1];
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  const int lane = threadIdx.x, j = lane & 15, q = lane >> 4;
  // this lane's byte address in slot 0: fragment 0 (k-step 0) of the group
  const unsigned ring_lds = (unsigned)(uintptr_t)(lds_ptr_t)ring + (F32 ? (unsigned)(q * 128 + j * 8) : (unsigned)lane * 16u);
  const int ns = g.n_sites, n1 = ns + 1;
  const char* const xdata = reinterpret_cast<const char*>(g.xdata);
  const char* const ydata = reinterpret_cast<const char*>(g.ydata);
  auto uni = [](const int v) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(v); };
  auto unil = [](const long long v) __attribute__((always_inline)) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
  };
  const int xcc = qk_xcc_id();
  if (lane == 0) qk_tail_start(g);
  for (;;) {
    if (lane == 0) slot = qk_pull(g, xcc);
    __syncthreads();
    const long long p = unil(slot);
    __syncthreads();
    if (p < 0) break;
    // per-pair tables through the scalar cache (wave-uniform addresses in the constant address space): a vector load
    // per site and table would put its whole latency in front of the site's first tensor load
    typedef const __attribute__((address_space(4))) int* sint_p;
    typedef const __attribute__((address_space(4))) int64_t* slong_p;
    const int xi = ((sint_p)g.pairs)[2 * p], yj = ((sint_p)g.pairs)[2 * p + 1];
    const sint_p xd = (sint_p)(g.xdims + (long long)xi * n1);
    const sint_p yd = (sint_p)(g.ydims + (long long)yj * n1);
    const sint_p xt = (sint_p)(g.xtrue + (long long)xi * n1);
    const sint_p yt = (sint_p)(g.ytrue + (long long)yj * n1);
    const slong_p xo = (slong_p)(g.xoffs + (long long)xi * ns);
    const slong_p yo = (slong_p)(g.yoffs + (long long)yj * ns);
    QkfTile XA[2][2], XN[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) XA[u][v].re = XA[u][v].im = XN[u][v].re = XN[u][v].im = (v4d){0, 0, 0, 0};
    XA[0][0].re[0] = (lane == 0) ? 1.0 : 0.0;  // X_0 = 1: A-operand element [k = 0][m = 0]
    // ---- fetch side (NG > 0): group order = for tb, ta, p: { P1 groups tk < kb, P2 groups tn < nn }, site after site.
    // Entering a site, lane g computes the descriptor of the site's group g (<= 32 groups): element offset in its tensor,
    // k-steps below the true bond, which tensor -- a dozen vector instructions for the whole site; fetching a group is then a
    // v_readlane and the LDS-DMAs, with no branch but "site finished".  (The first version walked the loop nest as nested
    // scalar ifs and picked the wait with a switch: ~250 scalar instructions and ~30 branches between two groups of 3-12
    // MFMAs -- the wave was bound by its own control code.)
    int f_k = 0, f_i = 0, f_n = 0, f_slot = 0, c_slot = 0;
    int f_a2 = 0, f_b2 = 0;
    const char* f_A = xdata;
    const char* f_B = ydata;
    int desc = 0;
    auto enter = [&]() __attribute__((always_inline)) {  // descriptors of site f_k
      // (pinned to scalar registers: left alone, the compiler folds the two true-bond loads and the per-lane select below into
      //  ONE per-lane vector load -- and the s_waitcnt vmcnt(0) behind it drains the LDS-DMAs in flight at every site)
      const int fa = xd[f_k], fb = yd[f_k], fat = __builtin_amdgcn_readfirstlane(xt[f_k]), fbt = __builtin_amdgcn_readfirstlane(yt[f_k]);
      f_a2 = xd[f_k + 1], f_b2 = yd[f_k + 1];
      f_A = xdata + (xo[f_k] >> 1) * ES, f_B = ydata + (yo[f_k] >> 1) * ES;
      const int kb = fb >> 4, nn = f_a2 >> 4, mt = fa >> 4, nt = f_b2 >> 4, gpb = kb + nn;
      const int inv = (gpb == 2) ? 32768 : (gpb == 3) ? 21846 : 16384;  // g / gpb == (g * inv) >> 16 for g < 64
      const int gi = lane, blk = (gi * inv) >> 16, h = gi - blk * gpb, pp = blk & 1, r = blk >> 1;
      const int ta = (mt == 2) ? (r & 1) : 0, tb = (mt == 2) ? (r >> 1) : r;
      const bool is_b = h < kb;
      const int off = is_b ? ((h * TILE) * 2 + pp) * f_b2 + tb * TILE : ((ta * TILE) * 2 + pp) * f_a2 + (h - kb) * TILE;
      const int cnt = is_b ? min(4, (fbt - h * TILE + 3) >> 2) : min(4, (fat - ta * TILE + 3) >> 2);
      desc = off | (cnt << 16) | ((is_b ? 1 : 0) << 20);
      f_n = nt * mt * 2 * gpb, f_i = 0;
    };
    // fetch the next group: its k-steps below the true bond (the rows above are zero padding: a third of the image at bonds
    // around 20); the pieces above are asked for again at the address of the last one needed -- an L1 hit, no fabric bytes --
    // so that every group is the same number of LDS-DMAs and the consumer's wait is a constant.
    auto issue = [&]() __attribute__((always_inline)) {
      if (f_k >= ns) return;
      const int d = __builtin_amdgcn_readlane(desc, f_i);
      const int off = d & 0xffff, cnt = (d >> 16) & 7;
      const bool is_b = (d >> 20) != 0;
      const int ld = is_b ? f_b2 : f_a2;
      const char* const base = (is_b ? f_B : f_A) + (long)off * ES;
      if constexpr (F32) {
        // piece p = rows 8 p .. 8 p + 7 (two k-steps): lane L brings the 16 bytes of columns 2 (L & 7), + 1 of row 8 p + (L >> 3)
        const char* const src = base + (((lane >> 3) * 2) * ld + (lane & 7) * 2) * ES;
        const int last = (cnt - 1) >> 1;
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) if (!(QKF_ABL & 16)) __builtin_amdgcn_global_load_lds(src + (min(pc, last) * 16 * ld) * ES, (lds_ptr_t)(ring + f_slot * GROUP + pc * 64), 16, 0, 0);
      } else {
        const char* const src = base + ((q * 2) * ld + j) * ES;
#pragma unroll
        for (int i = 0; i < 4; ++i) if (!(QKF_ABL & 16)) __builtin_amdgcn_global_load_lds(src + (min(i, cnt - 1) * 8 * ld) * ES, (lds_ptr_t)(ring + (f_slot * 4 + i) * 64), 16, 0, 0);
      }
      f_slot = (f_slot == NG - 1) ? 0 : f_slot + 1;
      if (++f_i == f_n) {
        if (++f_k < ns) enter();
      }
    };
    // the next group of the order above, as four fragments in registers (those above the true bond hold copies and are not used)
    auto take = [&](v2d(&f)[4]) __attribute__((always_inline)) {
      issue();
      if (f_k >= ns) qkw_wait_vmcnt<0>();  // the last groups of a chain: nothing more is fetched behind them
      else qkw_wait_vmcnt<(NG > 0 ? (F32 ? 2 : 4) * (NG - 1) : 0)>();
      // (read by hand: the compiler puts vmcnt(0) in front of every LDS read it can see next to an LDS-DMA)
      const unsigned at = ring_lds + (unsigned)c_slot * (unsigned)(GROUP * 16);
      if constexpr (F32) {  // k-step i of lane (q, j): row q + 4 i, column j of the 16 x 16 image (128-byte rows)
        double h[4];  // (two floats each)
        asm volatile("ds_read_b64 %0, %1" : "=v"(h[0]) : "v"(at));
        asm volatile("ds_read_b64 %0, %1 offset:512" : "=v"(h[1]) : "v"(at));
        asm volatile("ds_read_b64 %0, %1 offset:1024" : "=v"(h[2]) : "v"(at));
        asm volatile("ds_read_b64 %0, %1 offset:1536" : "=v"(h[3]) : "v"(at));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3])::"memory");
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long long bits = __double_as_longlong(h[i]);
          f[i] = (v2d){(double)__int_as_float((int)bits), (double)__int_as_float((int)(bits >> 32))};
        }
      } else if (QKF_ABL & 32) {
        asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) : "v"(at));
      } else {
        asm volatile("ds_read_b128 %0, %1" : "=v"(f[0]) : "v"(at));
        asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(f[1]) : "v"(at));
        asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(f[2]) : "v"(at));
        asm volatile("ds_read_b128 %0, %1 offset:3072" : "=v"(f[3]) : "v"(at));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3])::"memory");
      }
      c_slot = (c_slot == NG - 1) ? 0 : c_slot + 1;
    };
    if constexpr (NG > 0) {
      enter();
#pragma unroll
      for (int i = 0; i < NG - 1; ++i) issue();
    }
    // the tables of site k + 1 are fetched while site k is swept
    int a_nx = xd[0], b_nx = yd[0], a2_nx = xd[1], b2_nx = yd[1], at_nx = xt[0], bt_nx = yt[0];
    long long xo_nx = xo[0], yo_nx = yo[0];
    for (int k = 0; k < ns; ++k) {
      const int a = a_nx, a2 = a2_nx, b = b_nx, b2 = b2_nx, at = at_nx, bt = bt_nx;
      const v2d* const Ak = reinterpret_cast<const v2d*>(xdata) + (xo_nx >> 1);  // (the plain-load path: complex128 images only)
      const v2d* const Bk = reinterpret_cast<const v2d*>(ydata) + (yo_nx >> 1);
      {
        const int k1 = min(k + 1, ns - 1);
        a_nx = a2, b_nx = b2, a2_nx = xd[k1 + 1], b2_nx = yd[k1 + 1], at_nx = xt[k1], bt_nx = yt[k1];
        xo_nx = xo[k1], yo_nx = yo[k1];
      }
      const int mt = a >> 4, kb = b >> 4, nn = a2 >> 4, nt = b2 >> 4;  // blocks of a, b, a', b' (1 or 2 each)
#pragma unroll
      for (int tb = 0; tb < 2; ++tb) {
        if (tb < nt) {
          v4d n1a[2], n2a[2], n3a[2];  // raw accumulators of X'[tb][tn]
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) n1a[tn] = n2a[tn] = n3a[tn] = (v4d){0, 0, 0, 0};
#pragma unroll
          for (int ta = 0; ta < 2; ++ta) {
            if (ta < mt) {
              const int ka = min(4, (at - ta * TILE + 3) >> 2);  // k-steps of this block of a below the true bond
#pragma unroll
              for (int pp = 0; pp < 2; ++pp) {
                // ---- T = sum_tk XA[tk][ta]^T B[tk rows, pp, tb cols]
                v4d p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0};
#pragma unroll
                for (int tk = 0; tk < 2; ++tk) {
                  if (tk < kb) {
                    const int kk = min(4, (bt - tk * TILE + 3) >> 2);
                    const v2d* const bp = Bk + ((tk * TILE + q) * 2 + pp) * b2 + tb * TILE + j;
                    v2d f[4];
                    if constexpr (NG > 0) take(f);
                    else {
#pragma unroll
                      for (int i = 0; i < 4; ++i) f[i] = bp[i * 8 * b2];  // (rows up to the padded bond exist and are zero)
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                      if (i < kk) qkf_kstep<false>(p1, p2, p3, XA[tk][ta].re[i], XA[tk][ta].im[i], f[i].x, f[i].y);
                  }
                }
                QkfTile t;
                if (QKF_ABL & 64) t.re = p1, t.im = p3;
                else t.re = p1 - p2, t.im = p3 - p1 - p2;
                // ---- N[tn] += T^T conj(A[ta rows, pp, tn cols])
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                  if (tn < nn) {
                    const v2d* const ap = Ak + ((ta * TILE + q) * 2 + pp) * a2 + tn * TILE + j;
                    v2d f[4];
                    if constexpr (NG > 0) take(f);
                    else {
#pragma unroll
                      for (int i = 0; i < 4; ++i) f[i] = ap[i * 8 * a2];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                      if (i < ka) qkf_kstep<true>(n1a[tn], n2a[tn], n3a[tn], t.re[i], t.im[i], f[i].x, f[i].y);
                  }
                }
              }
            }
          }
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) XN[tb][tn].re = n1a[tn] + n2a[tn], XN[tb][tn].im = n3a[tn] - n1a[tn] + n2a[tn];
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) XA[u][v] = XN[u][v];
    }
    {
      // z = X_n[0][0] sits in lane 0; broadcast and stored by every lane (see qk_sweep_wave_kernel for why)
      const double re = __longlong_as_double(unil(__double_as_longlong(XA[0][0].re[0])));
      const double im = __longlong_as_double(unil(__double_as_longlong(XA[0][0].im[0])));
      g.values[p] = re * re + im * im;
      if (g.z) {
        g.z[2 * p] = re;
        g.z[2 * p + 1] = im;
      }
    }
  }
  if (lane == 0) qk_tail_exit(g);
}
