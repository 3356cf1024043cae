/*
 * qkgram.h -- C ABI of the MI355X (gfx950) quantum-kernel Gram engine.
 *
 * Drop-in boundary for ONE hot path of mmetcalf14/qml-cutensornet: filling
 *     K[j, i] = |<psi(x_i)|psi(y_j)>|^2
 * from matrix-product states.  Each entry point below names the reference
 * interface it replaces.  Short names:
 *     G = gpu_backend/kernel_state_ansatz.py     (reference, GPU backend)
 *     J = KernelPkg/src/KernelPkg.jl             (reference, CPU engine)
 *
 * Conventions
 *   - every function returns 0 on success, a negative QK_E* code otherwise;
 *     qk_last_error() gives a thread-local message.  No exception, callback or
 *     C++/torch type crosses this ABI: plain pointers and sizes only.
 *   - the library is batch-first: nothing here is called per Gram entry.
 *   - the caller owns host buffers; the library owns device memory behind
 *     opaque handles.  Calls on one context are serialised by the caller.
 *   - "device pointer" arguments are plain HIP device addresses (for example
 *     torch.Tensor.data_ptr()); work is enqueued on the context's stream.
 *   - there is NO CPU fallback: without a usable gfx950 device
 *     qk_ctx_create() fails and nothing else can be called.
 */
#ifndef QKGRAM_H
#define QKGRAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QK_OK 0
#define QK_EINVAL (-1)   /* bad argument / inconsistent shapes            */
#define QK_EDEVICE (-2)  /* HIP error (no device, launch/alloc failure)   */
#define QK_ENOMEM (-3)   /* host allocation failure                       */

/* host layout of one site tensor handed to qk_mps_set_create() */
#define QK_LAYOUT_LPR 0 /* [left bond][physical][right bond], C order */
#define QK_LAYOUT_LRP 1 /* [left bond][right bond][physical], C order */

/* flags of qk_plan_create() */
#define QK_PLAN_SYMMETRIC 1u /* Y is X: compute i <= j only, mirror on scatter (G:390-395) */
#define QK_PLAN_QUADS 2u     /* pairs in 2x2 blocks {i1,i2} x {j1,j2} of consecutive states: one workgroup sweeps a block in
                                lockstep (experimental: measured no faster than pairs on cfg4; such plans can be CREATED here but are
                                swept only by the lab library libqklab.so -- qk_gram_values of libqkgram.so returns QK_EINVAL).  The pair list then holds 4 entries per
                                block (a symmetric plan's diagonal blocks include one mirrored pair i > j, an odd set's last
                                block repeats its state): scatter handles both. */

#define QK_PLAN_ORIENT 4u    /* symmetric plans only: a pair {i, j} is listed as (i, j) or as (j, i), whichever order of contraction is
                                cheaper on the matrix cores (the sweep contracts the environment with the Y tensor first; which state
                                plays Y decides the padded tile counts).  |<x_i|x_j>| = |<x_j|x_i>|, so K is unchanged and the optional z
                                output is the overlap of the pair AS LISTED.  This is the host-side greedy choice of the contraction
                                order (north star; reference call site G:380). */

typedef struct qk_ctx qk_ctx;         /* one per device; replaces CuTensorNetHandle(device_id), G:213,255,366 */
typedef struct qk_mps_set qk_mps_set; /* a device-resident list of MPS; replaces the per-rank lists of
                                         pytket-cutensornet MPS objects mps_x_chunk / mps_y_chunk, G:210,252,290 */
typedef struct qk_plan qk_plan;       /* ordered list of (x, y) pairs assigned to one rank; replaces the chunk /
                                         round-robin bookkeeping of G:154,184,331-334,384-385 */

/* Algorithmic work of the last gram launch: complex128,
 * 8 real flops per complex multiply-add, each site tensor of both operands
 * read once per pair.  kernel_ms is the HIP-event time of the sweep kernel
 * on the context's stream (0 until the events have completed). */
typedef struct qk_stats {
  int64_t pairs;
  double flops;        /* sum over pairs and sites of 8*min(a*b*2*b' + 2*a*a'*b', a*b*2*a' + 2*b*a'*b'): the cheaper association per site */
  double padded_flops; /* the same with every bond rounded up to the MFMA tile (16)   */
  double bytes;        /* sum over pairs of 16*2*sum_k(a_k a_k+1 + b_k b_k+1) + 8     */
  double kernel_ms;    /* device time of the last sweep launch                        */
  int32_t grid;        /* workgroups launched                                         */
  int32_t max_bond;    /* largest padded bond among the two sets                      */
  int32_t kernel;      /* which sweep kernel ran: QK_KERNEL_* (see qk_kernel_name)    */
  int32_t precision;   /* 64 or 32: bits of a real of the sets it ran on              */
  /* A split sweep (sets of very different entanglement: the pairs whose sites all fit the site-fused kernel's smaller LDS
   * buffer are listed last and swept by its two-workgroups-per-CU shape, right after the launch named by `kernel`):
   * the second launch's share of the numbers above; all zero when the sweep was one launch. */
  int64_t second_pairs;
  double second_flops, second_padded_flops, second_bytes;
  double second_ms;     /* device time of the second launch (kernel_ms covers both)    */
  int32_t second_kernel; /* QK_KERNEL_FUSED2; QK_KERNEL_WAVE2 for a mixed set (its pairs of two small states); or QK_KERNEL_NONE */
  int32_t queues;        /* device work queues of the launch: 8 per class of pairs (one per XCD), 1 = one list */
  /* Tail accounting from device clocks (first workgroup start, first and last workgroup exit per launch): the share of a
   * launch's duration during which the chip was draining -- some workgroups had run out of work, the last one had not.
   * 0 for kernels that do not record it.  At a 1/8 share of the Gram the tails weigh eight times more than on one GPU.   */
  double tail_frac, second_tail_frac;
  /* Device time between the start of the call and the start of the sweep: the kernels that make a set's derived images
   * (interleaved image, edge blocks, merged steps) on the FIRST Gram of a set -- part of a cold Gram (the reference's
   * kernel_mat_time, G:322, 432-434, brackets set-up and tiles alike), ~0 afterwards.                                   */
  double derive_ms;
  /* Dynamic LDS bytes per workgroup of the launch and of the second launch (0: none).  A 12-wave site-fused launch asks for its X buffer
   * and the chain's tables behind it; the bytes tell the instantiation with the large X buffer (9728 elements) from the one with the
   * segmentation's (8192), which qk_kernel_name does not: both carry the name of the shape.                                          */
  int32_t lds_bytes, second_lds_bytes;
} qk_stats;

/* sweep kernels of qk_gram_values (qk_stats.kernel) */
#define QK_KERNEL_NONE 0
#define QK_KERNEL_WAVE 1    /* qk_sweep_wave_kernel: one pair per wavefront, bonds <= 16, fp64           */
#define QK_KERNEL_SMALL 2   /* qk_sweep_small_kernel: X, T in LDS, bonds <= 32                            */
#define QK_KERNEL_FUSED1 3  /* qk_sweep_fused_kernel<12, 2, 8192, 3, false>: site-fused sweep, one workgroup per CU, single tiles (QK_FUSED_DUAL=0) */
#define QK_KERNEL_FUSED2 4  /* qk_sweep_fused_kernel<8, 1, 4608, 4, false>: site-fused sweep, two workgroups per CU */
#define QK_KERNEL_RING 5    /* qk_sweep_ring_kernel: X, T in an L2-resident scratch                       */
#define QK_KERNEL_LAB 6     /* an experimental kernel (libqklab.so only)                                  */
#define QK_KERNEL_WAVE2 7   /* qk_sweep_wave2_kernel<3, double | float>: one pair per wavefront, bonds <= 32 (2 x 2 tiles), fp64 arithmetic on a complex128 or complex64 image */
#define QK_KERNEL_WAVE2_PLAIN 9 /* qk_sweep_wave2_kernel<0, double>: the same with plain loads instead of the LDS-DMA ring (QK_WAVE2=2) */
#define QK_KERNEL_FUSED_DUAL 8 /* qk_sweep_fused_dual_kernel<12, 8192, 3, false>: site-fused sweep, one workgroup per CU, pairs of tiles per wave (the default form of that shape) */
/* the DET forms of the three site-fused shapes (QK_DETERMINISTIC=1: contributions to X' added in a fixed order -- bit-reproducible Grams) */
#define QK_KERNEL_FUSED_DUAL_DET 10
#define QK_KERNEL_FUSED2_DET 11
#define QK_KERNEL_FUSED1_DET 12
/* the kernel's name as rocprofv3 prints it (without the "void " and the argument list) */
const char* qk_kernel_name(int32_t kernel, int32_t precision);

const char* qk_last_error(void);

/* number of gfx950 devices visible to the process (0 if none); replaces
 * cupy.cuda.runtime.getDeviceCount(), G:5,152 */
int qk_device_count(void);

/* ---- context --------------------------------------------------------------- */
int qk_ctx_create(int device_id, qk_ctx** out);
int qk_ctx_destroy(qk_ctx* ctx);
/* Run subsequent work on exactly this hipStream_t.  NULL is HIP's null (default) stream --
 * which is what torch.cuda.current_stream().cuda_stream returns for torch's default stream.
 * A new context starts on a private non-blocking stream; qk_ctx_use_own_stream() goes back to it. */
int qk_ctx_set_stream(qk_ctx* ctx, void* hip_stream);
int qk_ctx_use_own_stream(qk_ctx* ctx);
int qk_ctx_synchronize(qk_ctx* ctx);
/* Release the device memory a context keeps between calls: the sweep's per-workgroup scratch and the device builder's arena and
 * workspace (tens of GB at large bond caps; kept because allocating them costs seconds).  They come back on demand.          */
int qk_ctx_trim(qk_ctx* ctx);

/* ---- MPS sets ---------------------------------------------------------------
 * Upload n_states MPS of n_sites sites each.
 *   bond_dims    [n_states][n_sites+1] int32, bond_dims[s][0] = bond_dims[s][n_sites] = 1
 *   site_tensors [n_states][n_sites]   host pointers to complex128 (re,im interleaved)
 *                arrays of shape (chi_k, 2, chi_k+1) in `layout`
 * Replaces keeping pytket-cutensornet MPS objects (cupy tensors) alive on the
 * device between simulate() and vdot(), G:221-226, 290, 370-374.
 * Device layout: per site, split re/im planes [chi_k^][2][chi_k+1^] with every
 * bond zero-padded to a multiple of 16 (the f64 MFMA tile).                    */
int qk_mps_set_create(qk_ctx* ctx, int32_t n_states, int32_t n_sites, const int32_t* bond_dims,
                      const double* const* site_tensors, int32_t layout, qk_mps_set** out);
int qk_mps_set_destroy(qk_mps_set* set);
int qk_mps_set_info(const qk_mps_set* set, int32_t* n_states, int32_t* n_sites, int32_t* max_padded_bond,
                    int64_t* device_bytes);

/* ---- packed set images: the exchange format between ranks --------------------------------------------------
 * Replaces the pickled per-MPS sendrecv / send / recv of the reference's ring (G:341-352, 415-419): a rank packs
 * only ITS share of the states (qk_mps_set_create from host tensors, or qk_mps_set_from_built on the device), the
 * images are exchanged as flat buffers (one RCCL all-gather of the planes, the small tables beside it) and every rank
 * assembles the whole set with qk_mps_set_from_packed -- nothing is re-packed element by element, and with RCCL
 * nothing crosses PCIe.
 * qk_mps_set_image: the fp64 image of a set: *n_doubles doubles at *planes_dev (valid while the set lives); tables
 *   copied to dims_true[n_states][n_sites+1] and offsets[n_states][n_sites] (re-plane offsets in doubles); each may be NULL.
 * qk_mps_set_from_packed: a set of n_states states whose site tensors lie in the device buffer `planes_dev`
 *   (n_doubles doubles, copied device-to-device into memory the new set owns) at the given offsets, each in the
 *   padded split-plane layout of qk_mps_set_create (what qk_mps_set_image hands out).
 * qk_mps_set_copy_image: the planes copied into `dst` (n_doubles doubles; a device buffer -- for example the send
 *   buffer of the all-gather -- or a host buffer: the direction is inferred from the pointer).
 * In qk_mps_set_from_packed `planes` may likewise be a device or a host buffer.                                     */
int qk_mps_set_image(const qk_mps_set* set, int64_t* n_doubles, const double** planes_dev, int32_t* dims_true, int64_t* offsets);
int qk_mps_set_copy_image(const qk_mps_set* set, double* dst, int64_t n_doubles);
int qk_mps_set_from_packed(qk_ctx* ctx, int32_t n_states, int32_t n_sites, const int32_t* dims_true, const int64_t* offsets,
                           const double* planes_dev, int64_t n_doubles, qk_mps_set** out);

/* Precision of a set's device image: 64 (complex128 planes, what qk_mps_set_create builds) or 32.
 * qk_mps_set_to_f32 makes a complex64 copy on the device (same layout, same element offsets).  A sweep whose two
 * sets are fp32 runs on v_mfma_f32_16x16x4_f32 with fp32 X/T scratch; outputs stay double.  The reference never
 * leaves fp64 (G:141-144 does not set float_precision); this is SURVEY.md section 8f row N4, the fp32-vs-fp64
 * tolerance sweep its cfg5 asks for.  Mixing an fp32 and an fp64 set in one call is QK_EINVAL.                  */
int qk_mps_set_precision(const qk_mps_set* set);
int qk_mps_set_to_f32(qk_ctx* ctx, const qk_mps_set* src, qk_mps_set** out);

/* Host-only packing helper used by qk_mps_set_create (exported so that the
 * packing can be unit-tested without a GPU).  Writes one state's padded planar
 * image; `out` must hold qk_pack_state_size() doubles.                         */
int64_t qk_pack_state_size(int32_t n_sites, const int32_t* bond_dims);
int qk_pack_state(int32_t n_sites, const int32_t* bond_dims, const double* const* site_tensors, int32_t layout,
                  double* out, int64_t* site_offsets /* [n_sites] offsets of each re-plane, in doubles */);

/* ---- plans (host side; no GPU needed) ---------------------------------------
 * Enumerate the pairs of the Gram in tiles of `block` x `block` states (block <= 0:
 * one tile = the whole Gram), sort each tile by decreasing estimated cost, deal the
 * pairs to `world_size` ranks in serpentine order (0..W-1, W-1..0, ...: equal counts
 * +-1 and flops within a fraction of a percent) and keep rank `rank`'s share, itself
 * ordered heaviest first for the device-side work queue.  x_dims / y_dims are the bond_dims tables of the two sets
 * (y_dims = NULL with QK_PLAN_SYMMETRIC).  Pairs are (x index i, y index j);
 * the Gram entry is K[j][i]  (rows = Y, cols = X: G:387, J:106).               */
int qk_plan_create(int32_t n_sites, int32_t nx, const int32_t* x_dims, int32_t ny, const int32_t* y_dims,
                   uint32_t flags, int32_t world_size, int32_t rank, int32_t block, qk_plan** out);
int qk_plan_destroy(qk_plan* plan);
int64_t qk_plan_num_pairs(const qk_plan* plan);       /* this rank's pairs              */
int64_t qk_plan_total_pairs(const qk_plan* plan);     /* all ranks                      */
int64_t qk_plan_max_pairs_per_rank(const qk_plan* plan);
const int32_t* qk_plan_pairs(const qk_plan* plan);    /* [num_pairs][2] = (i, j), host  */
int qk_plan_stats(const qk_plan* plan, qk_stats* out); /* algorithmic flops/bytes of this rank's share */
/* Pairs [qk_plan_first_run, num_pairs) are the SECOND RUN of the list, swept by its own launch right behind the first:
 *   - a mixed set (states with every bond <= 32 next to larger ones, at least 64 pairs of two small states): those small-small
 *     pairs, for the one-pair-per-wavefront sweep -- kernel choice is per PAIR, one large state does not drag the rest along;
 *   - otherwise the pairs with >= QK_PLAN_SPLIT (environment, default 0.75) of their padded work in sites that fit the site-fused
 *     kernel's smaller LDS buffer, for its two-workgroups-per-CU shape.
 * == num_pairs when the plan holds (nearly) one class only: the launch then takes the two-workgroups-per-CU shape when >= 75 % of
 * the padded work sits in sites that fit its buffer AND >= 50 % in sites of at most the narrow size (QK_PLAN_FIT, 3072 elements of
 * X), the 12-wave dual shape otherwise (e.g. a set whose bonds were cut at 64: every site 4 x 4 tiles).                   */
int64_t qk_plan_first_run(const qk_plan* plan);
/* XCD-aware work queues (default plans; QK_PLAN_XCD=0 in the environment or an explicit `block` gives the flat cost-ordered
 * list).  The states are sorted by weight, the Gram is cut into tiles of QK_PLAN_TILE x QK_PLAN_TILE (default 8 x 8) pairs in
 * that order -- the pairs of a tile share their x and y states and cost about the same --, the tiles are dealt heaviest
 * first to the least loaded rank and, per run of this rank's list, to 8 queues: queue s of the first run = pairs
 * [qstart[s], qstart[s+1]), s = 0..7, of the second run s = 8..15 (qstart[8] = qk_plan_first_run, qstart[16] = num_pairs).
 * On the device a workgroup reads the id of the XCD it runs on (8 XCDs with a private 4 MiB L2 each) and drains that queue
 * first, then steals from the others: the workgroups that share an L2 stream the same few states.  Replaces the chunk
 * bookkeeping of G:154, 331-334, 384-385 like the rest of the plan.  Returns the number of queues (16, or 1 for a flat
 * list: then qstart[0] = 0 and qstart[1..16] = num_pairs); qstart may be NULL.                                            */
int qk_plan_queues(const qk_plan* plan, int64_t* qstart /* [17] */);
/* EDGE BLOCKS: how many sites at either end of the chain the site-fused sweep takes from per-state blocks instead of walking
 * them (0: none).  While the bonds still grow like 2^k, contracting the first k sites of each state across their physical legs
 * into one matrix L[s][a] and starting a pair's environment as X = Ly^T conj(Lx) -- one product with K = 2^k -- is cheaper than k
 * sites of the chain and saves their per-site costs; likewise at the right end, where the overlap is sum X . (Ry^T conj(Rx)).
 * The planner picks the k (4..9) that minimises a cost model over a sample of the pairs (qkgram.hip: choose_edge_k; QK_EDGE=0
 * disables, QK_EDGE=k forces); the blocks are made once per set on first use (2^k x padded bond complex numbers per state and
 * end; counted by qk_mps_set_info).  This is the host-side choice of the contraction order at the ends of the chain (north star;
 * reference call site G:380); the algorithmic flop count of qk_stats does not change.                                        */
int32_t qk_plan_edge_sites(const qk_plan* plan);
/* The plans of ALL world_size ranks from one cost pass (a one-process communicator, qk_gram_sharded: pricing the Gram's pairs and
 * dealing its tiles is the same work for every rank and is done once; each rank then prices only its own share).  out[world_size];
 * plan r equals what qk_plan_create(..., world_size, r, 0, ...) returns.  Replaces G:154, 331-334 like qk_plan_create.      */
int qk_plan_create_all(int32_t n_sites, int32_t nx, const int32_t* x_dims, int32_t ny, const int32_t* y_dims,
                       uint32_t flags, int32_t world_size, qk_plan** out);
/* What the plan cost and what it could save.  plan_ms = host wall time of qk_plan_create for this plan (the reference's
 * kernel_mat_time, G:322, 432-434, brackets the set-up of the tiling phase too: the planner is on the cold path of every Gram),
 * threads = host threads it used, tile_reuse_bytes = the bytes of this rank's share if every state were read once per plan
 * tile (8 x 8 pairs) it takes part in -- the tile-reuse lower bound of SURVEY 8d, beside qk_stats.bytes (every state read
 * once per PAIR).  Any out pointer may be NULL.                                                                          */
int qk_plan_cost(const qk_plan* plan, double* plan_ms, int32_t* threads, double* tile_reuse_bytes);
/* MERGED STEPS (no entry point: part of qk_gram_values; QK_MERGE=0 disables, 1 = the fixed pairs only, 2 = default).  Between the edge
 * blocks the site-fused sweep may walk two neighbouring sites as ONE step: the set holds, beside its plain image, neighbouring sites of
 * the chain contracted in twos over the true bond between them (tensors [l][4][r], one per start site, made once per set on first use
 * and counted by qk_mps_set_info; QK_MERGE=1, or a device too full for it: the even starts k + 2 t only).  Which steps of a pair are
 * merged is decided once per plan, sets and launch shape by a small kernel on the sweep's stream (csrc/qk_plan.h: qk_segment_chain), a
 * mask of 128 bits per pair that the plan keeps: a merge is admissible where it keeps an LDS-resident step in the LDS and costs no more
 * padded work than the two sites; among the admissible segmentations the one with the fewest executed matrix instructions plus a fixed
 * price per step is taken (QK_MERGE=1: every admissible merge of the fixed pairs (k + 2 t, k + 2 t + 1)).  A merged step neither pads
 * its middle bond to 16 nor walks it, and saves the barriers, set-ups and stream turn-arounds of a step; again a host-prepared choice of
 * the contraction order (reference call site G:380).  qk_stats' algorithmic flops and bytes stay those of the plain chain.
 * THE ASSOCIATION OF A STEP (QK_ASSOC=0 disables, 1 = default; with QK_MERGE=2): the same programme also chooses, per step, whether the
 * step contracts the y tensor first (T = X^T B, X' = T^T conj(A)) or, with the two states exchanged, the x tensor first on W = X^H; a
 * second mask of 128 bits per pair holds the choice.  A step may end with a switch only where it is LDS-resident (its phase 2 then leaves
 * X'^H), at QK_SWITCH_PRICE matrix instructions' worth.  Results are those of the plain chain; QK_DETERMINISTIC=1 keeps "y first".   */

/* ---- the hot path -----------------------------------------------------------
 * qk_gram_values: for every pair p of the plan compute z_p = <x_i|y_j> and write
 *     values_dev[p] = |z_p|^2                 (G:380-383, J:106)
 *     z_dev[2p], z_dev[2p+1] = re, im of z_p  (optional, may be NULL)
 * One persistent launch; returns after enqueueing (asynchronous).
 * yset = NULL means Y is X.
 * The sweep kernel is chosen from the two sets' largest padded bond and precision:
 *   16, fp64            one pair per wavefront, entirely in registers (qk_sweep_wave_kernel);
 *   <= 32, fp64         one pair per wavefront with 2 x 2 register tiles, fed through a per-wave LDS-DMA ring
 *                       (qk_sweep_wave2_kernel<3, double>);
 *   <= 32, complex64    the SAME kernel on the complex64 image: single-precision storage, fp64 arithmetic
 *                       (qk_sweep_wave2_kernel<3, float>); with QK_WAVE2=0 | 2 the LDS-resident small-bond sweep in
 *                       complex64 arithmetic on the fp32 matrix cores (qk_sweep_small_kernel<float>);
 *   larger, fp64        the site-fused sweep (X in LDS, T in registers, qk_fused.h), bonds up to 512;
 *   larger, complex64   and fp64 bonds > 512: the ring sweep (X / T in an L2-resident scratch; complex64 arithmetic on
 *                       the fp32 matrix cores for complex64 sets).
 * All compute the same chain of complex GEMMs on the matrix cores and agree to rounding (tests/test_gpu_parity.py);
 * QK_WAVE=0 / QK_WAVE2=0 / QK_SMALL=0 / QK_FUSED=0 in the environment fall back to the next more general one, QK_FUSED=2
 * uses the fused sweep from bond 17, QK_FUSED_WGS=1|2 fixes its workgroups per CU.                                   */
int qk_gram_values(qk_ctx* ctx, const qk_mps_set* xset, const qk_mps_set* yset, const qk_plan* plan,
                   double* values_dev, double* z_dev);

/* Synchronous form for host communicators (mpi4py, gloo): the same sweep, values copied back
 * into values_host[num_pairs] (and z_host[2*num_pairs] unless NULL) before returning.        */
int qk_gram_values_host(qk_ctx* ctx, const qk_mps_set* xset, const qk_mps_set* yset, const qk_plan* plan,
                        double* values_host, double* z_host);

/* Scatter packed values into the dense matrix K (device, row-major, leading
 * dimension ld): K[j][i] = v, and K[i][j] = v as well when `mirror` != 0
 * (G:387, 390-395).  pairs_dev: [n][2] int32 on the device.                    */
int qk_scatter(qk_ctx* ctx, const int32_t* pairs_dev, const double* values_dev, int64_t n, double* k_dev,
               int64_t ld, int32_t mirror);

/* Convenience, synchronous: whole Gram of xset (cols) vs yset (rows, NULL =
 * symmetric) into a host matrix out[ny][ld].  Replaces the double loop
 * G:372-400 plus the final reduce G:428 for a single process.                  */
int qk_gram_host(qk_ctx* ctx, const qk_mps_set* xset, const qk_mps_set* yset, double* out, int64_t ld);

/* Convenience, synchronous: complex overlaps z[j][i] = <x_i|y_j> (re,im
 * interleaved, out[ny][nx][2]); the batched form of MPS.vdot, G:380.           */
int qk_overlaps_host(qk_ctx* ctx, const qk_mps_set* xset, const qk_mps_set* yset, double* out);

int qk_get_stats(qk_ctx* ctx, qk_stats* out);

/* ---- projected quantum kernel (Huang et al., Nat. Commun. 12, 2631 (2021)) ----------------------------------------------
 * Local Bloch vectors of every state of a set, synchronous on the context's stream.  Site k is qubit k, physical index 0 = |0>;
 * states need not be normalised:
 *     rho_k[s][s'] = sum over all other sites of psi(..s..) conj(psi(..s'..)) / <psi|psi>
 *     out[state][k] = (<X_k>, <Y_k>, <Z_k>) = (2 Re rho_k[0][1], -2 Im rho_k[0][1], rho_k[0][0] - rho_k[1][1])
 *     norms[state]  = <psi|psi> from the same sweep (norms may be NULL)
 * One environment sweep per state (left environments and those of the reversed chain), spread over the chip; every
 * state's result is bit-identical whatever the rest of the set and from run to run.  fp64 sets only (a complex64 set is
 * QK_EINVAL).  Device scratch is kept on the context (qk_ctx_trim releases it), bounded by a quarter of the free memory;
 * the Gram statistics (qk_get_stats) are not touched.                                                                     */
int qk_local_paulis_host(qk_ctx* ctx, const qk_mps_set* set, double* out /* [n_states][n_sites][3] */,
                         double* norms /* [n_states], may be NULL */);

/* The projected-kernel Gram from Bloch vectors (host arrays [n][n_sites][3]), synchronous:
 *     out[j * ld + i] = exp(-g/2 * sum_k sum_c (fx[i][k][c] - fy[j][k][c])^2)  = exp(-g sum_k ||rho_k(x_i) - rho_k(y_j)||_F^2)
 * Rows are Y, columns are X (as qk_gram_host); fy = NULL means Y is X (then ny must equal nx).  Each entry is summed over the
 * 3 n_sites terms in one fixed order: a symmetric Gram is exactly symmetric with a diagonal of exactly 1.0.
 * QK_EINVAL: g <= 0 or not finite, ld < nx, n_sites < 1, nx or ny < 1.                                                       */
int qk_projected_gram_host(qk_ctx* ctx, int32_t n_sites, int32_t nx, const double* fx /* [nx][n_sites][3] */,
                           int32_t ny, const double* fy /* NULL: Y is X */, double g, double* out, int64_t ld);

/* Pauli correlators of neighbouring qubits: the two-qubit reduced density matrices of the pairs (k, k+1), k = 0 .. n_sites - 2,
 * of every state of a set, synchronous on the context's stream.  P_0..P_3 = I, X, Y, Z:
 *     rho_{k,k+1}[(s,t)][(s',t')] = sum over all other sites of psi(..s,t..) conj(psi(..s',t'..)) / <psi|psi>
 *     out2[state][k][p][q] = <P_p on k, P_q on k+1> = sum rho_{k,k+1}[(s,t)][(s',t')] P_p[s'][s] P_q[t'][t]      (real)
 * so rho_{k,k+1} = 1/4 sum_{p,q} out2[k][p][q] P_p (x) P_q.  out2[k][0][0] is exactly 1.0; out2[k][p][0] and out2[k][0][q] are the
 * Bloch vectors of qubits k and k+1 (to rounding).  out1 and norms, when given, are what qk_local_paulis_host returns for the same
 * set, bit for bit: the sweep is that call's with two more GEMMs per site (the open right environment of site k+1), and shares its
 * guarantees -- every state's result is bit-identical whatever the rest of the set and from run to run.  fp64 sets only (a complex64
 * set is QK_EINVAL); n_sites < 2 is QK_EINVAL.  Device scratch as qk_local_paulis_host (26 instead of 14 P^2 doubles per state).  */
int qk_local_pair_paulis_host(qk_ctx* ctx, const qk_mps_set* set, double* out2 /* [n_states][n_sites-1][4][4] */,
                              double* out1 /* [n_states][n_sites][3], may be NULL */, double* norms /* [n_states], may be NULL */);

/* The two-qubit projected-kernel Gram from Pauli correlators (host arrays [n][n_sites-1][4][4]), synchronous:
 *     out[j * ld + i] = exp(-g/4 * sum_k sum_{p,q} (tx[i][k][p][q] - ty[j][k][p][q])^2)
 *                     = exp(-g sum_k ||rho_{k,k+1}(x_i) - rho_{k,k+1}(y_j)||_F^2)
 * Rows, columns, ty = NULL, the fixed summation order (exact symmetry, unit diagonal) and the argument errors are those of
 * qk_projected_gram_host, except that n_sites < 2 is QK_EINVAL.                                                              */
int qk_projected_pair_gram_host(qk_ctx* ctx, int32_t n_sites, int32_t nx, const double* tx /* [nx][n_sites-1][4][4] */,
                                int32_t ny, const double* ty /* NULL: Y is X */, double g, double* out, int64_t ld);

/* Pauli correlators of every pair of qubits up to distance max_dist = D, 1 <= D <= n_sites - 1: the pairs (k, k+d), d = 1 .. D,
 * k = 0 .. n_sites - 1 - d, listed distance-major,
 *     index(d, k) = sum_{e=1}^{d-1} (n_sites - e) + k,      n_pairs = D n_sites - D (D + 1) / 2
 *     out2[state][index(d, k)][p][q] = <P_p on k, P_q on k+d>                    (out2[..][0][0] is exactly 1.0)
 * with rho_{k,k+d} defined as rho_{k,k+1} above.  It is the neighbour sweep plus, per site, the four open left environments of each
 * of the last D - 1 qubits carried one site further (two GEMM launches for all of them) and one more reduction launch.  The
 * neighbour launches are untouched: out2[state][0 .. n_sites - 2] equals qk_local_pair_paulis_host's output bit for bit for every D,
 * out1 and norms equal qk_local_paulis_host's, D = 1 is qk_local_pair_paulis_host, and every state's result is bit-identical
 * whatever the rest of the set and from run to run.  QK_EINVAL when max_dist < 1 or max_dist > n_sites - 1; the other argument
 * errors are qk_local_pair_paulis_host's.  Device scratch: 26 + 24 (D - 1) P^2 doubles per state (the window of D - 1 live qubits,
 * 8 P^2 each, and the intermediates of their step, 16 P^2 each), counted by the batching rule and released by qk_ctx_trim.     */
int qk_local_pair_paulis_dist_host(qk_ctx* ctx, const qk_mps_set* set, int32_t max_dist, double* out2 /* [n_states][n_pairs][4][4] */,
                                   double* out1 /* [n_states][n_sites][3], may be NULL */, double* norms /* [n_states], may be NULL */);

/* The two-qubit projected-kernel Gram over the pairs up to distance max_dist (host arrays [n][n_pairs][4][4]), synchronous:
 *     out[j * ld + i] = exp(-g/4 * sum_pairs sum_{p,q} (tx[i][pair][p][q] - ty[j][pair][p][q])^2)
 *                     = exp(-g sum_pairs ||rho_pair(x_i) - rho_pair(y_j)||_F^2)
 * As qk_projected_pair_gram_host (max_dist = 1 is that call, bit for bit); QK_EINVAL also when max_dist < 1 or
 * max_dist > n_sites - 1.                                                                                                     */
int qk_projected_pair_gram_dist_host(qk_ctx* ctx, int32_t n_sites, int32_t max_dist, int32_t nx, const double* tx /* [nx][n_pairs][4][4] */,
                                     int32_t ny, const double* ty /* NULL: Y is X */, double g, double* out, int64_t ld);

/* Expectation values of Pauli strings for every state of a set, synchronous on the context's stream.  P_0..P_3 = I, X, Y, Z; a
 * string is c[0 .. n_sites - 1] with codes 0..3 (site k = qubit k, physical index 0 = |0>; the states need not be normalised):
 *     out[state][m] = <psi| P_c[0] (x) ... (x) P_c[n-1] |psi> / <psi|psi>                                        (real)
 *                   = sum psi(..s_k..) conj(psi(..s'_k..)) prod_k P_c[k][s'_k][s_k] / <psi|psi>
 * the convention of out2[k][p][q] above.  The support of a string is [a, b], its first and last non-identity sites: the left
 * environment L_a, one closed transfer step per site of [a, b] with the Pauli on the ket index (two GEMMs, as one step of the
 * sweep, and an elementwise pass where the site is not I), and one reduction against the right environment R_{b+1}.  A string
 * costs work on its support only; every L_k and R_k of a state is made once per call.  An all-identity string is written as
 * exactly 1.0; duplicates are allowed.  n_sites = 1 is valid.  norms, when given, are the bits qk_local_paulis_host returns.
 * The value of a (state, string) is the same bits whatever the other states of the set, the other strings of the call and their
 * order, however the call was cut into batches, and from run to run.  Agreement with qk_local_paulis_host and the pair
 * correlators is to rounding.
 * Device scratch: per state the sweep's planes and every L_k and R_k, and 6 P^2 doubles per (state, string) of a batch (P = the
 * state's largest padded bond), counted by the batching rule of qk_local_paulis_host (the strings of a state go in several
 * batches when they do not fit) and released by qk_ctx_trim.  QK_STRINGS_BATCH=<k> (read per call) caps the (state, string)
 * chains of a batch at k.
 * QK_EINVAL: a null ctx, set, strings or out; a set of another context; a complex64 set; n_strings < 1; a code above 3.       */
int qk_pauli_strings_host(qk_ctx* ctx, const qk_mps_set* set, int32_t n_strings,
                          const uint8_t* strings /* [n_strings][n_sites], codes 0..3 = I, X, Y, Z */,
                          double* out /* [n_states][n_strings] */, double* norms /* [n_states], may be NULL */);

/* Expectation values of strings of single-site operators for every state of a set, synchronous on the context's stream: the
 * Pauli strings above with any 2 x 2 complex matrix at a site.  The call brings a table of n_ops operators, 1 <= n_ops <= 255,
 * ops[c - 1][s'][s] = (Re, Im) of <s'| O_c |s> for the code c = 1 .. n_ops; code 0 is the identity and costs no work.  A string
 * is c[0 .. n_sites - 1] (site k = qubit k, physical index 0 = |0>; the states need not be normalised):
 *     out[state][m] = <psi| O_c[0] (x) ... (x) O_c[n-1] |psi> / <psi|psi>                                     (complex: Re, Im)
 *                   = sum psi(..s_k..) conj(psi(..s'_k..)) prod_k O_c[k][s'_k][s_k] / <psi|psi>
 * With the table (X, Y, Z) it is qk_pauli_strings_host's value, to rounding, and an imaginary part of rounding size; with
 * projectors it is the probability of an outcome on the measured qubits, the others traced out (the real part; a probability
 * of exactly 0 may come out as rounding noise of either sign).  The operators need not be Hermitian or unitary.  The chain is
 * that of the Pauli strings: L_a, per site of the support [a, b] the two GEMMs of a transfer step and, where the code is not 0,
 * an elementwise pass T'[(a, s')] = sum_s O[s'][s] T[(a, s)], then the complex sum of E_{b+1} R_{b+1}.  A string costs work on
 * its support only, whatever its operators: the cost of a Pauli string of the same support.  An all-identity string is written
 * as exactly (1.0, 0.0); duplicates are allowed.  n_sites = 1 is valid.  norms, when given, are the bits qk_local_paulis_host
 * returns.  The value of a (state, string) is the same bits whatever the other states of the set, the other strings of the
 * call and their order, the other operators of the table, however the call was cut into batches, and from run to run.
 * Device scratch, batching and qk_ctx_trim are those of qk_pauli_strings_host (a chain's chunk sums are two doubles wide);
 * QK_OPSTR_BATCH=<k> (read per call) caps the (state, string) chains of a batch at k.
 * QK_EINVAL: a null ctx, set, ops, strings or out; a set of another context; a complex64 set; n_strings < 1; n_ops outside
 * 1 .. 255; a table entry that is not finite (the message names the operator and the position); a code above n_ops (the message
 * names the string and the site); QK_OPSTR_BATCH < 1.  QK_EDEVICE: a state of norm 0 (the message names the state).          */
int qk_operator_strings_host(qk_ctx* ctx, const qk_mps_set* set, int32_t n_ops, const double* ops /* [n_ops][2][2][2] re, im */,
                             int32_t n_strings, const uint8_t* strings /* [n_strings][n_sites], codes 0 .. n_ops */,
                             double* out /* [n_states][n_strings][2] */, double* norms /* [n_states], may be NULL */);

/* Expectation values of matrix-product operators (sums of operator strings) for every state of a set, synchronous on the
 * context's stream.  MPO m is n_sites tensors W_k of bonds[m][k] x bonds[m][k + 1] blocks of 2 x 2 complex matrices,
 * W_k[u][v][s'][s] = (Re, Im) of <s'| . |s> (site k = qubit k, physical index 0 = |0>), bonds[m][0] = bonds[m][n_sites] = 1 and
 * every bond in 1 .. 32; the tensors are packed MPO-major, then site-major, then [u][v][s'][s][re, im].  With
 * H_m = sum_{u_1 .. u_{n-1}} (x)_k W_k[u_k][u_{k+1}], which need not be Hermitian,
 *     out[state][m] = <psi| H_m |psi> / <psi|psi>                                                           (complex: Re, Im)
 * in the conventions of qk_operator_strings_host (general-gauge and unnormalised states).  The support [a, b] of an MPO is the
 * hull of the sites whose tensor is not exactly the 1 x 1 identity; its chain starts from L_a and closes with R_{b+1}.  Per site
 * of the support: one GEMM over the w_k planes of the environment stacked along M, an elementwise mix of the planes by W_k, and
 * one GEMM launch that contracts every new plane with the conjugated site -- about w times the cost of one string over the
 * support, whatever the number of terms.  Per (MPO, site) the host lists the blocks (u, v) whose four entries are not all exactly
 * zero, by v then u; a zero block costs nothing and adds nothing, and the sum of an element runs over the listed blocks in
 * ascending u, s = 0 before s = 1, the imaginary factor before the real one, each component one chain of fused multiply-adds.
 * A site inside the support whose tensor is the exact 1 x 1 identity has no mix.  A bond-1 MPO gives the bits of its operator
 * string; an MPO whose tensors are all the 1 x 1 identity is written as exactly (1.0, 0.0); scaling one tensor by 2 scales the
 * value by 2 bit for bit.  norms, when given, are the bits qk_local_paulis_host returns.  The value of a (state, MPO) is the same
 * bits whatever the other states of the set, the other MPOs of the call and their order, however the call was cut into batches,
 * and from run to run.  A chain's slot is 10 w P^2 doubles (w = the MPO's largest bond, P = the state's largest padded bond);
 * device scratch, batching and qk_ctx_trim are those of qk_pauli_strings_host; QK_MPO_BATCH=<k> (read per call) caps the
 * (state, MPO) chains of a batch at k.
 * QK_EINVAL: a null ctx, set, bonds, tensors or out; a set of another context; a complex64 set; n_mpos < 1; a bond outside
 * 1 .. 32 (the message names the MPO and the cut); bonds[m][0] or bonds[m][n_sites] not 1; a tensor entry that is not finite (the
 * message names the MPO, the site and the indices); QK_MPO_BATCH < 1.  QK_EDEVICE: a state of norm 0 (the message names the
 * state).                                                                                                                    */
int qk_mpo_expectations_host(qk_ctx* ctx, const qk_mps_set* set, int32_t n_mpos, const int32_t* bonds /* [n_mpos][n_sites + 1] */,
                             const double* tensors /* MPO-major, site-major: [w_k][w_{k+1}][2][2][2] (re, im), packed */,
                             double* out /* [n_states][n_mpos][2] */, double* norms /* [n_states], may be NULL */);

/* A new set O|psi> of one matrix-product operator and every state of an fp64 set, synchronous on the context's stream.  The MPO is
 * given in the conventions and packing of qk_mpo_expectations_host (one MPO: bonds[n_sites + 1], tensors site-major).  With the
 * source's site tensors A_k[a][s][b] of true bonds chi_k, the product has true bonds w_k chi_k and the sites
 *     B_k[(u, a)][s'][(v, b)] = sum_s W_k[u][v][s'][s] A_k[a][s][b],     row u chi_k + a, column v chi_{k+1} + b
 * in the padded split-plane layout of qk_mps_set_create (every new bond padded to a multiple of 16, states and sites in order), in a
 * set that owns its memory.  Expression order: an element is the sum over s = 0 before s = 1 of its block (u, v), the imaginary
 * factor before the real one, each real component one chain of fused multiply-adds that starts with a plain product -- the
 * expression of one block of qk_mpo_expectations_host's mix.  A block (u, v) whose four entries are all exactly zero is not read
 * and gives exact zeros, also against a NaN in the source; padding rows and columns are zero.  The kernel writes the zeros: there is
 * no memset, and every double of the new image is written by this call, once.  A site whose W_k is the exact 1 x 1 identity is
 * copied bit for bit, so an MPO of such sites gives an image bit-equal to qk_mps_set_copy_image of a source in that layout.  The
 * result records no centre (qk_mps_set_centre = -1); the source is untouched.  A state's product is the same bits whatever the other
 * states of the set and their order, and from run to run.  One launch of qk_mpo_apply_kernel per call; the new set is allocated
 * whole (about max_k w_k w_{k+1} times the source).
 * QK_EINVAL, before anything runs: a null ctx, src, bonds, tensors or out; a set of another context; a complex64 set; a bond
 * outside 1 .. 32 (the message names the cut); bonds[0] or bonds[n_sites] not 1; a tensor entry that is not finite (site and
 * indices); a product bond w_k chi_k above 512 (state and bond) -- 512 is the limit of qk_mps_set_compress and of the fused Gram
 * sweep, so every consumer takes every result.  QK_EDEVICE: an allocation that fails (the message names the bytes asked for).   */
int qk_mps_set_apply_mpo(qk_ctx* ctx, const qk_mps_set* src, const int32_t* bonds /* [n_sites + 1] */,
                         const double* tensors /* site-major [w_k][w_{k+1}][2][2][2] */, qk_mps_set** out);

/* The Gram of any real feature columns (host arrays [n][n_features], for instance qk_pauli_strings_host's output), synchronous:
 *     out[j * ld + i] = exp(-g * sum_m (fx[i][m] - fy[j][m])^2)
 * Rows, columns, fy = NULL, the fixed summation order (exact symmetry, unit diagonal) and the argument errors are those of
 * qk_projected_gram_host; n_features < 1 is QK_EINVAL.  With the 3 n_sites Bloch components as columns it is
 * qk_projected_gram_host at 2 g.                                                                                              */
int qk_feature_gram_host(qk_ctx* ctx, int32_t n_features, int32_t nx, const double* fx /* [nx][n_features] */,
                         int32_t ny, const double* fy /* NULL: Y is X */, double g, double* out, int64_t ld);

/* Entanglement across the bonds of every state of a set, synchronous on the context's stream.  The conventions above: site k =
 * qubit k, states need not be normalised, environments in the sweep's X[ket][bra] orientation (L_0 = R_n = 1, L_n[0][0] =
 * <psi|psi>).  Bond k, k = 1 .. n_sites - 1, cuts the chain between sites k-1 and k:
 *     N_k      = R_k L_k^T / <psi|psi>           (plain transpose; chi_k x chi_k; tr N_k = 1)
 *     lambda_k = the eigenvalues of N_k, descending, >= 0: the Schmidt weights of the cut, sum = 1
 *     purity_k = tr(N_k^2) = sum_i lambda_k[i]^2
 * N_k is not Hermitian but similar to one: with L_k^T = U S U^H and F = S^{1/2} U^H, H_k = F R_k F^H / <psi|psi> is Hermitian,
 * positive semi-definite and has the eigenvalues of N_k.  The values are properties of the state: in exact arithmetic they do not
 * change under a gauge change on any bond or a global factor.  As computed here the invariance holds to about 1e-15 cond(G)^2
 * for a gauge matrix G on the bond: the environments are Gram matrices of the gauge, so every weight carries that absolute error
 * and weights below it are rounding noise (cond = 1 for the builders' canonical forms; random Gaussian gauges of bond 64 reach
 * 1e-11 .. 1e-8); negative noise is clipped to 0.
 *
 * qk_bond_purities_host: out[state][k - 1] = purity_k.  The environment pass of qk_pauli_strings_host (every L_k and R_k of a
 * state, made once), then per bond one GEMM launch for all states (tasks (state, 64 x 64 block)) and one reduction launch in
 * 16-row chunks, the chunk sums added in a fixed order.
 * qk_bond_spectra_host: out[state][k - 1][i] = lambda_k[i] for i < min(chi_k, max_values), zero beyond the true bond; a bond of
 * true dimension 1 has the single weight 1.0 exactly; max_values below a bond returns that bond's largest weights.  The same
 * environment pass, then one workgroup per (state, bond) in one launch per state batch: L_k^T is factorised by the device builder's
 * Jacobi primitive (in LDS below 48 columns, preconditioned block Jacobi on the f64 matrix cores from 48 on), H_k is formed by
 * two workgroup GEMMs and its eigenvalues come from the same primitive.  A factorisation that does not converge is QK_EDEVICE.
 * norms, when given, are the bits qk_local_paulis_host returns.  n_sites = 1 is valid (nothing is written to out).  A value is
 * the same bits whatever the other states of the set, however the call was cut into batches, and from run to run.
 * Device scratch: per state the sweep's planes and every L_k and R_k, for the spectra also a workspace of about 5 chi^2 complex
 * numbers per resident workgroup (chi = the batch's largest bond); counted by the batching rule of qk_local_paulis_host (a quarter
 * of the free memory; the states go in several batches when they do not fit) and released by qk_ctx_trim.
 * QK_EINVAL: a null ctx, set or out; a set of another context; a complex64 set; max_values < 1; for the spectra a true bond above
 * 512 (the factorisation's bookkeeping in LDS is reserved for that bond whatever the set holds, so that a state's path -- and its
 * bits -- do not depend on the other bonds of its batch).                               */
int qk_bond_purities_host(qk_ctx* ctx, const qk_mps_set* set, double* out /* [n_states][n_sites - 1] */, double* norms /* [n_states], may be NULL */);
int qk_bond_spectra_host(qk_ctx* ctx, const qk_mps_set* set, int32_t max_values, double* out /* [n_states][n_sites - 1][max_values] */,
                         double* norms /* [n_states], may be NULL */);

/* ---- block kernels: reduced-state overlaps of the first or last w qubits --------------------------------------------------------
 * The projected kernel of Huang et al. for a subsystem A that is a block at either end of the chain.  Site k is qubit k, states
 * need not be normalised, environments are in the sweep's X[ket][bra] orientation, rows are Y and columns X, yset = NULL means Y is X.
 *     side = 0 (left):   A = qubits 0 .. w-1,       cut at bond w
 *     side = 1 (right):  A = qubits n-w .. n-1,     cut at bond m = n - w            width w = 1 .. n
 *     rho_A(psi) = tr_{not A} |psi><psi| / <psi|psi>
 *     O_w[j][i]  = tr(rho_A(x_i) rho_A(y_j))         real, 0 <= O <= sqrt(S_w(x_i) S_w(y_j)) <= 1
 *     S_w(psi)   = tr(rho_A(psi)^2)                  the self overlap = the purity of the cut
 * Left, at bond w, with E_0 = 1 and E_{k+1}[b'][a'] = sum_s sum_{b,a} E_k[b][a] Ay_k[b][s][b'] conj(Ax_k[a][s][a']) (the mixed left
 * environment the fidelity sweep carries) and the self right environments Rx_w, Ry_w:
 *     O_w <x|x> <y|y> = sum_{a,a',b,b'} Rx_w[a][a'] Ry_w[b][b'] E_w[b][a'] conj(E_w[b'][a])
 * Right, at bond m, with F_n = 1, F_k[b][a] = sum_s sum_{b',a'} Ay_k[b][s][b'] F_{k+1}[b'][a'] conj(Ax_k[a][s][a']) and the self left
 * environments Lx_m, Ly_m:
 *     O_w <x|x> <y|y> = sum_{a,a',b,b'} Lx_m[a][a'] Ly_m[b][b'] F_m[b][a'] conj(F_m[b'][a])
 * (the left form on the reversed images the local sweeps make).  Identities: O_n = |<x|y>|^2 / (<x|x> <y|y>) for both sides; left
 * O_1 = (1 + F_x[0] . F_y[0]) / 2 with the Bloch vectors of qk_local_paulis_host (right: qubit n-1); S_w = the purity of
 * qk_bond_purities_host at bond w (left) or n - w (right) for w < n, S_n = 1; O_w(x, y) = O_w(y, x).
 * Kernels from O are host arithmetic: "overlap" K = O_w; "normalized" K = O_w[j][i] / sqrt(S_w(x_i) S_w(y_j)); "rbf"
 * K = exp(-g (S_w(x_i) + S_w(y_j) - 2 O_w[j][i])) = exp(-g ||rho_A(x_i) - rho_A(y_j)||_F^2), g > 0.
 *
 * qk_block_values_host: values_host[wi][p] = O_w of width widths[wi] for pair p of the plan's list, (x state, y state) as
 * qk_plan_pairs lists them.  One pair chain along the chain gives every width at once: per step two GEMM launches for all pair
 * chains of a batch (tasks (chain, 64 x 64 block)), per chosen width three more (V = Ry^T E, W = E^T conj(V), and the reduction
 * Re sum Rx conj(W) in 16-row chunks added in a fixed order); the chain stops at the largest width.  The self environments come
 * from the environment pass of qk_pauli_strings_host, run once per set; those of the chosen cuts are kept for every state of both
 * sets in one compact buffer.  qk_block_self_host: out[wi][s] = S_w of state s, the pairs (s, s) through the same route, so the
 * diagonal of a symmetric call and S_w are the same bits; norms, when given, are the bits qk_local_paulis_host returns.
 * A (pair, width) value is the same bits whatever the other pairs of the plan, the other widths asked for, the cut into batches
 * and the run: no atomics, no grid barrier, no spin wait.  QK_BLOCK_BATCH=k (read per call) caps the pair chains of a batch.
 * Both calls are synchronous and leave the Gram statistics (qk_get_stats) alone.  Device scratch: the kept environments and the
 * reversed images for the length of the call; per state batch the environments, per pair batch a slot of 6 P^2 doubles per chain
 * (P = the pair's largest padded bond), each bounded by a quarter of the free memory and released by qk_ctx_trim.
 * QK_EINVAL: a null argument (yset and norms may be NULL); a set of another context; a complex64 set; two sets whose numbers of
 * sites differ; a plan whose pair indices exceed the sets; side not 0 or 1; n_widths < 1; widths not strictly increasing or
 * outside 1 .. n_sites.  QK_EDEVICE: the kept environments do not fit a quarter of the free memory (the message names the bytes). */
int qk_block_values_host(qk_ctx* ctx, const qk_mps_set* xset, const qk_mps_set* yset /* NULL: Y is X */, const qk_plan* plan,
                         int32_t side /* 0 left, 1 right */, int32_t n_widths, const int32_t* widths /* strictly increasing, 1..n_sites */,
                         double* values_host /* [n_widths][num_pairs]: O_w of the plan's pairs as listed */);
int qk_block_self_host(qk_ctx* ctx, const qk_mps_set* set, int32_t side, int32_t n_widths, const int32_t* widths,
                       double* out /* [n_widths][n_states]: S_w */, double* norms /* may be NULL; the bits of qk_local_paulis_host */);

/* ---- windows of k qubits: reduced density matrices of contiguous blocks at every position -----------------------------------------
 * The projected kernel of Huang et al. for k-qubit reduced density matrices, and the overlaps, purities and Renyi-2 entropies of
 * interior blocks.  Conventions of the other local sweeps: site k is qubit k, physical index 0 = |0>, states need not be normalised,
 * environments in the sweep's X[ket][bra] orientation, L_0 = R_n = 1, L_n[0][0] = <psi|psi>; fp64 sets only.
 * Window (a, w) = the qubits a .. a+w-1, b = a + w, 1 <= w <= min(n_sites, 6), 0 <= a <= n_sites - w; the row index of rho is
 * s = sum_j s_{a+j} 2^(w-1-j), so qubit a is the most significant bit:
 *     rho_{a,w}[s][s'] = sum over all other sites of psi(.. s ..) conj(psi(.. s' ..)) / <psi|psi>
 *     M^s[alpha][gamma] = (A_a^{s_a} A_{a+1}^{s_{a+1}} ... A_{b-1}^{s_{b-1}})[alpha][gamma]                          chi_a x chi_b
 *     rho_{a,w}[s][s'] <psi|psi> = sum_{alpha,alpha',gamma,gamma'} L_a[alpha][alpha'] M^s[alpha][gamma] R_b[gamma][gamma'] conj(M^{s'}[alpha'][gamma'])
 * Route: G_0 = 1, Gr_0 = R_b, G_{j+1}[beta][(t, sigma, gamma)] = sum_beta' A_c[beta][t][beta'] G_j[beta'][(sigma, gamma)] with c = b-1-j
 * (likewise Gr), H[alpha'][(s, gamma)] = sum_alpha L_a[alpha][alpha'] G_w[alpha][(s, gamma)], and
 * rho[s][s'] <psi|psi> = sum_{alpha, gamma'} Gr_w[alpha][(s, gamma')] conj(H[alpha][(s', gamma')]): about 5 2^w chi^3 complex
 * multiply-adds per window on the matrix cores (4^w chi^3 with open environments) and 4^w chi^2 / 2 in the closing sum.
 * Derived quantities are host arithmetic: O_a[j][i] = tr(rho_a(x_i) rho_a(y_j)) = Re sum rho_a(x_i)[s][s'] conj(rho_a(y_j)[s][s']),
 * the purity S_a = O_a(x, x), K_w[j][i] = exp(-g sum_a ||rho_a(x_i) - rho_a(y_j)||_F^2) = qk_feature_gram_host at g over the columns
 * (Re rho, Im rho); the Pauli coefficients c[p_0 .. p_{w-1}] = tr(rho P_{p_0} (x) .. (x) P_{p_{w-1}}) are real, in the convention of
 * out2[k][p][q] above, and rho = 2^-w sum c P.  w = 1 and w = 2 agree with qk_local_paulis_host and the pair correlators to rounding;
 * the purity of the window (0, w) is qk_bond_purities_host's at bond w.
 *
 * qk_window_rdms_host: rho[state][i] = rho_{starts[i], width}, complex128 with re and im interleaved; starts = NULL means every
 * window 0 .. n_sites - width (n_starts is then ignored).  Guarantees: rho is exactly Hermitian (s <= s' is computed and the
 * conjugate mirrored; the diagonal's imaginary part is exactly 0.0); tr rho = 1 to rounding; pad rows and columns never reach a
 * result; a (state, window) value is the same bits whatever the other states of the set, the other windows asked for, the cut
 * into batches and the run; no atomics, no grid barrier, no spin wait.  norms, when given, are the bits qk_local_paulis_host returns.
 * Per state batch the environment pass of qk_pauli_strings_host, then one chain per (state, window) in chain batches: per step
 * one GEMM launch for every chain of the batch (tasks (chain, 64 x 64 block)), one for H, one closing launch over (chain, 16-row
 * chunk) and one kernel that adds the chunks in a fixed order.
 * Device scratch: per state the sweep's planes and every L_k and R_k, and 8 2^w P^2 doubles per (state, window) of a batch (P = the
 * state's largest padded bond) plus its partial sums, counted by the batching rule of qk_local_paulis_host (a quarter of the free
 * memory; the windows of a state go in several batches when they do not fit) and released by qk_ctx_trim.  QK_WINDOW_BATCH=<k>
 * (read per call) caps the (state, window) chains of a batch at k; the result is the same bits for every k.
 * QK_EINVAL, naming the argument: a null ctx, set or rho; a set of another context; a complex64 set; a width outside
 * 1 .. min(n_sites, 6); a start outside 0 .. n_sites - width; starts that are not strictly increasing; n_starts < 1 when starts
 * are given.  QK_EDEVICE, naming the state: a state of norm 0.                                                                   */
int qk_window_rdms_host(qk_ctx* ctx, const qk_mps_set* set, int32_t width, int32_t n_starts, const int32_t* starts /* NULL: 0 .. n_sites - width */,
                        double* rho /* [n_states][n_windows][2^w][2^w] complex128, re/im interleaved */, double* norms /* [n_states], may be NULL */);

/* ---- measurement shots: perfect sampling of every state of a set -----------------------------------------------------------------
 * qk_sample_host: bits[s][shot][k] = the outcome of measuring qubit k of state s in the Pauli basis bases[shot][k] (1..3 = X, Y, Z;
 * bit 0 = eigenvalue +1), n_shots independent shots per state; logp[s][shot], when given, = the log of the exact probability of
 * the drawn string in the drawn bases, |<b| U_bases |psi>|^2 / <psi|psi>.  One shot: v = [1] over the left bond, for k = 0 .. n-1
 *     W_t = v A_k[.][t][.] (t = 0, 1);   Z: W' = W;  X: W'_0,1 = (W_0 +- W_1)/sqrt2;  Y: W'_0,1 = (W_0 -+ i W_1)/sqrt2
 *     p_o = max(0, Re W'_o R_{k+1} W'_o^H),  tot = p_0 + p_1,  u = uniform(seed, first_state + s, shot, k) in [0, 1)
 *     bit = 1 if (p_1 > 0 and u tot >= p_0) else 0;   logp += log(p_bit / tot);   v = W'_bit / sqrt(p_bit)
 * with the right environments R_k of qk_local_paulis_host (X[ket][bra], R_n = 1).  The uniform is Philox4x32-10 written out in
 * this library: counter (k, shot, first_state + s, 0), key (seed & 0xffffffff, seed >> 32), u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53.
 * Per state batch the reversed chain keeps every R_k; a shot chain is one (state, tile of 64 shots); at site k every chain of a
 * chain batch goes through one launch each of two GEMMs on the f64 matrix cores (shot rows as M, 3-product complex form, fixed K
 * order), the basis rotation and the draw: 4 n_sites launches per chain batch whatever n_shots.  The bits and logp of a
 * (state, shot) depend only on seed, first_state + s, the shot index, that shot's bases and that state's tensors -- not on the other
 * states or shots, the cut into batches and tiles, or the run: no atomics, no grid barrier.  QK_SAMPLE_BATCH=k (read per call)
 * caps the shot chains of a batch.  Synchronous; leaves the Gram statistics alone.  Device scratch: the reversed image, the bits
 * and logp for the length of the call; per state batch the environments, per chain batch a slot of 14 P R doubles per chain (P = the
 * state's largest padded bond, R = its shots padded to 16), each bounded by a quarter of the free memory, released by qk_ctx_trim.
 * QK_EINVAL (the message names the argument): a null ctx, set or bits; a set of another context; a complex64 set; n_shots < 1; a
 * basis code outside 1..3; first_state < 0 or first_state + n_states > 2^32.  QK_EDEVICE: a shot whose tot is 0 or not finite, as
 * for a state of norm 0 (the message names the state).                                                                            */
int qk_sample_host(qk_ctx* ctx, const qk_mps_set* set, int32_t n_shots, const uint8_t* bases /* [n_shots][n_sites], NULL: all Z */,
                   uint64_t seed, int64_t first_state /* global index of state 0 */, uint8_t* bits /* [n_states][n_shots][n_sites] */,
                   double* logp /* [n_states][n_shots], may be NULL */);

/* ---- amplitudes and outcome likelihoods of given strings ---------------------------------------------------------------------------
 * qk_amplitudes_host: the amplitude <b| U_c |psi_s> of every given string under every state of a set -- strings the library did not
 * draw, such as shots measured on hardware -- in the sampler's conventions (site k = qubit k, physical index 0 = |0>, states not
 * necessarily normalised, codes 1..3 = X, Y, Z, outcome bit 0 = eigenvalue +1).  One string b in the bases c: v = [1], E = 0, for
 * k = 0 .. n-1
 *     W_t = v A_k[.][t][.] (t = 0, 1);   Z: W' = W;  X: W'_0,1 = (W_0 +- W_1)/sqrt2;  Y: W'_0,1 = (W_0 -+ i W_1)/sqrt2
 *     u = W'_{b[k]} over the true bond;   m = max_a max(|Re u[a]|, |Im u[a]|)
 *     m > 0: m = f 2^e with 0.5 <= f < 1 (frexp), v = u 2^-e (exact), E += e;   m == 0: v = 0, E = 0
 *     amplitude = v_n[0] 2^E:   mant[s][j] = (Re, Im) of v_n[0],  expo[s][j] = E
 *     logp[s][j] = 2 (log |v_n[0]| + E log 2) - log <psi_s|psi_s>          (-inf for a zero amplitude: not an error)
 * The larger component of a mantissa is in [0.5, 1), or the mantissa is exactly 0 with E = 0.  The rescale is a power of two and
 * the maximum has no order, so it costs no bits and amplitudes far below the smallest double (long or unnormalised chains) survive.
 * <psi|psi> is L_n[0][0] of the environment pass of qk_pauli_strings_host -- the bits qk_local_paulis_host returns -- and is computed
 * only when logp or norms is given.  bits_per_state = 0: one table [n_strings][n_sites] for every state; 1: a table per state
 * (the shots of state s under state s; state s' x shots of state s is a call per s with the shared form).  bases are shared by
 * every state, as the sampler's.
 * An amplitude chain is one (state, tile of 64 strings), rows padded to 16; at site k every chain of a chain batch goes through one
 * GEMM launch on the f64 matrix cores (string rows as M, K = the true left bond, fixed K order) and one launch that rotates, picks,
 * takes the row maximum and scales: 2 n_sites + 1 launches per chain batch whatever n_strings -- half the sampler's, and no right
 * environments.  mant and expo of a (state, string) are the same bits whatever the other states of the set, the other strings and
 * their order, a shared or a per-state table, the cut into batches and the run: no atomics, no grid barrier, no spin wait.
 * QK_AMP_BATCH=k (read per call) caps the chains of a batch; the result is the same bits for every k.  Synchronous; leaves the Gram
 * statistics alone.  Device scratch: the reversed image, the tables and the results for the length of the call; per state batch
 * the sweep's planes (and every L_k and R_k when <psi|psi> is asked for), per chain batch a slot of 6 P R doubles per chain (P = the
 * state's largest padded bond, R = its strings padded to 16), each bounded by a quarter of the free memory, released by qk_ctx_trim.
 * QK_EINVAL (the message names the argument): a null ctx, set, bits, mant or expo; a set of another context; a complex64 set;
 * n_strings < 1; a byte of bits other than 0 or 1; a basis code outside 1..3; bits_per_state not 0 or 1.  QK_EDEVICE: a state of
 * norm 0 when logp is asked for (the message names the state).                                                                      */
int qk_amplitudes_host(qk_ctx* ctx, const qk_mps_set* set, int32_t n_strings,
                       const uint8_t* bits, int32_t bits_per_state /* 0: [n_strings][n_sites] shared; 1: [n_states][n_strings][n_sites] */,
                       const uint8_t* bases /* [n_strings][n_sites], NULL: all Z; shared by every state */,
                       double* mant /* [n_states][n_strings][2] */, int32_t* expo /* [n_states][n_strings] */,
                       double* logp /* [n_states][n_strings], may be NULL */, double* norms /* [n_states], may be NULL */);

/* ---- block overlaps at finite shots: the randomised-measurement estimator -------------------------------------------------------
 * qk_shot_block_sums_host: the integer sums of the randomised-measurement overlap (Elben et al., PRL 124, 010504 (2020)) of two
 * outcome tables, for the first (side 0) or last (side 1) w qubits and every w of widths, from the same shot pairs.  It needs no
 * MPS set: it works on any outcome tables, such as the bits of qk_sample_host.
 * Shots.  There are U settings of M shots each.  The shot index is u M + a.  All M shots of setting u were measured in the same
 * bases (row u of the caller's bases table), and every state of X and Y in the same table.
 * Packed word of a shot.  It holds the block's qubits, at most 32 of them.  side = left: bit k of the word is bits[k], for
 * k < min(n, 32).  side = right: bit k is bits[n-1-k].  Other bits of the word are 0.  Widths are 1 <= w <= min(n, 32), strictly
 * increasing.
 *     D_w(s, s')  = popcount((s xor s') & (2^w - 1))                 (w = 32: the whole word; no shift by 32)
 *     term_w      = (-1)^D_w 2^(w - D_w)                             an integer in [-2^(w-1), 2^w]
 *     S_u[w][p]   = sum_{a,b < M} term_w(X[i][uM+a], Y[j][uM+b])  -  [p is a self pair] M 2^w
 *     sums[w][p]  = sum_u S_u[w][p]                                  int64, exact
 *     N           = M^2  (cross pair),   M (M - 1)  (self pair: Y is X and i == j; the a == b terms are removed)
 *     O^_w        = sums / (U N)
 *     stderr_w    = std over u of S_u / N (ddof = 1) / sqrt(U)       (U >= 2, else nan)
 * E[O^_w] = O_w = tr(rho_A(x_i) rho_A(y_j)) exactly for bases drawn uniformly from X, Y, Z per setting and qubit: averaging Z(x)Z
 * over the three gives (XX + YY + ZZ) / 3, so the per-qubit weight (1 + 3 z z') / 2 averages to SWAP.  A self pair needs M >= 2.  In
 * a call with bits_y given, equal indices are not a self pair.
 * Overflow rule: U M^2 2^w_max <= 2^62, else QK_EINVAL.
 * A pack kernel makes the words (one lane per (state, shot)); the sums kernel takes one workgroup per (pair, chunk of settings),
 * x words in registers, y words staged in LDS, and writes S_u; a second kernel adds over the settings.  Everything is integer
 * arithmetic: the result is exact and does not depend on any order, batch cut or run.  Device scratch: the words (4 bytes per
 * shot), and per pair batch n_widths U int64 per pair in the context's local scratch (qk_ctx_trim releases it), by the batching rule
 * of qk_local_paulis_host (a quarter of the free memory; pairs go in batches when they do not fit).  Synchronous; leaves the Gram
 * statistics alone.
 * QK_EINVAL: a null ctx, bits_x, pairs, widths or sums; n_sites, n_settings, shots_per_setting, nx, ny, n_pairs or n_widths below 1;
 * bits_y NULL with ny != nx; a pair index outside its table; a self pair with shots_per_setting 1; side not 0 or 1; widths not
 * strictly increasing in 1 .. min(n_sites, 32); the overflow rule (the message names the three numbers); a byte other than 0 or 1
 * among the block's qubits (the message names bits_x or bits_y).                                                                  */
int qk_shot_block_sums_host(qk_ctx* ctx, int32_t n_sites, int32_t n_settings, int32_t shots_per_setting,
                            int32_t nx, const uint8_t* bits_x /* [nx][U*M][n_sites] */, int32_t ny, const uint8_t* bits_y /* NULL: Y is X */,
                            int64_t n_pairs, const int32_t* pairs /* [n_pairs][2] = (x index, y index), any order, duplicates allowed */,
                            int32_t side, int32_t n_widths, const int32_t* widths,
                            int64_t* sums /* [n_widths][n_pairs] */, int64_t* per_setting /* [n_widths][n_pairs][U], may be NULL */);

/* ---- the classical-shadow kernel: exact shot-pair histograms ---------------------------------------------------------------------
 * qk_shadow_hist_host: what the shadow kernel of Huang, Kueng, Torlai, Albert and Preskill (Science 377, eabk3333 (2022)) needs of
 * two outcome tables.  It needs no MPS set: it works on any outcome tables, such as the bits of qk_sample_host, with the bases they
 * were measured in (bit 0 = eigenvalue +1; codes 1, 2, 3 = X, Y, Z).  bases_*_per_state = 0: one table [shots][n_sites] shared by
 * every state of that side; 1: a table per state [n][shots][n_sites].
 * The single-qubit shadow of a shot is sigma = 3 |s><s| - I, and tr(sigma_k sigma'_k) of two shots is 5 (qubit k measured in the
 * same basis, same outcome), -4 (same basis, other outcome) or 1/2 (other basis).  With a and b the numbers of qubits of the first
 * and second kind,
 *     sum_k tr(sigma_k sigma'_k) = n/2 + 4.5 d,      d = a - b  in [-n, n]
 *     hist[p][d + n]  = #{(t, t') : d(X[i] shot t, Y[j] shot t') = d}      int64, exact;  sum_d hist[p][.] = shots_x shots_y
 *     equal[p][d + n] = the same over the pairs t = t' alone               (shots_x == shots_y)
 *     inner[p]        = sum_d hist[p][d + n] exp(gamma / n (n/2 + 4.5 d)) / (shots_x shots_y),   K_shadow[p] = exp(tau inner[p])
 * The weights are applied on the host (engine.shadow_inner, shadow_kernel): one histogram serves every gamma, tau and f(d).  When
 * both tables were measured in one shared bases table the pairs t = t' share their bases on every qubit and bias a cross-pair
 * estimate at order 1/shots; hist - equal over shots (shots - 1) pairs is the estimate without them.  In a self pair they are a shot
 * paired with itself, d = n.
 * Packed record of a shot: per group of 32 qubits three uint32 planes; bit k % 32 of group k / 32 holds the outcome bit (plane 0),
 * code & 1 (plane 1), code >> 1 (plane 2); pad bits 0.  Then
 *     eq = ~(p1 ^ p1') & ~(p2 ^ p2') & (p1 | p2),      d = popcount(eq) - 2 popcount(eq & (p0 ^ p0'))      summed over the groups.
 * A pack kernel makes the records (one lane per (state, shot)); the histogram kernel takes one workgroup per (pair, range of blocks
 * of 64 x shots), x records in registers, y records staged in LDS, one LDS increment per shot pair into per-lane counters (or, up to
 * 2^14 shot pairs per pair of states, into one histogram per wave), and writes an int64 row per task; a second kernel adds the
 * tasks of a pair; a third counts the pairs t = t'.  Cost: n_pairs shots_x shots_y shot pairs of about 9 vector instructions per
 * group each.  Everything is integer arithmetic: the result is exact and does not depend on any order, batch cut, launch cut or run.
 * Device scratch: the records (12 bytes per 32 qubits per shot), and per pair batch (tasks per pair + 2) (2 n + 1) int64 per pair in
 * the context's local scratch (qk_ctx_trim releases it), by the batching rule of qk_local_paulis_host (a quarter of the free memory;
 * pairs go in batches when they do not fit; QK_SHADOW_BATCH=k caps the pairs of a batch).  Synchronous; leaves the Gram statistics
 * alone.
 * QK_EINVAL (the message names the argument): a null ctx, bits_x, bases_x, pairs or hist; n_sites, nx, shots_x, ny, shots_y or
 * n_pairs below 1; n_sites > 128; bits_y NULL with ny != nx, with shots_y != shots_x or with bases_y non-NULL; bits_y given with
 * bases_y NULL; a pair index outside its table; a *_per_state flag not 0 or 1; equal given with shots_x != shots_y; a bit other than
 * 0 or 1 (names bits_x or bits_y); a basis code outside 1 .. 3 (names bases_x or bases_y).                                       */
int qk_shadow_hist_host(qk_ctx* ctx, int32_t n_sites,
                        int32_t nx, int32_t shots_x, const uint8_t* bits_x /* [nx][shots_x][n_sites] */, const uint8_t* bases_x, int32_t bases_x_per_state,
                        int32_t ny, int32_t shots_y, const uint8_t* bits_y /* NULL: Y is X */, const uint8_t* bases_y, int32_t bases_y_per_state,
                        int64_t n_pairs, const int32_t* pairs /* [n_pairs][2] = (x index, y index), any order, duplicates allowed */,
                        int64_t* hist /* [n_pairs][2 n_sites + 1] */, int64_t* equal /* same shape, may be NULL */);

/* ---- Pauli strings estimated from measurement shots ---------------------------------------------------------------------------------
 * qk_shot_strings_host: for every state of an outcome table and every Pauli string, how many shots were measured in the string's
 * bases on its support, and the sum of their signs -- the finite-shot counterpart of qk_pauli_strings_host, and through the 4^w
 * strings of a window of w qubits that of qk_window_rdms_host.  Like qk_shadow_hist_host it needs no MPS set and shares its
 * conventions: qubit k = site k, bit 0 = eigenvalue +1, basis codes 1, 2, 3 = X, Y, Z, n_sites <= 128; bases_per_state = 0: one
 * table [shots][n_sites] shared by every state, 1: a table per state.  A string is n_sites codes 0 .. 3 = I, X, Y, Z; its support
 * is the qubits with a code other than 0.  For state s and string m:
 *     match(t)      = bases[(s,) t][k] == strings[m][k] for every k of the support
 *     counts[s][m]  = #{t : match(t)}
 *     sums[s][m]    = sum over the matching t of prod_{k in support} (1 - 2 bits[s][t][k])              both int64, exact
 *     value[s][m]   = sums / counts, 0.0 where counts == 0       (on the host: engine.string_values; the convention of estimate_paulis)
 * The all-identity string has counts = sums = shots.
 * Packed form: a shot is the record of qk_shadow_hist_host (planes p0, p1, p2 per group of 32 qubits); a string is two planes per
 * group, s1 = code & 1 and s2 = code >> 1, I and pad bits 0 in both, packed on the host.  With supp = s1 | s2 a shot matches when
 * supp & ((s1 ^ p1) | (s2 ^ p2)) == 0 in every group, and its sign is 1 - 2 (popcount(p0 & supp) summed over the groups & 1).
 * The pack kernel of qk_shadow_hist_host makes the shot records; the estimator kernel takes one workgroup per (state, block of 64
 * strings, range of shots): a string per lane with its record in registers, the shot records staged in LDS 256 at a time and read
 * as a broadcast, about 7 vector instructions per (shot, string, group) and as many again per (shot, string); a task writes int32 partial sums and counts to a row of
 * its own (a task's shots are capped so that neither can overflow), and a second kernel adds the rows of a (state, block of
 * strings) into int64.  The result is exact and does not depend on any order, batch cut, launch cut or run; a (state, string)
 * result does not depend on the other states or strings; no global atomic, no workgroup waits for another.
 * Device scratch: the shot records (12 bytes per 32 qubits per shot), and per string batch the string records, the task rows and
 * the int64 totals in the context's local scratch (qk_ctx_trim releases it), by the batching rule of qk_local_paulis_host (a
 * quarter of the free memory; strings go in batches when the rows do not fit; QK_SHOT_STRINGS_BATCH=k, read per call, caps the
 * strings of a batch).  A launch takes at most 2048 tasks.  Synchronous; leaves the Gram statistics alone.
 * QK_EINVAL (the message names the argument): a null ctx, bits, bases, strings, sums or counts; n_sites, n_states, shots or
 * n_strings below 1; n_sites > 128; bases_per_state not 0 or 1; a bit other than 0 or 1 (names bits); a basis code outside 1 .. 3
 * (names bases); a string code above 3 (names strings and the string's index).                                                    */
int qk_shot_strings_host(qk_ctx* ctx, int32_t n_sites, int32_t n_states, int32_t shots,
                         const uint8_t* bits /* [n_states][shots][n_sites] */,
                         const uint8_t* bases /* [shots][n_sites], or [n_states][shots][n_sites] */, int32_t bases_per_state,
                         int32_t n_strings, const uint8_t* strings /* [n_strings][n_sites], codes 0..3 */,
                         int64_t* sums /* [n_states][n_strings] */, int64_t* counts /* same shape */);

/* ---- compressing a set: one canonical truncation sweep per state -------------------------------------------------------------
 * qk_mps_set_compress: *out = a new fp64 set of the same context that owns its memory, every state of src truncated ONCE on its
 * final tensors; src is left untouched.  One workgroup per state (workgroup b takes states b, b + grid, ...), two passes over the
 * site tensors themselves -- no environments, so amplitudes are kept to rounding:
 *   pass 1, right to left, no truncation: site k as a chi_k x 2 chi_{k+1} matrix = carry x (row-orthonormal Q); the carry goes into
 *           site k - 1.  Singular values <= value_of_zero ||site||_F go: a bond whose rank is below its dimension shrinks to it.
 *   pass 2, left to right: the centre as a 2 chi'_k x chi_{k+1} matrix = U S V^H, sigma descending, total = sum sigma^2:
 *           1. sigma_i <= value_of_zero sqrt(total) go;  2. from the small end, values go while their summed weight stays
 *           <= max_discard total;  3. if max_bond > 0 at most max_bond stay;  4. at least one stays.
 *           Site k = U_m (an isometry), (S_m V_m^H) sqrt(total / kept) goes into site k + 1.
 * <psi'|psi'> = <psi|psi>, the norm sits in the last site, sites 0 .. n_sites - 2 are left isometries.
 * discarded[state][k - 1] = 1 - kept / total at bond k (the dropped weights summed from the small end); fidelity[state] = the
 * product over the bonds, in bond order, of kept / total = |<psi|psi'>|^2 / (<psi|psi> <psi'|psi'>) (the projectors of pass 2 are
 * nested).  By Eckart-Young 1 - fidelity >= max_k sum_{i >= chi'_k} lambda_k[i], lambda the spectra of the ORIGINAL state.
 * Every factorisation is the device builder's Jacobi primitive on the smaller side of the matrix (in LDS below 48 columns,
 * preconditioned block Jacobi on the f64 matrix cores from 48 on), every product a workgroup GEMM on the matrix cores.  The compact
 * sites are written into a staging buffer whose slots are sized by the input bonds (new bonds never exceed old ones); the host
 * reads the new bonds and a pack kernel writes the padded split planes of the new set (the layout of qk_mps_set_create).
 * A state's result -- image, fidelity, discarded -- is the same bits alone, in any set, under any batch cut and from run to run.
 * Device scratch: the staging buffer (the true-bond corners of a batch, interleaved) and about 6 chi^2 complex numbers per
 * resident workgroup (chi = the batch's largest bond), by the batching rule of qk_local_paulis_host (a quarter of the free
 * memory; the states go in several batches when they do not fit); all of it is released before the call returns, so qk_ctx_trim
 * has nothing of it to give back.
 * A one-site chain is copied (fidelity 1).  QK_EINVAL: a null ctx, src or out; a set of another context; a complex64 set;
 * max_bond < 0; a negative or non-finite max_discard or value_of_zero; a true bond above 512.  QK_EDEVICE: a factorisation that
 * does not converge; a state of norm 0 (named in the message).                                                            */
int qk_mps_set_compress(qk_ctx* ctx, const qk_mps_set* src, int32_t max_bond /* 0: no cap */, double max_discard /* >= 0 */,
                        double value_of_zero /* >= 0 */, qk_mps_set** out,
                        double* fidelity /* [n_states], may be NULL */, double* discarded /* [n_states][n_sites-1], may be NULL */);

/* ---- profiler ranges -----------------------------------------------------------------------------------------
 * roctx ranges (rocprofv3 --marker-trace) named "qk:build", "qk:upload", "qk:sweep", "qk:scatter", "qk:allgather_values",
 * "qk:allgather_sets" are opened by the library around its own phases -- the reference's MPI.Wtime() sites G:209-231
 * (circuit simulation), G:379-381 (vdot) and G:341-352 (round robin) --; callers use the same two entry points for theirs.
 * No-ops unless a profiler is attached (or QK_ROCTX=1): the marker library is resolved at first use.                  */
int qk_range_push(const char* name);
int qk_range_pop(void);

/* ---- multi-GPU: one process, k MI355X of one node, RCCL over xGMI ----------------------------------------------
 * Replaces the reference's communicator plumbing: rank / chunk bookkeeping G:149-199 (one MPI process per GPU, device =
 * rank % n_devices, G:152), the ring of pickled MPS G:341-352, 415-419 and the final comm.reduce(kernel_mat, SUM) G:428
 * (which only ever gathers: every rank's matrix is zero outside its own tiles).
 *   qk_comm_init_all      a context per device (device_ids = NULL: devices 0..n-1) and an RCCL communicator clique
 *                         (ncclCommInitAll); RCCL is loaded at run time (librccl.so.1), the single-GPU entry points do not
 *                         need it.  qk_comm_ctx(comm, r) is rank r's context: sets for rank r are created on it.
 *   qk_mps_set_allgather  local[r] = the states [lo[r], lo[r] + n_r) that rank r built or uploaded (NULL = an empty share);
 *                         ONE ncclAllGather of the packed images and full_out[r] = the whole set of `total` states on
 *                         every device (the caller destroys them).
 *   qk_gram_sharded       xsets[r] / ysets[r] = the whole set(s) on device r (ysets = NULL: symmetric Gram).  Every device
 *                         sweeps rank r's share of the plan (qk_plan_create(world = n, rank = r)) in one launch, the packed
 *                         values meet in ONE ncclAllGather, every device scatters (and mirrors) its own dense K; rank 0's K
 *                         is copied to out_host[ny][ld] (may be NULL) and the call returns when every device is done.
 *                         Plans and buffers are kept while the same sets come back.
 *   qk_comm_device_gram   device r's dense K of the last call (valid until the next one);  qk_comm_stats: rank r's sweep
 *                         statistics and the device time between enqueueing the all-gather on rank 0's stream and its
 *                         completion (includes waiting for the slowest rank; the reference's r0_RR_recv key).           */
typedef struct qk_comm qk_comm;
int qk_comm_init_all(int32_t n_devices, const int32_t* device_ids, qk_comm** out);
int qk_comm_destroy(qk_comm* comm);
int32_t qk_comm_size(const qk_comm* comm);
qk_ctx* qk_comm_ctx(qk_comm* comm, int32_t rank);
int qk_mps_set_allgather(qk_comm* comm, qk_mps_set* const* local, const int32_t* lo, int32_t total, qk_mps_set** full_out);
int qk_gram_sharded(qk_comm* comm, qk_mps_set* const* xsets, qk_mps_set* const* ysets, double* out_host, int64_t ld);
int qk_comm_device_gram(qk_comm* comm, int32_t rank, const double** k_dev);
int qk_comm_stats(const qk_comm* comm, int32_t rank, qk_stats* out, double* allgather_ms);

/* Device self-test of the f64 MFMA fragment maps the kernels rely on (returns
 * 0 if the 16x16x4 product of two known matrices matches the host result). */
int qk_selftest_mfma(qk_ctx* ctx);

/* ---- device MPS builder ------------------------------------------------------------
 * Replaces simulate(libhandle, circ, SimulationAlgorithm.MPSxGate, config) (G:141-144, 221, 263) for a gate program (qk_program below): all
 * data points share the gate structure and differ in the half-turn angles.  One persistent launch; per two-qubit gate a one-sided Jacobi
 * SVD and the truncation rule of the host builder: drop the trailing singular values whose squared weight stays <= trunc_budget (= 1 -
 * truncation_fidelity, G:141-144; criterion as KernelPkg.jl:68), values <= value_of_zero never count.  max_bond bounds every bond (QK_EINVAL
 * if a state outgrows it).  The result stays on the device until downloaded: per state and site a complex128 tensor [chi_l][2][chi_r]
 * row-major, sites back to back, state s at offsets[s] (complex elements). */
typedef struct qk_built qk_built;
#define QK_BUILD_PARTIAL 1u /* a state that outgrows max_bond is dropped (its fidelity reads -1, it has no tensors: build it
                             * elsewhere) instead of failing the call; its workgroup stops at the offending gate        */
#define QK_BUILD_TRUNCATE 2u /* max_bond is a bond CAP: at most max_bond singular values survive a gate (the `chi` of pytket-cutensornet's
                             * Config, reference G:141-144, which the reference leaves unset); the weight it costs goes into the
                             * state's fidelity like any other truncation.  Without it a state that needs more is an error (or, with
                             * QK_BUILD_PARTIAL, dropped).                                                                          */
/* What to build: the gate program.  A table whose count is 0 is absent: its pointers are not read and its op codes are unknown.  Before
 * anything runs the program is checked (csrc/qk_program.h; the host builder, csrc/qk_builder.cpp, runs the same struct with n_states = 1
 * through the same checks), QK_EINVAL with the gate's position in the message: an op code outside the vocabulary, then what each table lists. */
typedef struct qk_program {
  uint32_t size;  int32_t n_states, n_qubits, n_ops;  /* size = sizeof(qk_program); the data points share op, q0 and every table without a state stride; n_ops = 0: every state stays |0...0> (or the snapshot) */
  /* op[n_ops]: 0 = H, 1 = Rz, 2 = XXPhase on (q0, q0+1), 3 = SWAP on (q0, q0+1), 4 = Rx, 5 = Ry, 6 = YYPhase on (q0, q0+1), 7 = ZZPhase on
   * (q0, q0+1); TKET matrices, theta = pi alpha / 2.  With the matrix table: 8 = a 2x2 unitary on q0, 9 = a 4x4 unitary on (q0, q0+1).
   * With n_channels > 0: 10 = a one-qubit Kraus channel on q0.  With n_channels2 > 0: 11 = a two-qubit Kraus channel on (q0, q0+1) --
   * two-qubit depolarising noise, correlated dephasing, projectors on a pair, joint post-selection. A channel gate runs as a quantum
   * trajectory or with a forced branch (projectors, post-selection, a mid-circuit measurement with a chosen outcome, replay of a trajectory). */
  const int8_t* op;  const int32_t* q0;  /* [n_ops] each */
  const double* alpha;  /* [n_states][n_ops] half-turn angles; ignored at codes 8 to 11 */
  /* The matrix table of codes 8 and 9.  The matrix of gate i is entry mat[i]: complex128 [n_mats][4][4] row-major, (re, im) interleaved; a
   * 2x2 sits in [:2][:2] of its slot.  The 4x4 index is (s_q0, s_q0+1) with qubit q0 most significant (TKET's order), and new[(p,p')] = sum
   * M[(p,p')][(s,s')] old[(s,s')].  Checked: a matrix gate past the last qubit (pair); mat[i] outside 0..n_mats-1; a matrix with an entry
   * that is not finite; a matrix that is not unitary, max |M^H M - 1| > 1e-12 (the canonical-form bookkeeping assumes unitary gates: a
   * one-qubit gate never moves the orthogonality centre; what is not unitary -- a projector, a post-selection, noise -- is a channel). */
  int32_t n_mats, mats_state_stride; /* the stride: 0 -- one table for all states -- or n_mats -- state s reads mats + s * n_mats * 32 doubles (a data-dependent gate) */
  const double* mats;  const int32_t* mat;  /* [mats_state_stride ? n_states : 1][n_mats][4][4][2]; [n_ops], read only where op is 8 or 9 */
  /* The channel tables of codes 10 and 11; either may be absent when its code does not occur.  Channel c of code 10 is n_kraus[c] (1..4)
   * matrices kraus[c][k][s'][s] = <s'|K_k|s>; of code 11, n_kraus2[c] (1..16) matrices kraus2[c][k][(p,p')][(s,s')], the index convention
   * of the 4x4 matrix gates.  Checked: channel[i] outside its table; a count outside 1..4 (1..16); an entry that is not finite; branch[i]
   * outside -1 .. m-1; a DRAWN channel that is not trace preserving, max |sum_k K_k^H K_k - 1| > 1e-12 (a forced branch may be any finite
   * matrix); a channel gate outside the register.
   * Code 10 on A_q = t[l][2][r]: the orthogonality centre is brought onto site q exactly (the centre moves of the two-qubit gates; no
   * truncation); N = sum |t|^2, p_k = sum_{a,c} |K_k t[a][.][c]|^2, tot = p_0 + .. + p_{m-1} in ascending order; b = branch[i], or drawn:
   * the first k with p_k > 0 and u tot < p_0 + .. + p_k (none: the last k with p_k > 0), u the uniform of Philox4x32-10 with counter
   * (first_gate + i, trajectory[s], state_index[s], 2) and key (seed & 0xffffffff, seed >> 32), made from the first two output words as the
   * sampler's (qk_sample_host; stream 0 draws shots, stream 1 bases, stream 2 branches); A_q <- K_b A_q / sqrt(p_b), and log(p_b / N) is
   * added to the state's log-weight.  The centre stays on q, the bonds do not change.
   * Code 11: the centre is brought into the pair by the moves of a two-qubit gate and theta[(a,p)][(p',c)] = A_q A_q+1 is formed; N = sum
   * |theta|^2, p_k = sum_{a,c} |K_k theta[a,(.,.),c]|^2, tot, the branch b and the uniform as for code 10 (same counter); theta <- K_b
   * theta / sqrt(p_b); then the SVD, truncation, fidelity product, bond cap and centre placement of any two-qubit gate (the bond may shrink
   * or be cut), and log(p_b / N) is added to the log-weight.  The device adds the sums per thread over its strided (a, c) in ascending
   * order and the threads' partials in ascending thread order, the Kraus matrices in groups of four per pass over theta; a forced branch
   * takes one pass (N and p_b).  At run time QK_EDEVICE, naming the state and the gate, when p_b is 0 or not finite (an impossible outcome was post-selected) or tot is
   * 0 in a draw.  A state's result depends on seed, its two indices, its gates and the tables only -- not on the other states of the call,
   * their number, their order, or the launch; the sums use no atomics.  To that end a program with a channel table, and a build resumed
   * from a snapshot of one, takes its workgroup shape from max_bond alone (the switch to 512 threads for at most one state per CU at
   * max_bond 33..64 is for programs without channels); QK_BUILD_WGS overrides the shape and with it the bits.  A launch shape whose LDS
   * cannot hold the staging of a channel step is QK_EINVAL. */
  int32_t n_channels, n_channels2;
  const double* kraus;   const int32_t* n_kraus;   /* [n_channels][4][2][2][2] complex128, (re, im) interleaved; [n_channels] */
  const double* kraus2;  const int32_t* n_kraus2;  /* [n_channels2][16][4][4][2]; [n_channels2] */
  const int32_t* channel;  /* [n_ops], read where op is 10 (an index into kraus) or 11 (into kraus2); alpha[i] and mat[i] are ignored there */
  const int32_t* branch;   /* [branch_state_stride ? n_states : 1][n_ops], read where op is 10 or 11: -1 draws the branch, k >= 0 forces branch k */
  int32_t branch_state_stride; /* 0 -- one row for all states -- or n_ops -- state s reads branch + s * n_ops */
  uint32_t first_gate;  uint64_t seed;  /* first_gate: the position of gate 0 in the uninterrupted program: a resumed build, handed it, draws what that run draws */
  const uint32_t *state_index, *trajectory; /* [n_states] each; NULL: 0 .. n_states-1, and all 0 */
  /* Classical control, one entry per gate; cond_gate NULL: none.  cond_gate[i] is -1 (gate i is unconditional) or the position g < i, in
   * this program, of a gate of op code 10 or 11; cond_mask[i] (read where cond_gate[i] >= 0) has bit v set when branch v of gate g lets
   * gate i run.  With b the branch recorded for gate g of this state, gate i runs when b >= 0 and bit b of cond_mask[i] is set; else it is
   * skipped: no centre move, no theta, no SVD, no change of a bond, of the fidelity or of the log-weight, no draw.  A skipped gate is a
   * done gate all the same (checkpoints, first_gate + i and the positions conditions name count it), and the look-ahead that places the
   * centre behind a two-qubit gate reads the op codes alone.  A skipped gate of code 10 or 11 records branch -2, so a condition on it is
   * false; the gate conditioned on may itself be conditional; any op code may be conditional; cond_mask = 0 is "never".  The persistent
   * kernel decides per state and gate by one load of the state's branch record: no atomics, no barrier between workgroups.  Positions are
   * those of this program: a resumed build conditions only on gates it runs itself.  Checked: rows in a program without a channel table;
   * cond_gate[i] < -1 or >= i; op[cond_gate[i]] not 10 or 11; a mask bit at or above the number of Kraus matrices of that gate's channel; cond_mask NULL. */
  const int32_t* cond_gate;  const uint32_t* cond_mask;
} qk_program;
typedef struct qk_build_run { /* how to run it */
  uint32_t size, flags; /* sizeof(qk_build_run); QK_BUILD_PARTIAL, QK_BUILD_TRUNCATE */
  double trunc_budget, value_of_zero;  int32_t max_bond; /* 2..1024 */
  /* Snapshots, for scans over the depth of a circuit: the state after checkpoints[j] gates (counted from 1) is kept as well, j = 0 ..
   * n_checkpoints-1: strictly increasing, each in 1..n_ops, the last one n_ops.  n_checkpoints = 0 or checkpoints NULL: one snapshot after
   * the whole program (n_checkpoints < 0 is QK_EINVAL).  A snapshot is a copy: the run does the arithmetic of a run without checkpoints,
   * and the accessors without a snapshot index read the last one.  A snapshot is in mixed-canonical gauge, with its orthogonality centre
   * recorded.  All snapshots share the one heap, so it is sized for n_checkpoints states per state (QK_EDEVICE if it turns out too small). */
  int32_t n_checkpoints;  const int32_t* checkpoints;
  /* Resume (NULL: from |0...0>): every state starts as snapshot initial_snapshot of `initial` -- same context, n_states and n_qubits, no
   * dropped state, no bond above max_bond, else QK_EINVAL -- and the program holds the gates that FOLLOW it (with their tables); the
   * fidelity and the log-weight go on from the snapshot's, also when the gates that remain hold no channel (every record then carries the
   * snapshot's log-weight).  `initial` is only read.  Resuming snapshot j of a run with that run's gates from checkpoints[j] on is gate for
   * gate the arithmetic of the uninterrupted run.  QK_BUILD_PARTIAL with more than one checkpoint or with `initial` is QK_EINVAL. */
  const qk_built* initial;  int32_t initial_snapshot;
} qk_build_run;
/* The builder.  A struct whose size field is not its sizeof here is QK_EINVAL naming both sizes, before anything else is looked at;
 * qk_program_size and qk_build_run_size return the two sizeofs of this library, for bindings that mirror the structs. */
int qk_build_program(qk_ctx* ctx, const qk_program* program, const qk_build_run* run, qk_built** out);
uint32_t qk_program_size(void), qk_build_run_size(void);
/* The entries from before qk_program, their arguments in its fields' names: each fills the two structs and calls qk_build_program; every one
 * after qk_build_mps needs checkpoints (NULL or n_checkpoints < 1: QK_EINVAL).  qk_build_mps: op, q0, alpha, the budget, zero, max_bond, flags. */
int qk_build_mps(qk_ctx* ctx, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha,
                 double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, qk_built** out);
/* dims[n_states][n_qubits+1], fidelity[n_states], offsets[n_states], total complex elements, kernel time; any may be NULL */
int qk_built_info(const qk_built* built, int32_t* dims, double* fidelity, int64_t* offsets, int64_t* total_complex,
                  double* kernel_ms);
/* What the build launched (read-only; any pointer may be NULL): `grid` workgroups of `threads` threads each (512: one workgroup per
 * CU, 256: two or four), and `slots` = workgroups per CU x CUs, the number the grid was clipped to (free memory can clip it further).
 * The kernel is persistent: with grid < n_states workgroups take further states from the queue after their first.                    */
int qk_built_launch(const qk_built* built, int32_t* grid, int32_t* threads, int32_t* slots);
int qk_built_download(const qk_built* built, double* host /* 2 * total_complex doubles (re, im interleaved) */);
/* The built states as a set of the Gram engine (the image qk_mps_set_create makes from host tensors), packed on the
 * device: nothing crosses PCIe between the builder and the sweep.  The set is independent of `built` afterwards.  */
int qk_mps_set_from_built(qk_ctx* ctx, const qk_built* built, qk_mps_set** out);
int qk_built_destroy(qk_built* built);
/* qk_build_mps_scan: qk_build_mps plus n_checkpoints, checkpoints, initial, initial_snapshot */
int qk_build_mps_scan(qk_ctx* ctx, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double*
                      alpha, double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const
                      int32_t* checkpoints, const qk_built* initial, int32_t initial_snapshot, qk_built** out);
/* qk_build_mps_gates: qk_build_mps_scan plus n_mats, mats, mats_state_stride, mat */
int qk_build_mps_gates(qk_ctx* ctx, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double*
                       alpha, double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const
                       int32_t* checkpoints, const qk_built* initial, int32_t initial_snapshot, int32_t n_mats, const double* mats, int32_t
                       mats_state_stride, const int32_t* mat, qk_built** out);
/* qk_build_mps_channels: qk_build_mps_gates plus n_channels, kraus, n_kraus, channel, branch, branch_state_stride, seed, state_index,
 * trajectory, first_gate */
int qk_build_mps_channels(qk_ctx* ctx, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double*
                          alpha, double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, int32_t n_checkpoints, const
                          int32_t* checkpoints, const qk_built* initial, int32_t initial_snapshot, int32_t n_mats, const double* mats,
                          int32_t mats_state_stride, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                          const int32_t* channel, const int32_t* branch, int32_t branch_state_stride, uint64_t seed, const uint32_t*
                          state_index, const uint32_t* trajectory, uint32_t first_gate, qk_built** out);
/* qk_build_mps_channels2: qk_build_mps_channels plus n_channels2, kraus2, n_kraus2 */
int qk_build_mps_channels2(qk_ctx* ctx, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const
                           double* alpha, double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, int32_t
                           n_checkpoints, const int32_t* checkpoints, const qk_built* initial, int32_t initial_snapshot, int32_t n_mats,
                           const double* mats, int32_t mats_state_stride, const int32_t* mat, int32_t n_channels, const double* kraus, const
                           int32_t* n_kraus, const int32_t* channel, const int32_t* branch, int32_t branch_state_stride, uint64_t seed,
                           const uint32_t* state_index, const uint32_t* trajectory, uint32_t first_gate, int32_t n_channels2, const double*
                           kraus2, const int32_t* n_kraus2, qk_built** out);
/* qk_build_mps_conditions: qk_build_mps_channels2 plus cond_gate, cond_mask */
int qk_build_mps_conditions(qk_ctx* ctx, int32_t n_states, int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const
                            double* alpha, double trunc_budget, double value_of_zero, int32_t max_bond, uint32_t flags, int32_t
                            n_checkpoints, const int32_t* checkpoints, const qk_built* initial, int32_t initial_snapshot, int32_t n_mats,
                            const double* mats, int32_t mats_state_stride, const int32_t* mat, int32_t n_channels, const double* kraus,
                            const int32_t* n_kraus, const int32_t* channel, const int32_t* branch, int32_t branch_state_stride, uint64_t
                            seed, const uint32_t* state_index, const uint32_t* trajectory, uint32_t first_gate, int32_t n_channels2, const
                            double* kraus2, const int32_t* n_kraus2, const int32_t* cond_gate, const uint32_t* cond_mask, qk_built** out);
int qk_built_logw_at(const qk_built* built, int32_t j, double* logw /* [n_states] */); /* log-weights at snapshot j (0 without channels) */
int qk_built_num_channel_gates(const qk_built* built);                    /* gates of op codes 10 and 11 of the program */
/* The branch every channel gate took, in program order: [n_states][n_channel_gates]; -1 where a dropped state stopped early, -2
 * where the gate was skipped because its condition was false (qk_build_mps_conditions) */
int qk_built_branches(const qk_built* built, int8_t* branches);
int qk_built_num_snapshots(const qk_built* built);                        /* 1 for qk_build_mps */
int qk_built_checkpoints(const qk_built* built, int32_t* checkpoints);    /* [num_snapshots] gates done at each snapshot */
/* Snapshot j: dims[n_states][n_qubits+1], fidelity so far [n_states], offsets[n_states] into the one heap (complex elements),
 * centre[n_states] (site of the orthogonality centre), complex elements of the snapshot's states together; any may be NULL */
int qk_built_info_at(const qk_built* built, int32_t j, int32_t* dims, double* fidelity, int64_t* offsets, int32_t* centre,
                     int64_t* total_complex);
/* The states of snapshot j, packed back to back in state order (2 * total_complex doubles of qk_built_info_at) */
int qk_built_download_at(const qk_built* built, int32_t j, double* host);
int qk_mps_set_from_built_at(qk_ctx* ctx, const qk_built* built, int32_t j, qk_mps_set** out); /* qk_mps_set_from_built of snapshot j */
/* Building from given states: an fp64 set of this context becomes a qk_built with ONE snapshot of zero gates (qk_built_num_snapshots
 * 1, qk_built_checkpoints [0], no channel gates), from which every build entry above resumes through initial, initial_snapshot = 0.
 * index[s] (NULL: identity, n_states must be the set's) names the set state build state s starts from: the heap holds each set state
 * once, the per-state tables repeat (broadcast, trajectories).
 *   - Verbatim path (qk_mps_set_centre(set) >= 0 and QK_SEED_SWEEP not set): the true-bond corners are copied bit for bit, nothing is
 *     rescaled; fidelity 1, log-weight 0, the centre the recorded one, norms 1 (not computed); qk_built_launch reports zeros.
 *   - Sweep path (any gauge, any norm, bonds <= 512): a finite check (a state with an element that is not finite: QK_EDEVICE naming
 *     the first), the canonical sweep of qk_mps_set_compress with max_bond = 0, max_discard = 0 and value_of_zero (a bond whose rank
 *     is below its dimension shrinks to its rank; the centre ends on the last site), and the last site divided by its Frobenius norm,
 *     which goes to norms (0 or not finite: QK_EDEVICE naming the state).  fidelity is the sweep's; qk_built_launch its grid.
 * norms and fidelity ([set states], may be NULL) are indexed by the SET's states.  QK_EINVAL: a null argument, a set of another context, a
 * complex64 set, n_states < 1, an index entry outside the set, value_of_zero negative or not finite, a bond beyond 512 (sweep path).
 * A bond above a later build's max_bond is refused by that build.                                                                  */
#define QK_SEED_SWEEP 1u /* take the sweep path even where the set records its centre */
int qk_built_from_set(qk_ctx* ctx, const qk_mps_set* set, int32_t n_states, const int32_t* index, double value_of_zero, uint32_t flags,
                      qk_built** out, double* norms, double* fidelity);
/* The orthogonality centre a set records: the common centre of a snapshot of the device builder (qk_mps_set_from_built,
 * qk_mps_set_from_built_at), -1 where the gauge is unknown: every other origin (upload, from_packed, all-gather, to_f32, compress)
 * and a snapshot whose states do not share their centre.                                                                          */
int qk_mps_set_centre(const qk_mps_set* set);
/* Diagnostic: the builder's Jacobi primitive on one host matrix a[p][q] (complex128 row-major, overwritten by A V);
 * v_out[q][q], sig_out[q] = column norms of A V, ord_out[q] = columns by decreasing norm.                          */
int qk_debug_jacobi(qk_ctx* ctx, int32_t p, int32_t q, double* a_inout, double* v_out, double* sig_out, int32_t* ord_out);
/* Diagnostic: the builder's factorisation for matrices beyond its LDS working set -- columns sorted, R by Gram-Schmidt, block
 * Jacobi of R^H on the f64 matrix cores, W = A V -- on one host matrix a[p][q] (16 <= q <= 1024, p <= 1024): a <- W = A V
 * (columns beyond the numerical rank are zero), v_out[q][q], sig_out[q] (0 beyond the rank), ord_out[q] as above;
 * stats_out[6] (may be NULL) = sweeps, then device time in 100 MHz ticks: all, sort + copy, Gram-Schmidt, sweeps, V and W. */
int qk_debug_jacobi_precond(qk_ctx* ctx, int32_t p, int32_t q, double* a_inout, double* v_out, double* sig_out, int32_t* ord_out, int32_t* stats_out);

#ifdef __cplusplus
}
#endif
#endif /* QKGRAM_H */
