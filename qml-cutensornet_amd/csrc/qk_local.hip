// qk_local.hip -- per-qubit reduced density matrices of every state of a set (their Bloch vectors), the two-qubit reduced density
// matrices of neighbouring qubits (their Pauli correlators) and the projected quantum kernel (PQK) Grams built from either.  Part of
// libqkgram.so; entry points qk_local_paulis_host, qk_projected_gram_host, qk_local_pair_paulis_host,
// qk_projected_pair_gram_host and their forms for pairs up to a chosen distance, qk_local_pair_paulis_dist_host and
// qk_projected_pair_gram_dist_host, and the general form, expectation values of Pauli strings and the Gram of any feature columns,
// qk_pauli_strings_host and qk_feature_gram_host, strings of any single-site operators, qk_operator_strings_host, and the entanglement across every bond of a state from the same environments,
// qk_bond_purities_host and qk_bond_spectra_host (definitions above bond_call below), and the block kernels -- reduced-state
// overlaps of the first or last w qubits for every pair of two sets -- qk_block_values_host and qk_block_self_host (definitions
// above BlkSet below), and measurement shots of every state of a set, each shot and qubit in its own Pauli basis, qk_sample_host
// (definitions above SmpArgs below), the amplitudes and outcome likelihoods of given strings, qk_amplitudes_host (above AmpArgs
// below), the reduced density matrices of every window of k qubits, qk_window_rdms_host (above WinArgs
// below), the block overlaps estimated from such shots, qk_shot_block_sums_host (above SbkArgs below), and the
// shot-pair histograms of the classical-shadow kernel, qk_shadow_hist_host (above ShkArgs below), and Pauli strings estimated from
// shots, qk_shot_strings_host (above SstArgs below) (include/qkgram.h).
//
// Definitions (the contract, also in README.md).  For a state psi (site k = qubit k, physical index 0 = |0>, not necessarily
// normalised):
//     rho_k[s][s'] = sum over every other site of psi(..s..) conj(psi(..s'..)) / <psi|psi>
//     F[k] = (<X_k>, <Y_k>, <Z_k>) = (2 Re rho_k[0][1], -2 Im rho_k[0][1], rho_k[0][0] - rho_k[1][1])
//     K_P[j][i] = exp(-g/2 sum_k sum_c (Fx[i][k][c] - Fy[j][k][c])^2)      (= exp(-g sum_k ||rho_k(x_i) - rho_k(y_j)||_F^2))
//
// The local sweep.  A_k = site k of the set as a [a][(s, a')] matrix (split re/im planes, padded bonds), environments in the ring
// sweep's X[ket][bra] orientation (qk_ring.h):
//     L_0 = 1
//     T_k[a][(s, b')]       = sum_b L_k[b][a] A_k[b][(s, b')]                  (the ring sweep's first GEMM with y = x)
//     W_{k,s}[b'][(s', a')] = sum_a T_k[(a, s)][b'] conj(A_k[a][(s', a')])     (s = 0, 1: the T rows of one s, row stride 2 pad(b'))
//     rho_k[s][s']          = sum_{b', a'} W_{k,s}[b'][(s', a')] R_{k+1}[b'][a']
//     L_{k+1}[b'][a']       = W_{k,0}[b'][(0, a')] + W_{k,1}[b'][(1, a')]
//     <psi|psi>             = L_n[0][0]
// The right environments R_k are the left environments of the reversed chain (sites n-1 .. 0, left and right bonds exchanged),
// R_n = 1: a permutation kernel makes that reversed image once per call, the same two-GEMM recurrence runs on it and every R_k
// (k = 1 .. n) is kept.
//
// Work is spread over the chip: ONE launch per step for every state of a batch, ordered by the stream.  The tasks of a GEMM launch
// are (state, 64 x 64 output block), listed by the host from the bond tables; a workgroup computes its block with the ring GEMM
// (zgemm_ring3, fixed K order).  The rho sums are split into 16-row chunks, one workgroup each, with a fixed-order reduction; the
// chunks are added in a fixed order at the end.  No grid-wide barrier, no spin wait, no atomics: a state's features are the same
// bits whatever its batch, its neighbours or the run.
//
// The pair sweep (qk_local_pair_paulis_host).  P_0..P_3 = I, X, Y, Z:
//     rho_{k,k+1}[(s,t)][(s',t')] = sum over every other site of psi(..s,t..) conj(psi(..s',t'..)) / <psi|psi>
//     T[k][p][q] = <P_p on k, P_q on k+1> = sum rho_{k,k+1}[(s,t)][(s',t')] P_p[s'][s] P_q[t'][t]         (k = 0 .. n-2, real)
//     K_2[j][i]  = exp(-g/4 sum_k sum_{p,q} (Tx[i][k][p][q] - Ty[j][k][p][q])^2)   (= exp(-g sum_k ||rho_{k,k+1}(x_i) - rho_{k,k+1}(y_j)||_F^2))
// It is the local sweep with two more GEMMs per site: the mirror image of W at site k+1, open on its physical index,
//     T'_{k+1}[d'][(t, b')]     = sum_c' R_{k+2}[c'][d'] A_{k+1}[b'][t][c']              (the LOC_REV_T shape on the reversed image)
//     V_{k+1,t}[b'][(t', a')]   = sum_d' T'_{k+1}[d'][(t, b')] conj(A_{k+1}[a'][t'][d']) (the LOC_FWD_W shape on the reversed image)
//     rho_{k,k+1}[(s,t)][(s',t')] = sum_{b', a'} W_{k,s}[b'][(s', a')] V_{k+1,t}[b'][(t', a')]
// (R_{k+1} = V_0[.][(0, .)] + V_1[.][(1, .)]).  V is made in the forward pass from the stored R_{k+2}, one site at a time: keeping
// every V of the reverse pass would cost four times the R storage.  The reverse pass and the forward T / W / rho launches are the
// one-qubit sweep's, in its order, so the Bloch vectors and norms of a pair call are the bits qk_local_paulis_host returns.
//
// Pairs up to distance D (qk_local_pair_paulis_dist_host): (k, k+d), d = 1 .. D, listed distance-major,
//     index(d, k) = sum_{e=1}^{d-1} (n - e) + k,     n_pairs = D n - D (D + 1) / 2.
// E_{o->k+1}[s][s'] = W_{o,s}[.][(s', .)] are the four open left environments of qubit o at bond o+1.  Carrying them across a
// site k between the two qubits is the closed transfer step of L, the two GEMMs of the ring sweep:
//     T''[a][(u, b')]          = sum_b E_{o->k}[s][s'][b][a] A_k[b][(u, b')]                 (LOC_DIST_T, the LOC_FWD_T shape)
//     E_{o->k+1}[s][s'][b'][a'] = sum_{(a,u)} T''[(a, u)][b'] conj(A_k[(a, u)][a'])          (LOC_DIST_X: one product over K = 2 chi_k,
//                                                                                          only the u = u' blocks exist)
//     rho_{o,k+1}[(s,t)][(s',t')] = sum_{b', a'} E_{o->k+1}[s][s'][b'][a'] V_{k+1,t}[b'][(t', a')]
// A state keeps a window of D - 1 slots in its scratch, origin o in slot o mod (D - 1), each in W's own layout, so the pair
// reduction reads a slot exactly as it reads W.  At site k, after the neighbour launches: every live origin (k-D+1 .. k-1) goes
// through site k in ONE T-shaped and ONE X-shaped launch (a task's block number also names the origin and (s, s')), then one
// reduction launch makes rho_{o,k+1} of every live origin, then W_k is copied into the slot of the origin whose last distance was
// just used.  The neighbour launches are untouched and come first: the distance-1 block, the Bloch vectors and the norms are the
// bits of the neighbour call for every D, and D = 1 is the neighbour call.
//
// Pauli strings (qk_pauli_strings_host).  A string is c[0 .. n-1], codes 0..3 = I, X, Y, Z, with support [a, b] (its first and last
// non-identity sites); P[s ^ f][s] = i^e(s) as in qk_local_pair_features_kernel:
//     E_a = L_a
//     E_{k+1}[b'][a'] = sum_s i^{e_k(s)} sum_{b,a} E_k[b][a] A_k[b][s][b'] conj(A_k[a][s ^ f_k][a'])        (k = a .. b)
//     value = Re sum_{b', a'} E_{b+1}[b'][a'] R_{b+1}[b'][a'] / L_n[0][0]
// An environment pass per state batch -- the reversed chain and the forward T / W launches of the one-qubit sweep, then L_{k+1} from
// W by the sum the rho kernel makes, so the norms are that sweep's bits -- keeps every R_k and every L_k.  A chain is one
// (state, string) with its own slot (E and the intermediate T).  At site k every live chain (a <= k <= b) of the chain
// batch goes through ONE T-shaped launch (the LOC_DIST_T shape; a chain that starts at k reads the kept L_k in place of its slot),
// ONE elementwise launch over T for the chains whose code at k is not I (T[(a, s ^ f)] <- i^e(s) T[(a, s)]: the product below pairs
// row (a, u) of T with conj(A_k[(a, u)]), so the Pauli costs no matrix work), ONE X-shaped launch (LOC_DIST_X: one product over
// K = 2 chi_k) and, for the chains with b = k, one closing reduction against R_{k+1} in 16-row chunks.  A task's block number also
// names the chain.  4 n_sites launches per chain batch, whatever the number of strings; a string costs work on its support only.  The
// chunk sums of a chain are added in a fixed order and nothing of a chain depends on another chain, so a value is the same bits
// whatever the other states and strings, their order and the cut of the batches (QK_STRINGS_BATCH caps the chains of one).
//
// Strings of single-site operators (qk_operator_strings_host).  The same chain with any 2 x 2 complex matrix at a site: codes
// 1 .. n_ops name the operators O_c[s'][s] of a table that comes with the call, 0 is the identity,
//     E_{k+1}[b'][a'] = sum_{s, s'} O_{c_k}[s'][s] sum_{b,a} E_k[b][a] A_k[b][s][b'] conj(A_k[a][s'][a'])           (k = a .. b)
//     value = sum_{b', a'} E_{b+1}[b'][a'] R_{b+1}[b'][a'] / L_n[0][0]                                              (complex)
// The launches, the tasks, the slots and the cut are those of the Pauli strings (one driver, string_chains); the elementwise launch
// is qk_str_op_kernel (T'[(a, s')] = sum_s O[s'][s] T[(a, s)]) and the closing sum keeps Re and Im (qk_str_closez_kernel,
// qk_str_valuesz_kernel).  QK_OPSTR_BATCH caps the chains of a batch.
//
// The launch kinds, the layout of a state's scratch and of a chain's slot, the pair index, the sizes, the cut into batches and the
// task lists are host-side planning, in qk_local_plan.h (tested on the CPU).  Every entry point runs on one driver: env_sizes,
// env_tables (the batch's tables and the task lists of its plan) and env_run (upload, reverse, init, then the plan on the stream).
// The chain families (strings, block, sample, amplitude, window, MPO) cut the chains of a state batch into chain batches below that:
// chain_stage (qk_local_plan.h) owns the layout of a chain batch's device buffer -- the offsets, the slot bases and the host image
// of its tables, chain_stage_max the room a cut needs behind the state batch -- and chain_run the loop over the chain batches of a
// cut: per batch the family's task lists, the stage, the upload, the family's pointers and launches (each_launch walks a task list
// and skips its empty launches), hipGetLastError, the synchronise.  batch_cap reads a QK_*_BATCH variable.
#include "qk_host.h"
#include "qk_local_plan.h"
#include "qk_ring.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <vector>

namespace {

using namespace qkl;
static_assert(at_L() == 0 && chain_E() == 0, "the kernels address L and a chain's E at the base of the scratch / slot");
static_assert(sizeof(Task2) == sizeof(int2) && offsetof(Task2, x) == offsetof(int2, x) && offsetof(Task2, y) == offsetof(int2, y), "Task2 is the host image of int2");

constexpr int LOC_KTL = 8, LOC_NSLOT = 3;                           // the ring GEMM's fp64 shape (K-tile 8, three 16-KiB slots)
constexpr int LOC_LDS_DOUBLES = LOC_NSLOT * (4 * LOC_KTL * 64);     // 48 KiB
constexpr int LOC_RED_THREADS = 256;                                // workgroup of the rho / L_{k+1} step
constexpr int LOC_PAIR_VALS = 16;                                   // reals of a Hermitian 4 x 4 matrix
struct LocArgs {
  const double* data;     // the set's planes
  const double* rev;      // the reversed image: site o of a state transposed to [pad_{o+1}][2][pad_o], at the set's offset of site o
  const int32_t* dims;    // padded bonds [n_states][n_sites + 1]
  const int32_t* tru;     // true bonds
  const int64_t* offs;    // re-plane offsets [n_states][n_sites]
  const int32_t* states;  // batch entry -> state of the set
  const int32_t* pmax;    // batch entry -> P
  const int64_t* sbase;   // batch entry -> first double of its scratch
  const int64_t* roff;    // [batch][n_sites + 1]: R_k at sbase + rmul P^2 + roff[k]
  const int64_t* loff;    // [batch][n_sites + 1]: the kept L_k at sbase + rmul P^2 + loff[k]; NULL where they are not kept (the local sweeps)
  const int2* tasks;      // this launch: (batch entry, block)
  double* scratch;
  double* part;           // rho partial sums [batch][n_sites][max chunks][4]
  double* part2;          // pair sweep: rho_{k,k+d} partial sums [batch][n_pairs][max chunks][16], pairs in index(d, k) order
  int rmul;
  int max_dist;           // D of the pair sweep (1: neighbours only)
  int n_pairs;
  int n_sites;
  int max_chunks;
  int step;               // reversed-chain step j (LOC_REV_*) or site k (forward, LOC_PAIR_*: the pair (k, k+1))
};

__device__ __forceinline__ long long uni64(const long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// One 64 x 64 output block of one state's GEMM of this step.  CONJB: the LOC_REV_X / LOC_FWD_W / LOC_PAIR_V / LOC_DIST_X products (conjugated site tensor).
template <bool CONJB>
__global__ __launch_bounds__(512) void qk_local_gemm_kernel(const LocArgs g, const int kind) {
  __shared__ __attribute__((aligned(16))) double lds[LOC_LDS_DOUBLES];
  const int2 t = g.tasks[blockIdx.x];
  const int i = __builtin_amdgcn_readfirstlane(t.x);
  int blk = __builtin_amdgcn_readfirstlane(t.y);
  const int n = g.n_sites, n1 = n + 1;
  const long long st = __builtin_amdgcn_readfirstlane(g.states[i]);
  const int* pd = g.dims + st * n1;
  const int* td = g.tru + st * n1;
  const long long P = __builtin_amdgcn_readfirstlane(g.pmax[i]);
  double* const S = g.scratch + uni64(g.sbase[i]);
  const long long P2 = P * P;
  double* const Tre = S + at_T() * P2;
  const long long tpl = 2 * P2;  // T and W planes
  const double *Are, *Aim, *Bre, *Bim;
  double *Cre, *Cim;
  int lda, ldb, ldc, M, N, K;
  if (kind == LOC_BOND_M) {  // M_k[a][a'] = sum_b L_k[b][a] R_k[b][a'] over the true bond
    const int k = g.step;
    const int pk = __builtin_amdgcn_readfirstlane(pd[k]);
    Are = S + g.rmul * P2 + uni64(g.loff[(long long)i * n1 + k]);
    Aim = Are + (long long)pk * pk;
    Bre = S + g.rmul * P2 + uni64(g.roff[(long long)i * n1 + k]);
    Bim = Bre + (long long)pk * pk;
    Cre = Tre, Cim = Tre + tpl;
    lda = pk, ldb = pk, ldc = pk, M = pk, N = pk, K = __builtin_amdgcn_readfirstlane(td[k]);
  } else if (kind == LOC_REV_T || kind == LOC_REV_X || kind == LOC_PAIR_T || kind == LOC_PAIR_V) {
    const int o = (kind == LOC_REV_T || kind == LOC_REV_X) ? n - 1 - g.step : g.step + 1;
    const int al = __builtin_amdgcn_readfirstlane(pd[o + 1]), ar = __builtin_amdgcn_readfirstlane(pd[o]);
    const int at = __builtin_amdgcn_readfirstlane(td[o + 1]);
    Bre = g.rev + uni64(g.offs[st * n + o]);
    Bim = Bre + (long long)al * 2 * ar;
    if (kind == LOC_REV_T || kind == LOC_PAIR_T) {
      Are = S + g.rmul * P2 + uni64(g.roff[(long long)i * n1 + o + 1]);
      Aim = Are + (long long)al * al;
      Cre = (kind == LOC_REV_T) ? Tre : S + at_Tp() * P2, Cim = Cre + tpl;
      lda = al, ldb = 2 * ar, ldc = 2 * ar, M = al, N = 2 * ar, K = at;
    } else if (kind == LOC_PAIR_V) {
      M = ar, N = 2 * ar;
      const int t = blk >= ((M + 63) / 64) * ((N + 63) / 64);
      Are = S + at_Tp() * P2 + t * ar, Aim = Are + tpl;
      Cre = S + at_V(t) * P2, Cim = Cre + tpl;
      lda = 2 * ar, ldb = 2 * ar, ldc = 2 * ar, K = at;
    } else {
      Are = Tre, Aim = Tre + tpl;
      Cre = S + g.rmul * P2 + uni64(g.roff[(long long)i * n1 + o]);
      Cim = Cre + (long long)ar * ar;
      lda = ar, ldb = ar, ldc = ar, M = ar, N = ar, K = 2 * at;
    }
  } else {
    const int k = g.step;
    const int l = __builtin_amdgcn_readfirstlane(pd[k]), r = __builtin_amdgcn_readfirstlane(pd[k + 1]);
    const int lt = __builtin_amdgcn_readfirstlane(td[k]);
    Bre = g.data + uni64(g.offs[st * n + k]);
    Bim = Bre + (long long)l * 2 * r;
    if (kind == LOC_DIST_T || kind == LOC_DIST_X) {
      // block number = (w, block of the product), w = 4 (k - 1 - o) + 2s + s' for the live origin o
      const int per = (kind == LOC_DIST_T) ? ((l + 63) / 64) * ((2 * r + 63) / 64) : ((r + 63) / 64) * ((r + 63) / 64);
      const int w = blk / per, o = k - 1 - (w >> 2), s = (w >> 1) & 1, sp = w & 1;
      double* const E = S + window_slot(o, g.max_dist) * P2 + s * 2 * tpl;  // E[s][.][(s', .)] of origin o
      double* const Tw = S + window_tmp(w, g.max_dist) * P2;
      blk -= w * per;
      if (kind == LOC_DIST_T) {
        Are = E + sp * l, Aim = Are + tpl;
        Cre = Tw, Cim = Tw + tpl;
        lda = 2 * l, ldb = 2 * r, ldc = 2 * r, M = l, N = 2 * r, K = lt;
      } else {
        Are = Tw, Aim = Tw + tpl;
        Cre = E + sp * r, Cim = Cre + tpl;
        lda = r, ldb = r, ldc = 2 * r, M = r, N = r, K = 2 * lt;
      }
    } else if (kind == LOC_FWD_T) {
      Are = S, Aim = S + P2;
      Cre = Tre, Cim = Tre + tpl;
      lda = l, ldb = 2 * r, ldc = 2 * r, M = l, N = 2 * r, K = lt;
    } else {
      M = r, N = 2 * r;
      const int per_s = ((M + 63) / 64) * ((N + 63) / 64);
      const int s = blk >= per_s;
      Are = Tre + s * r, Aim = Are + tpl;
      Cre = S + at_W(s) * P2, Cim = Cre + tpl;
      lda = 2 * r, ldb = 2 * r, ldc = 2 * r, K = lt;
    }
  }
  const int npm = (M + 63) / 64;
  const int b = (kind == LOC_FWD_W || kind == LOC_PAIR_V) ? blk % (npm * ((N + 63) / 64)) : blk;
  const int m0 = 64 * (b % npm), n0 = 64 * (b / npm);
  zgemm_ring3<CONJB, LOC_KTL, LOC_NSLOT, true, 8, 64, double, 7>(Cre + (long long)m0 * ldc + n0, Cim + (long long)m0 * ldc + n0, ldc, Are + m0, Aim + m0, lda,
                                                                  Bre + n0, Bim + n0, ldb, min(64, M - m0), min(64, N - n0), K, lds);
}

// The sum of NV values per thread over the 256 threads of a workgroup, into red[v][0]: a fixed-order tree, halving from 128, the
// same order whatever NV, so a result is the same bits as when each reduction kernel wrote its own loop.
// LDS: red[NV][256] doubles -- 32 KiB at NV = 16 (qk_local_pair_rho_kernel), five workgroups (20 waves) per CU: that kernel waits on
// its 16 global loads per element, not on occupancy.  Every access is red[v][thread]: the 32 lanes that a ds_read_b64 /
// ds_write_b64 serves together touch 32 consecutive doubles, each of the 64 banks once, so the layout is conflict-free for every NV.
template <int NV>
__device__ __forceinline__ void tree_sum(double (&red)[NV][LOC_RED_THREADS], const double (&acc)[NV]) {
  for (int v = 0; v < NV; ++v) red[v][threadIdx.x] = acc[v];
  __syncthreads();
  for (int h = LOC_RED_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h)
      for (int v = 0; v < NV; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
    __syncthreads();
  }
}

// rho_k partial sums of one 16-row chunk of b' and the same rows of L_{k+1} = W_0[.][(0, .)] + W_1[.][(1, .)].
// part[(i, k, chunk)] = (Re rho00, Re rho11, Re rho01, Im rho01), unnormalised.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_local_rho_kernel(const LocArgs g) {
  __shared__ double red[4][LOC_RED_THREADS];
  const int2 t = g.tasks[blockIdx.x];
  const int i = t.x, c = t.y;
  const int n = g.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.states[i];
  const int r = g.dims[st * n1 + k + 1];
  const long long P = g.pmax[i], P2 = P * P, tpl = 2 * P2;
  double* const S = g.scratch + g.sbase[i];
  const double* W0 = S + at_W(0) * P2;
  const double* W1 = S + at_W(1) * P2;
  const double* R = S + g.rmul * P2 + g.roff[(long long)i * n1 + k + 1];
  const long long rpl = (long long)r * r;
  double a00 = 0, a11 = 0, a01r = 0, a01i = 0;
  const int rows = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < rows; e += LOC_RED_THREADS) {
    const int bp = c * LOC_CHUNK + e / r, ap = e % r;
    const long long w = (long long)bp * 2 * r + ap;
    const double w00r = W0[w], w00i = W0[w + tpl], w01r = W0[w + r], w01i = W0[w + r + tpl];
    const double w11r = W1[w + r], w11i = W1[w + r + tpl];
    const long long q = (long long)bp * r + ap;
    const double rr = R[q], ri = R[q + rpl];
    a00 += w00r * rr - w00i * ri;
    a11 += w11r * rr - w11i * ri;
    a01r += w01r * rr - w01i * ri;
    a01i += w01r * ri + w01i * rr;
    S[q] = w00r + w11r;  // L_{k+1}[b'][a'], ld r
    S[q + P2] = w00i + w11i;
  }
  const double acc[4] = {a00, a11, a01r, a01i};
  tree_sum(red, acc);
  if (threadIdx.x < 4) g.part[(((long long)i * n + k) * g.max_chunks + c) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// rho_{k,k+1} partial sums of one 16-row chunk of b': the products W_{k,s}[b'][(s', a')] V_{k+1,t}[b'][(t', a')] over the chunk's
// rows and every a'.  The matrix is Hermitian (row 2s + t, column 2s' + t'), so a chunk keeps its 16 reals, unnormalised:
//     part2[(i, k, chunk)] = Re rho[0][0], [1][1], [2][2], [3][3], then (Re, Im) of rho[0][1], [0][2], [0][3], [1][2], [1][3], [2][3]
// The 16 sums go through tree_sum (red[16][256] doubles of LDS).
// DIST: the pairs (o, k+1) of the live origins o = k-1, k-2, ..: a task is (batch entry, (k - 1 - o) chunks + chunk) and the left
// operand is the origin's window slot, which has W's layout; the LDS layout, the accesses and the tree are the same for both forms.
template <bool DIST>
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_local_pair_rho_kernel(const LocArgs g) {
  __shared__ double red[LOC_PAIR_VALS][LOC_RED_THREADS];
  const int2 t = g.tasks[blockIdx.x];
  const int i = t.x;
  const int n = g.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.states[i];
  const int r = g.dims[st * n1 + k + 1];
  const int age = DIST ? t.y / (r / LOC_CHUNK) : 0, c = t.y - age * (r / LOC_CHUNK);
  const long long P = g.pmax[i], P2 = P * P, tpl = 2 * P2;
  const double* const S = g.scratch + g.sbase[i];
  const double* const W0 = S + (DIST ? window_slot(k - 1 - age, g.max_dist) : at_W(0)) * P2;
  const double* W[2] = {W0, W0 + 2 * tpl};
  const double* V[2] = {S + at_V(0) * P2, S + at_V(1) * P2};
  double acc[LOC_PAIR_VALS] = {};
  const int rows = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < rows; e += LOC_RED_THREADS) {
    const int bp = c * LOC_CHUNK + e / r, ap = e % r;
    const long long w = (long long)bp * 2 * r + ap;
    double wr[2][2], wi[2][2], vr[2][2], vi[2][2];  // [s][s'] and [t][t']
    for (int s = 0; s < 2; ++s)
      for (int sp = 0; sp < 2; ++sp) {
        wr[s][sp] = W[s][w + sp * r], wi[s][sp] = W[s][w + sp * r + tpl];
        vr[s][sp] = V[s][w + sp * r], vi[s][sp] = V[s][w + sp * r + tpl];
      }
    int m = 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b) {
        const int s = a >> 1, tt = a & 1, sp = b >> 1, tp = b & 1;
        const double re = wr[s][sp] * vr[tt][tp] - wi[s][sp] * vi[tt][tp];
        if (a == b) {
          acc[a] += re;
        } else {
          acc[m] += re;
          acc[m + 1] += wr[s][sp] * vi[tt][tp] + wi[s][sp] * vr[tt][tp];
          m += 2;
        }
      }
  }
  tree_sum(red, acc);
  const long long pi = DIST ? pair_index(age + 2, k - 1 - age, n) : k;  // the pair (o, k+1) of origin o = k - 1 - age
  if (threadIdx.x < LOC_PAIR_VALS)
    g.part2[(((long long)i * g.n_pairs + pi) * g.max_chunks + c) * LOC_PAIR_VALS + threadIdx.x] = red[threadIdx.x][0];
}

// W_k = (W_0 | W_1) of site k, rows b' of one 16-row chunk, into window slot k mod (D - 1): the new origin of the distant pairs.
// Both have the same layout, so it is a plain copy of the rows' 2 pad(b') columns in the four planes.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_local_admit_kernel(const LocArgs g) {
  const int2 t = g.tasks[blockIdx.x];
  const int i = t.x, c = t.y;
  const int n1 = g.n_sites + 1, k = g.step;
  const long long st = g.states[i];
  const int r = g.dims[st * n1 + k + 1];
  const long long P = g.pmax[i], P2 = P * P;
  double* const S = g.scratch + g.sbase[i];
  const double* const W = S + at_W(0) * P2;
  double* const E = S + window_slot(k, g.max_dist) * P2;
  const long long row0 = (long long)c * LOC_CHUNK * 2 * r;
  const int cnt = LOC_CHUNK * 2 * r;
  for (int e = threadIdx.x; e < cnt; e += LOC_RED_THREADS)
    for (int pl = 0; pl < 4; ++pl) E[pl * 2 * P2 + row0 + e] = W[pl * 2 * P2 + row0 + e];
}

// L_0 = 1 and R_n = 1 (16 x 16, [0][0] = 1) of every state of the batch, and the kept L_0 where the L_k are kept.
__global__ __launch_bounds__(256) void qk_local_init_kernel(const LocArgs g, const int nb) {
  const int i = blockIdx.x;
  if (i >= nb) return;
  const long long P = g.pmax[i], P2 = P * P;
  double* const S = g.scratch + g.sbase[i];
  double* const Rn = S + g.rmul * P2 + g.roff[(long long)i * (g.n_sites + 1) + g.n_sites];
  const int e = threadIdx.x;  // 256 = 16 x 16
  const double v = (e == 0) ? 1.0 : 0.0;
  S[e] = v, S[P2 + e] = 0.0;
  Rn[e] = v, Rn[256 + e] = 0.0;
  if (g.loff) {
    double* const L0 = S + g.rmul * P2 + g.loff[(long long)i * (g.n_sites + 1)];
    L0[e] = v, L0[256 + e] = 0.0;
  }
}

// The reversed image of the batch's states: site o of state st, [a][s][b] -> [b][s][a] in both planes, at the same offset.
__global__ __launch_bounds__(256) void qk_local_reverse_kernel(const LocArgs g, double* rev) {
  const int i = blockIdx.x, o = blockIdx.y, n = g.n_sites, n1 = n + 1;
  const long long st = g.states[i];
  const int l = g.dims[st * n1 + o], r = g.dims[st * n1 + o + 1];
  const long long off = g.offs[st * n + o], pl = (long long)l * 2 * r;
  const double* src = g.data + off;
  double* dst = rev + off;
  for (long long e = threadIdx.x; e < 2 * pl; e += 256) {
    const long long p = e >= pl, f = e - p * pl;
    const int a = (int)(f / (2 * r)), rem = (int)(f % (2 * r)), s = rem / r, bb = rem % r;
    dst[p * pl + (long long)bb * 2 * l + s * l + a] = src[e];
  }
}

// Bloch vectors and norms: the chunk sums of each (state, site) in a fixed order, normalised by L_n[0][0].
__global__ __launch_bounds__(256) void qk_local_features_kernel(const LocArgs g, const int nb, double* out, double* norms) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n = g.n_sites, n1 = n + 1;
  if (id >= (long long)nb * n) return;
  const int i = (int)(id / n), k = (int)(id % n);
  const long long st = g.states[i];
  const double nrm = g.scratch[g.sbase[i]];  // L_n[0][0]
  const int chunks = g.dims[st * n1 + k + 1] / LOC_CHUNK;
  const double* p = g.part + ((long long)i * n + k) * g.max_chunks * 4;
  double a00 = 0, a11 = 0, a01r = 0, a01i = 0;
  for (int c = 0; c < chunks; ++c) a00 += p[4 * c], a11 += p[4 * c + 1], a01r += p[4 * c + 2], a01i += p[4 * c + 3];
  double* f = out + (st * n + k) * 3;
  f[0] = 2.0 * a01r / nrm;
  f[1] = -2.0 * a01i / nrm;
  f[2] = (a00 - a11) / nrm;
  if (norms && k == 0) norms[st] = nrm;
}

// Pauli correlators of the pairs (neighbours, or every pair up to distance D): the chunk sums of each (state, pair) in a fixed order, then
//     T[p][q] = sum_{s,t} rho[(s,t)][(s ^ f_p, t ^ f_q)] i^(e_p(s) + e_q(t)) / L_n[0][0]
// -- a Pauli matrix has one entry per column: P_p[s ^ f_p][s] = i^e_p(s), f = (0, 1, 1, 0), e_I = e_X = (0, 0), e_Y = (1, 3),
// e_Z = (0, 2); the imaginary parts cancel between (s, t) and its image, so only Re is summed.  T[0][0] is written as exactly 1.
__global__ __launch_bounds__(256) void qk_local_pair_features_kernel(const LocArgs g, const int nb, double* out) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n = g.n_sites, n1 = n + 1, np = g.n_pairs;
  if (id >= (long long)nb * np) return;
  const int i = (int)(id / np), k = (int)(id % np);  // k = index(d, o) of the pair (o, o + d)
  const long long st = g.states[i];
  const double nrm = g.scratch[g.sbase[i]];  // L_n[0][0]
  const int chunks = g.dims[st * n1 + pair_second(k, n)] / LOC_CHUNK;  // the partial sums are over the chunks of the second qubit's left bond
  const double* p = g.part2 + ((long long)i * np + k) * g.max_chunks * LOC_PAIR_VALS;
  double v[LOC_PAIR_VALS] = {};
  for (int c = 0; c < chunks; ++c)
    for (int e = 0; e < LOC_PAIR_VALS; ++e) v[e] += p[LOC_PAIR_VALS * c + e];
  double re[4][4], im[4][4];
  int m = 4;
  for (int a = 0; a < 4; ++a) {
    re[a][a] = v[a], im[a][a] = 0.0;
    for (int b = a + 1; b < 4; ++b, m += 2) re[a][b] = re[b][a] = v[m], im[a][b] = v[m + 1], im[b][a] = -v[m + 1];
  }
  double* f = out + (st * np + k) * 16;
  for (int pp = 0; pp < 4; ++pp)
    for (int q = 0; q < 4; ++q) {
      const int fp = (pp == 1 || pp == 2), fq = (q == 1 || q == 2);
      double acc = 0.0;
      for (int s = 0; s < 2; ++s)
        for (int t = 0; t < 2; ++t) {
          const int ep = (pp == 2) ? 1 + 2 * s : (pp == 3) ? 2 * s : 0, eq = (q == 2) ? 1 + 2 * t : (q == 3) ? 2 * t : 0;
          const int a = 2 * s + t, b = 2 * (s ^ fp) + (t ^ fq), e = (ep + eq) & 3;
          acc += (e == 0) ? re[a][b] : (e == 1) ? -im[a][b] : (e == 2) ? -re[a][b] : im[a][b];
        }
      f[4 * pp + q] = (pp == 0 && q == 0) ? 1.0 : acc / nrm;
    }
}

// The PQK Gram: K[j][i] = exp(-g/2 sum_d (fx[i][d] - fy[j][d])^2), d = 3 n_sites (pair form: -g/4, d = 16 (n_sites - 1)).  A 64 x 64 tile per workgroup (4 x 4 entries per
// thread), features staged in LDS in 32-wide slices of d.  Each entry adds its d terms in ascending order into one accumulator: the
// differences of (i, j) and (j, i) are negatives of each other, so a symmetric Gram is exactly symmetric and its diagonal exactly 1.
constexpr int PG_T = 64, PG_D = 32;
__global__ __launch_bounds__(256) void qk_projected_gram_kernel(const double* fx, int nx, const double* fy, int ny, int D, double half_g, double* K, long long ld) {
  __shared__ double sx[PG_D][PG_T + 1], sy[PG_D][PG_T + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.x * PG_T, j0 = blockIdx.y * PG_T;
  double acc[4][4] = {};
  for (int d0 = 0; d0 < D; d0 += PG_D) {
    for (int e = threadIdx.x; e < PG_T * PG_D; e += 256) {
      const int row = e / PG_D, d = e % PG_D;
      const bool dv = d0 + d < D;
      sx[d][row] = (dv && i0 + row < nx) ? fx[(long long)(i0 + row) * D + d0 + d] : 0.0;
      sy[d][row] = (dv && j0 + row < ny) ? fy[(long long)(j0 + row) * D + d0 + d] : 0.0;
    }
    __syncthreads();
    const int dn = min(PG_D, D - d0);
    for (int d = 0; d < dn; ++d) {
      double xv[4], yv[4];
      for (int u = 0; u < 4; ++u) xv[u] = sx[d][tx + 16 * u], yv[u] = sy[d][ty + 16 * u];
      for (int a = 0; a < 4; ++a)
        for (int u = 0; u < 4; ++u) {
          const double diff = xv[u] - yv[a];
          acc[a][u] = __fma_rn(diff, diff, acc[a][u]);
        }
    }
    __syncthreads();
  }
  for (int a = 0; a < 4; ++a)
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + tx + 16 * u, j = j0 + ty + 16 * a;
      if (i < nx && j < ny) K[(long long)j * ld + i] = exp(-half_g * acc[a][u]);
    }
}

// The PQK Gram of host feature arrays [n][D]: out[j * ld + i] = exp(-factor sum_d (fx[i][d] - fy[j][d])^2).
int projected_gram(qk_ctx* c, const char* what, const char* range, int32_t n_sites, int min_sites, int D, double factor, int32_t nx, const double* fx,
                   int32_t ny, const double* fy, double g, double* out, int64_t ld) {
  if (!c || !fx || !out) return qk_fail(QK_EINVAL, "%s: null argument", what);
  if (n_sites < min_sites) return qk_fail(QK_EINVAL, "%s: n_sites must be >= %d (got %d)", what, min_sites, n_sites);
  if (nx < 1 || ny < 1) return qk_fail(QK_EINVAL, "%s: empty feature set (nx %d, ny %d)", what, nx, ny);
  if (!fy && ny != nx) return qk_fail(QK_EINVAL, "%s: Y is X (fy NULL) but ny %d != nx %d", what, ny, nx);
  if (!(g > 0.0) || !std::isfinite(g)) return qk_fail(QK_EINVAL, "%s: g must be > 0 and finite (got %g)", what, g);
  if (ld < nx) return qk_fail(QK_EINVAL, "%s: ld %lld is smaller than the %d columns", what, (long long)ld, nx);
  QkRangeGuard range_(range);
  HIP_TRY_AS(what, hipSetDevice(c->device));
  const size_t bx = (size_t)nx * D * sizeof(double), by = fy ? (size_t)ny * D * sizeof(double) : 0, bk = (size_t)ny * nx * sizeof(double);
  QkDevBuf buf;
  HIP_TRY_AS(what, buf.alloc(bx + by + bk));
  double* dx = buf.get<double>();
  double* dy = fy ? dx + (size_t)nx * D : dx;
  double* dk = dx + (size_t)nx * D + (fy ? (size_t)ny * D : 0);
  HIP_TRY_AS(what, hipMemcpyAsync(dx, fx, bx, hipMemcpyHostToDevice, c->stream));
  if (fy) HIP_TRY_AS(what, hipMemcpyAsync(dy, fy, by, hipMemcpyHostToDevice, c->stream));
  qk_projected_gram_kernel<<<dim3((nx + PG_T - 1) / PG_T, (ny + PG_T - 1) / PG_T), dim3(256), 0, c->stream>>>(dx, nx, dy, ny, D, factor * g, dk, nx);
  HIP_TRY_AS(what, hipGetLastError());
  HIP_TRY_AS(what, hipMemcpy2DAsync(out, (size_t)ld * sizeof(double), dk, (size_t)nx * sizeof(double), (size_t)nx * sizeof(double), (size_t)ny, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  return QK_OK;
}

// ---- Pauli strings (qk_pauli_strings_host) ------------------------------------------------------------------------------------
// A chain is one (state, string) with a non-identity site; its support is [a, b].  Its slot is laid out in qk_local_plan.h.
struct StrArgs {
  LocArgs e;              // the set and the state batch of the environment pass: e.scratch holds the sweep planes, every R_k, every L_k
  const int32_t* cent;    // chain -> batch entry
  const int32_t* cstr;    // chain -> string
  const int64_t* cbase;   // chain -> first double of its slot
  const uint8_t* strings; // [n_strings][n_sites]
  const int32_t* supp;    // [n_strings][2]: a, b
  const int2* tasks;      // this launch: (chain, block)
  double* slots;
  double* part;           // closing partial sums [chain][max chunks]
  int step;               // site k
};

// One 64 x 64 output block of one chain's GEMM at site k.  CONJB = false: STR_T, true: STR_X.
template <bool CONJB>
__global__ __launch_bounds__(512) void qk_str_gemm_kernel(const StrArgs g) {
  __shared__ __attribute__((aligned(16))) double lds[LOC_LDS_DOUBLES];
  const int2 t = g.tasks[blockIdx.x];
  const int ch = __builtin_amdgcn_readfirstlane(t.x);
  const int blk = __builtin_amdgcn_readfirstlane(t.y);
  const int i = __builtin_amdgcn_readfirstlane(g.cent[ch]);
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = __builtin_amdgcn_readfirstlane(g.e.states[i]);
  const int l = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k]), r = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k + 1]);
  const int lt = __builtin_amdgcn_readfirstlane(g.e.tru[st * n1 + k]);
  const long long P = __builtin_amdgcn_readfirstlane(g.e.pmax[i]), P2 = P * P;
  double* const E = g.slots + uni64(g.cbase[ch]);
  double* const T = E + chain_T() * P2;
  const double* Bre = g.e.data + uni64(g.e.offs[st * n + k]);
  const double* Bim = Bre + (long long)l * 2 * r;
  const double *Are, *Aim;
  double *Cre, *Cim;
  int lda, ldb, ldc, M, N, K;
  if (!CONJB) {
    const int a = __builtin_amdgcn_readfirstlane(g.supp[2 * __builtin_amdgcn_readfirstlane(g.cstr[ch])]);
    if (a == k) {  // the chain starts here: E_a = L_a
      Are = g.e.scratch + uni64(g.e.sbase[i]) + g.e.rmul * P2 + uni64(g.e.loff[(long long)i * n1 + k]);
      Aim = Are + (long long)l * l;
    } else {
      Are = E, Aim = E + P2;
    }
    Cre = T, Cim = T + 2 * P2;
    lda = l, ldb = 2 * r, ldc = 2 * r, M = l, N = 2 * r, K = lt;
  } else {
    Are = T, Aim = T + 2 * P2;
    Cre = E, Cim = E + P2;
    lda = r, ldb = r, ldc = r, M = r, N = r, K = 2 * lt;
  }
  const int npm = (M + 63) / 64;
  const int m0 = 64 * (blk % npm), n0 = 64 * (blk / npm);
  zgemm_ring3<CONJB, LOC_KTL, LOC_NSLOT, true, 8, 64, double, 8>(Cre + (long long)m0 * ldc + n0, Cim + (long long)m0 * ldc + n0, ldc, Are + m0, Aim + m0, lda,
                                                                  Bre + n0, Bim + n0, ldb, min(64, M - m0), min(64, N - n0), K, lds);
}

// The Pauli of site k on the ket index of T, in place, rows a of one 16-row chunk: P[s ^ f][s] = i^e(s), so the row (a, s ^ f)
// that the X-shaped product pairs with conj(A_k[(a, s ^ f)]) becomes i^e(s) T[(a, s)].  X: the halves swap; Y: (T_0, T_1) <-
// (-i T_1, i T_0); Z: T_1 <- -T_1.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_str_pauli_kernel(const StrArgs g) {
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const int i = g.cent[ch], m = g.cstr[ch];
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.e.states[i];
  const int r = g.e.dims[st * n1 + k + 1];
  const int code = g.strings[(long long)m * n + k];
  const long long P = g.e.pmax[i], P2 = P * P, tpl = 2 * P2;
  double* const T = g.slots + g.cbase[ch] + chain_T() * P2;
  const int cnt = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < cnt; e += LOC_RED_THREADS) {
    const long long q0 = (long long)(c * LOC_CHUNK + e / r) * 2 * r + e % r, q1 = q0 + r;
    const double r0 = T[q0], i0 = T[q0 + tpl], r1 = T[q1], i1 = T[q1 + tpl];
    const bool x = code == 1, y = code == 2;
    T[q0] = x ? r1 : y ? i1 : r0;
    T[q0 + tpl] = x ? i1 : y ? -r1 : i0;
    T[q1] = x ? r0 : y ? -i0 : -r1;
    T[q1 + tpl] = x ? i0 : y ? r0 : -i1;
  }
}

// Re sum_{b', a'} E_{b+1}[b'][a'] R_{b+1}[b'][a'] over one 16-row chunk of b', unnormalised: part[(chain, chunk)].
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_str_close_kernel(const StrArgs g) {
  __shared__ double red[1][LOC_RED_THREADS];
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const int i = g.cent[ch];
  const int n1 = g.e.n_sites + 1, k = g.step;
  const long long st = g.e.states[i];
  const int r = g.e.dims[st * n1 + k + 1];
  const long long P = g.e.pmax[i], P2 = P * P, rpl = (long long)r * r;
  const double* const E = g.slots + g.cbase[ch];
  const double* const R = g.e.scratch + g.e.sbase[i] + g.e.rmul * P2 + g.e.roff[(long long)i * n1 + k + 1];
  double acc[1] = {};
  const int rows = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < rows; e += LOC_RED_THREADS) {
    const long long q = (long long)c * rows + e;
    acc[0] += E[q] * R[q] - E[q + P2] * R[q + rpl];
  }
  tree_sum(red, acc);
  if (threadIdx.x == 0) g.part[(long long)ch * g.e.max_chunks + c] = red[0][0];
}

// Environment pass, rows b' of one 16-row chunk: L_{k+1} = W_0[.][(0, .)] + W_1[.][(1, .)] -- the sum qk_local_rho_kernel makes,
// so L_n[0][0] is that sweep's norm bit for bit -- into the sweep's L plane and, for k + 1 < n_sites, into the kept L_{k+1}.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_str_lnext_kernel(const LocArgs g) {
  const int2 t = g.tasks[blockIdx.x];
  const int i = t.x, c = t.y;
  const int n = g.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.states[i];
  const int r = g.dims[st * n1 + k + 1];
  const long long P = g.pmax[i], P2 = P * P, tpl = 2 * P2, rpl = (long long)r * r;
  double* const S = g.scratch + g.sbase[i];
  const double* W0 = S + at_W(0) * P2;
  const double* W1 = S + at_W(1) * P2;
  double* const Lk = (k + 1 < n) ? S + g.rmul * P2 + g.loff[(long long)i * n1 + k + 1] : nullptr;
  const int rows = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < rows; e += LOC_RED_THREADS) {
    const int bp = c * LOC_CHUNK + e / r, ap = e % r;
    const long long w = (long long)bp * 2 * r + ap, q = (long long)bp * r + ap;
    const double re = W0[w] + W1[w + r], im = W0[w + tpl] + W1[w + r + tpl];
    S[q] = re, S[q + P2] = im;
    if (Lk) Lk[q] = re, Lk[q + rpl] = im;
  }
}

__global__ __launch_bounds__(256) void qk_str_norms_kernel(const LocArgs g, const int nb, double* norms) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nb) norms[g.states[i]] = g.scratch[g.sbase[i]];  // L_n[0][0]
}

// The values of a chain batch: the chunk sums of each chain in a fixed order, normalised by L_n[0][0].
__global__ __launch_bounds__(256) void qk_str_values_kernel(const StrArgs g, const int nc, const int n_strings, double* out) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= nc) return;
  const int i = g.cent[ch], m = g.cstr[ch];
  const long long st = g.e.states[i];
  const int chunks = g.e.dims[st * (g.e.n_sites + 1) + g.supp[2 * m + 1] + 1] / LOC_CHUNK;
  const double* p = g.part + (long long)ch * g.e.max_chunks;
  double v = 0;
  for (int c = 0; c < chunks; ++c) v += p[c];
  out[st * n_strings + m] = v / g.e.scratch[g.e.sbase[i]];
}

// ---- strings of single-site operators (qk_operator_strings_host) ------------------------------------------------------------------
// The chain of the Pauli strings with a general 2 x 2 complex matrix at a site and a complex closing sum.
struct OpArgs {
  StrArgs s;
  const double* ops;  // [n_ops][2][2][2]: (re, im) of O_c[s'][s], c = code - 1
};

// The operator of site k on the ket index of T, in place, rows a of one 16-row chunk: T'[(a, s')] = sum_s O[s'][s] T[(a, s)], both
// halves of a row pair read, then both written.  Each component is one chain of fused multiply-adds in the written order (s = 0
// before s = 1, the imaginary factor before the real one), so it is the same bits wherever the chain runs.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_str_op_kernel(const OpArgs a) {
  const StrArgs& g = a.s;
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const int i = g.cent[ch], m = g.cstr[ch];
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.e.states[i];
  const int r = g.e.dims[st * n1 + k + 1];
  const int code = g.strings[(long long)m * n + k];  // 1 .. n_ops: a chain has a task here only where its code is not 0
  const double* const o = a.ops + 8 * (code - 1);
  const double ar = o[0], ai = o[1], br = o[2], bi = o[3], cr = o[4], ci = o[5], dr = o[6], di = o[7];  // O = [[a, b], [c, d]]
  const long long P = g.e.pmax[i], P2 = P * P, tpl = 2 * P2;
  double* const T = g.slots + g.cbase[ch] + chain_T() * P2;
  const int cnt = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < cnt; e += LOC_RED_THREADS) {
    const long long q0 = (long long)(c * LOC_CHUNK + e / r) * 2 * r + e % r, q1 = q0 + r;
    const double r0 = T[q0], i0 = T[q0 + tpl], r1 = T[q1], i1 = T[q1 + tpl];
    T[q0] = fma(br, r1, fma(-bi, i1, fma(ar, r0, -(ai * i0))));
    T[q0 + tpl] = fma(br, i1, fma(bi, r1, fma(ar, i0, ai * r0)));
    T[q1] = fma(dr, r1, fma(-di, i1, fma(cr, r0, -(ci * i0))));
    T[q1 + tpl] = fma(dr, i1, fma(di, r1, fma(cr, i0, ci * r0)));
  }
}

// sum_{b', a'} E_{b+1}[b'][a'] R_{b+1}[b'][a'] over one 16-row chunk of b', Re and Im, unnormalised: part[(chain, chunk)][2].  The
// order of the sum is qk_str_close_kernel's.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_str_closez_kernel(const OpArgs a) {
  __shared__ double red[2][LOC_RED_THREADS];
  const StrArgs& g = a.s;
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const int i = g.cent[ch];
  const int n1 = g.e.n_sites + 1, k = g.step;
  const long long st = g.e.states[i];
  const int r = g.e.dims[st * n1 + k + 1];
  const long long P = g.e.pmax[i], P2 = P * P, rpl = (long long)r * r;
  const double* const E = g.slots + g.cbase[ch];
  const double* const R = g.e.scratch + g.e.sbase[i] + g.e.rmul * P2 + g.e.roff[(long long)i * n1 + k + 1];
  double acc[2] = {};
  const int rows = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < rows; e += LOC_RED_THREADS) {
    const long long q = (long long)c * rows + e;
    acc[0] += E[q] * R[q] - E[q + P2] * R[q + rpl];
    acc[1] += E[q] * R[q + rpl] + E[q + P2] * R[q];
  }
  tree_sum(red, acc);
  if (threadIdx.x < 2) g.part[((long long)ch * g.e.max_chunks + c) * 2 + threadIdx.x] = red[threadIdx.x][0];
}

// The values of a chain batch: the chunk sums of each chain in ascending order, divided by L_n[0][0], as (Re, Im).
__global__ __launch_bounds__(256) void qk_str_valuesz_kernel(const StrArgs g, const int nc, const int n_strings, double* out) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= nc) return;
  const int i = g.cent[ch], m = g.cstr[ch];
  const long long st = g.e.states[i];
  const int chunks = g.e.dims[st * (g.e.n_sites + 1) + g.supp[2 * m + 1] + 1] / LOC_CHUNK;
  const double* p = g.part + (long long)ch * g.e.max_chunks * 2;
  double vr = 0, vi = 0;
  for (int c = 0; c < chunks; ++c) vr += p[2 * c], vi += p[2 * c + 1];
  const double nrm = g.e.scratch[g.e.sbase[i]];
  out[2 * (st * n_strings + m)] = vr / nrm;
  out[2 * (st * n_strings + m) + 1] = vi / nrm;
}

// tr(M_k^2) = sum_{a, a'} M_k[a][a'] M_k[a'][a] over one 16-row chunk of a (the imaginary parts cancel between (a, a') and its
// image, so only Re is summed), unnormalised: part[(i, k, chunk)].  M_k is in the T planes, ld = the padded bond.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_bond_trace_kernel(const LocArgs g) {
  __shared__ double red[1][LOC_RED_THREADS];
  const int2 t = g.tasks[blockIdx.x];
  const int i = t.x, c = t.y;
  const int n = g.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.states[i];
  const int pk = g.dims[st * n1 + k];
  const long long P = g.pmax[i], P2 = P * P;
  const double* const Mre = g.scratch + g.sbase[i] + at_T() * P2;
  const double* const Mim = Mre + 2 * P2;
  double acc[1] = {};
  const int cnt = LOC_CHUNK * pk;
  for (int e = threadIdx.x; e < cnt; e += LOC_RED_THREADS) {
    const int a = c * LOC_CHUNK + e / pk, ap = e % pk;
    const long long q = (long long)a * pk + ap, qt = (long long)ap * pk + a;
    acc[0] += Mre[q] * Mre[qt] - Mim[q] * Mim[qt];
  }
  tree_sum(red, acc);
  if (threadIdx.x == 0) g.part[((long long)i * n + k) * g.max_chunks + c] = red[0][0];
}

// Purities of a state batch: the chunk sums of each (state, bond) in a fixed order, divided by L_n[0][0]^2.
__global__ __launch_bounds__(256) void qk_bond_purities_kernel(const LocArgs g, const int nb, double* out) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n = g.n_sites, n1 = n + 1;
  if (id >= (long long)nb * (n - 1)) return;
  const int i = (int)(id / (n - 1)), k = 1 + (int)(id % (n - 1));
  const long long st = g.states[i];
  const double nrm = g.scratch[g.sbase[i]];  // L_n[0][0]
  const int chunks = g.dims[st * n1 + k] / LOC_CHUNK;
  const double* p = g.part + ((long long)i * n + k) * g.max_chunks;
  double v = 0;
  for (int c = 0; c < chunks; ++c) v += p[c];
  out[st * (n - 1) + k - 1] = v / (nrm * nrm);
}

// ---- the driver of a state batch, shared by every entry point -------------------------------------------------------------------
struct EnvBatch : EnvTables {
  std::vector<char> stage;  // host image of the tables: alive until the stream has taken it (the caller synchronises per batch)
  LocArgs g{};
  char* base = nullptr;  // the batch's device buffer
};
// upload the tables, then enqueue reverse, init and the launches of `plan` on the context's stream; eb.g describes the batch afterwards
int env_run(qk_ctx* c, const qk_mps_set* set, const char* what, double* rev, const EnvSizes& z, const Plan& plan, EnvBatch& eb, const size_t extra) {
  const int n = set->n_sites, nb = eb.nb;
  HIP_TRY_AS(what, c->local_scratch.ensure(eb.used() + extra));
  char* base = eb.base = c->local_scratch.get<char>();
  std::vector<char>& stage = eb.stage;
  stage.assign(eb.b_tab, 0);
  size_t at = 0;
  auto put = [&](const void* src, size_t bytes, size_t span) {
    if (bytes) std::memcpy(stage.data() + at, src, bytes);  // (an empty plan has no tasks)
    const size_t here = at;
    at += span;
    return base + here;
  };
  LocArgs& g = eb.g;
  g = LocArgs{};
  g.data = set->d_data.get<double>();
  g.rev = rev;
  g.dims = set->d_dims.get<int32_t>();
  g.tru = set->d_true.get<int32_t>();
  g.offs = set->d_offs.get<int64_t>();
  g.states = reinterpret_cast<const int32_t*>(put(eb.h_states.data(), nb * sizeof(int32_t), eb.b_states));
  g.pmax = reinterpret_cast<const int32_t*>(put(eb.h_pmax.data(), nb * sizeof(int32_t), eb.b_pmax));
  g.sbase = reinterpret_cast<const int64_t*>(put(eb.h_sbase.data(), nb * sizeof(int64_t), eb.b_sbase));
  g.roff = reinterpret_cast<const int64_t*>(put(eb.h_roff.data(), eb.h_roff.size() * sizeof(int64_t), eb.b_roff));
  if (z.keep_l) g.loff = reinterpret_cast<const int64_t*>(put(eb.h_loff.data(), eb.h_loff.size() * sizeof(int64_t), eb.b_roff));
  const int2* d_tasks = reinterpret_cast<const int2*>(put(eb.tasks.data(), eb.tasks.size() * sizeof(int2), eb.b_tasks));
  g.part = reinterpret_cast<double*>(base + eb.b_tab);
  if (z.n_pairs) g.part2 = g.part + (size_t)nb * n * z.max_chunks * 4;  // behind the one-qubit partial sums
  g.scratch = reinterpret_cast<double*>(base + eb.b_tab + eb.b_part);
  g.rmul = z.rmul;
  g.max_dist = z.max_dist;
  g.n_pairs = z.n_pairs;
  g.n_sites = n;
  g.max_chunks = z.max_chunks;
  HIP_TRY_AS(what, hipMemcpyAsync(base, stage.data(), eb.b_tab, hipMemcpyHostToDevice, c->stream));
  qk_local_reverse_kernel<<<dim3(nb, n), dim3(256), 0, c->stream>>>(g, rev);
  qk_local_init_kernel<<<dim3(nb), dim3(256), 0, c->stream>>>(g, nb);
  HIP_TRY_AS(what, hipGetLastError());
  for (size_t li = 0; li < plan.size(); ++li) {
    const int kind = plan[li].first;
    g.tasks = d_tasks + eb.first[li];
    g.step = plan[li].second;
    if (eb.first[li + 1] <= eb.first[li]) continue;
    const dim3 grid((unsigned)(eb.first[li + 1] - eb.first[li])), red(LOC_RED_THREADS);
    if (kind >= 0 && conj_b(kind)) qk_local_gemm_kernel<true><<<grid, dim3(512), 0, c->stream>>>(g, kind);
    else if (kind >= 0) qk_local_gemm_kernel<false><<<grid, dim3(512), 0, c->stream>>>(g, kind);
    else if (kind == LOC_RHO) qk_local_rho_kernel<<<grid, red, 0, c->stream>>>(g);
    else if (kind == LOC_PAIR_RHO) qk_local_pair_rho_kernel<false><<<grid, red, 0, c->stream>>>(g);
    else if (kind == LOC_DIST_RHO) qk_local_pair_rho_kernel<true><<<grid, red, 0, c->stream>>>(g);
    else if (kind == LOC_ADMIT) qk_local_admit_kernel<<<grid, red, 0, c->stream>>>(g);
    else if (kind == LOC_BOND_TR) qk_bond_trace_kernel<<<grid, red, 0, c->stream>>>(g);
    else qk_str_lnext_kernel<<<grid, red, 0, c->stream>>>(g);
  }
  HIP_TRY_AS(what, hipGetLastError());
  return QK_OK;
}
// doubles of a quarter of the device memory that is free, counting the context's own scratch: the memory bound of a state batch
int quarter_of_free(qk_ctx* c, const char* what, long long& budget) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY_AS(what, hipMemGetInfo(&free_b, &total_b));
  budget = (long long)((free_b + c->local_scratch.bytes) / 4 / sizeof(double));
  return QK_OK;
}

// ---- the driver of a chain batch, shared by the six chain families (strings, block, sample, amplitude, window, MPO) ---------------
// the launches of a task list that have tasks: launch(li, first task, grid)
template <class Launch>
void each_launch(const std::vector<long long>& first, Launch&& launch) {
  for (size_t li = 0; li + 1 < first.size(); ++li)
    if (first[li + 1] > first[li]) launch(li, first[li], dim3((unsigned)(first[li + 1] - first[li])));
}
struct ChainBatch {  // the chain batch at hand, as its family sees it: the chains [c0, c0 + nc) in the device buffer at base, offsets in st
  char* base;
  const ChainStage& st;
  size_t c0, nc;
  const std::vector<long long>& first;  // of its task list, per launch
};
using ChainLists = std::function<void(size_t c0, size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first)>;
using ChainHook = std::function<int(const ChainBatch&)>;
// The chain batches of a cut, one after the other, in the device buffer at `base` (NULL: the start of the context's scratch, made
// large enough here).  Per batch: the family's task lists, the stage (chain_stage), the upload of its table image on the context's
// stream, `enqueue` -- the family sets its pointers from base + the offsets and enqueues its launches -- then `before_sync` (what
// the family must still enqueue), the synchronise -- the staged tables are reused by the next batch -- and `after_sync` (what the
// family reads back).
int chain_run(qk_ctx* c, const char* what, char* base, const std::vector<ChainCol>& cols, const ChainCore& ch, const std::vector<size_t>& cstart, const long long width,
              const ChainLists& lists, const std::function<void(const ChainBatch&)>& enqueue, const ChainHook& before_sync = nullptr, const ChainHook& after_sync = nullptr) {
  std::vector<Task2> tasks;
  std::vector<long long> first;
  ChainStage st;
  for (size_t cb = 0; cb + 1 < cstart.size(); ++cb) {
    const size_t c0 = cstart[cb], nc = cstart[cb + 1] - c0;
    if (nc == 0) continue;
    lists(c0, nc, tasks, first);
    chain_stage(cols, ch, c0, c0 + nc, width, tasks, st);
    if (!base) HIP_TRY_AS(what, c->local_scratch.ensure(st.total));
    const ChainBatch b{base ? base : c->local_scratch.get<char>(), st, c0, nc, first};
    HIP_TRY_AS(what, hipMemcpyAsync(b.base, st.image.data(), st.part, hipMemcpyHostToDevice, c->stream));
    enqueue(b);
    HIP_TRY_AS(what, hipGetLastError());
    if (before_sync)
      if (const int rc = before_sync(b)) return rc;
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
    if (after_sync)
      if (const int rc = after_sync(b)) return rc;
  }
  return QK_OK;
}

// The local sweep of a set.  out1 = Bloch vectors [n_states][n_sites][3] (may be NULL when out2 is given), norms (may be NULL);
// out2 = Pauli correlators of the pairs up to distance max_dist [n_states][n_pairs][4][4] (NULL: the one-qubit sweep alone).
int local_sweep(qk_ctx* c, const qk_mps_set* set, const char* what, const char* range, double* out1, double* norms, double* out2, const int max_dist) {
  const bool pair = out2 != nullptr;
  if (!c || !set || (!out1 && !out2)) return qk_fail(QK_EINVAL, "%s: null argument", what);
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: the set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: complex64 sets are not supported; local Paulis need an fp64 set", what);
  const int ns = set->n_states, n = set->n_sites;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: empty set", what);
  if (pair && n < 2) return qk_fail(QK_EINVAL, "%s: pairs of neighbouring qubits need n_sites >= 2 (got %d)", what, n);
  if (pair && (max_dist < 1 || max_dist > n - 1)) return qk_fail(QK_EINVAL, "%s: max_dist must be in 1 .. n_sites - 1 = %d (got %d)", what, n - 1, max_dist);
  QkRangeGuard range_(range);
  const int D = pair ? max_dist : 1;
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  EnvSizes z;
  env_sizes(set->dims_true.data(), ns, n, set->max_pad, rmul(pair, D), false, z);  // the window and its intermediates count in need[s]
  z.max_dist = D, z.n_pairs = pair ? n_pairs(D, n) : 0;
  const int np = z.n_pairs;
  const long long part_per_state = (long long)n * z.max_chunks * 4 + (long long)np * z.max_chunks * LOC_PAIR_VALS;
  // memory bound of the per-state scratch: a quarter of what is free once the reversed image and the outputs exist
  QkDevBuf rev, dout, dnorm, dout2;
  HIP_TRY_AS(what, rev.alloc((size_t)set->bytes));
  HIP_TRY_AS(what, dout.alloc((size_t)ns * n * 3 * sizeof(double)));
  HIP_TRY_AS(what, dnorm.alloc((size_t)ns * sizeof(double)));
  if (pair) HIP_TRY_AS(what, dout2.alloc((size_t)ns * np * 16 * sizeof(double)));
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const std::vector<int> bstart = batch_cut(z.need, part_per_state, budget);  // scratch and rho partial sums of a state
  const Plan plan = local_plan(n, pair, D);
  EnvBatch eb;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(z, plan, s0, nb, part_per_state, eb);
    if (const int rc = env_run(c, set, what, rev.get<double>(), z, plan, eb, 0)) return rc;
    const long long nf = (long long)nb * n;
    qk_local_features_kernel<<<dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, c->stream>>>(eb.g, nb, dout.get<double>(), dnorm.get<double>());
    if (pair) qk_local_pair_features_kernel<<<dim3((unsigned)(((long long)nb * np + 255) / 256)), dim3(256), 0, c->stream>>>(eb.g, nb, dout2.get<double>());
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the staged tables are reused by the next batch
  }
  if (out1) HIP_TRY_AS(what, hipMemcpy(out1, dout.get(), (size_t)ns * n * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (norms) HIP_TRY_AS(what, hipMemcpy(norms, dnorm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
  if (pair) HIP_TRY_AS(what, hipMemcpy(out2, dout2.get(), (size_t)ns * np * 16 * sizeof(double), hipMemcpyDeviceToHost));
  return QK_OK;
}

// Pauli strings and strings of single-site operators: one driver.  Per state batch the environment pass -- the reversed chain and
// the forward T / W launches of the one-qubit sweep, then L_{k+1} from W by the sum the rho kernel makes (so L_n[0][0] is that
// sweep's norm bit for bit), every R_k (k = 1 .. n) and every L_k (k = 0 .. n-1) kept -- then its chains in chain batches
// (qk_local_plan.h: list_chains, chain_cut, chain_lists).  ops == NULL: Pauli strings (codes 0..3, the real part of the closing
// sum, out [n_states][n_strings]).  ops != NULL: the table [n_ops][2][2][2] of the operator strings (codes 0 .. n_ops, the complex
// closing sum, out [n_states][n_strings][2]); the two forms differ in the elementwise kernel, the closing kernels and the width of
// a chain's partial sums, nothing else.
int string_chains(qk_ctx* c, const qk_mps_set* set, const char* what, const char* range, const char* batch_var, const int32_t n_ops, const double* ops,
                  const int32_t n_strings, const uint8_t* strings, double* out, double* norms) {
  const bool general = ops != nullptr;
  const int vals = general ? 2 : 1;  // doubles of a value and of a chunk sum
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!set) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!strings) return qk_fail(QK_EINVAL, "%s: strings is null", what);
  if (!out) return qk_fail(QK_EINVAL, "%s: out is null", what);
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; %s need an fp64 set", what, general ? "operator strings" : "Pauli strings");
  if (n_strings < 1) return qk_fail(QK_EINVAL, "%s: n_strings must be >= 1 (got %d)", what, n_strings);
  if (general && (n_ops < 1 || n_ops > OPSTR_MAX_OPS)) return qk_fail(QK_EINVAL, "%s: n_ops must be in 1 .. %d (got %d)", what, OPSTR_MAX_OPS, n_ops);
  for (long long e = 0; general && e < 8ll * n_ops; ++e)
    if (!std::isfinite(ops[e]))
      return qk_fail(QK_EINVAL, "%s: ops[%d][%d][%d] (code %d) has a %s part that is not finite", what, (int)(e / 8), (int)(e / 4 % 2), (int)(e / 2 % 2), (int)(e / 8) + 1,
                     e % 2 ? "imaginary" : "real");
  const int ns = set->n_states, n = set->n_sites;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  std::vector<int32_t> supp;  // a, b of each string; -1: all identity
  if (const long long bad = operator_supports(strings, n_strings, n, general ? n_ops : 3, supp); bad >= 0) {
    if (general) return qk_fail(QK_EINVAL, "%s: strings[%d][%d] = %d is above n_ops = %d (0 = identity, c = ops[c - 1])", what, (int)(bad / n), (int)(bad % n), strings[bad], n_ops);
    return qk_fail(QK_EINVAL, "%s: strings[%d][%d] = %d is not a Pauli code (0..3 = I, X, Y, Z)", what, (int)(bad / n), (int)(bad % n), strings[bad]);
  }
  long long cap = 0;  // chains per batch
  if (const int rc = batch_cap(what, batch_var, cap)) return rc;
  QkRangeGuard range_(range);
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  EnvSizes z;
  env_sizes(set->dims_true.data(), ns, n, set->max_pad, LOC_RMUL, true, z);
  const int max_chunks = z.max_chunks;
  const size_t b_str = al256((size_t)n_strings * n), b_supp = al256(supp.size() * sizeof(int32_t));
  QkDevBuf rev, dout, dnorm, dstr, dops;
  HIP_TRY_AS(what, rev.alloc((size_t)set->bytes));
  HIP_TRY_AS(what, dout.alloc((size_t)ns * n_strings * vals * sizeof(double)));
  HIP_TRY_AS(what, dnorm.alloc((size_t)ns * sizeof(double)));
  HIP_TRY_AS(what, dstr.alloc(b_str + b_supp));
  HIP_TRY_AS(what, hipMemcpy(dstr.get<char>(), strings, (size_t)n_strings * n, hipMemcpyHostToDevice));
  HIP_TRY_AS(what, hipMemcpy(dstr.get<char>() + b_str, supp.data(), supp.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (general) {
    HIP_TRY_AS(what, dops.alloc((size_t)n_ops * 8 * sizeof(double)));
    HIP_TRY_AS(what, hipMemcpy(dops.get(), ops, (size_t)n_ops * 8 * sizeof(double), hipMemcpyHostToDevice));
  }
  // memory bound of a state batch (environments and the slots of its live chains): a quarter of what is free; the environments
  // of a batch take at most half of that (at least one state per batch), the chains of a batch the rest (at least one chain)
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const std::vector<int> bstart = batch_cut(z.need, 0, budget / 2);
  const Plan plan = env_plan(n);
  EnvBatch eb;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(z, plan, s0, nb, 0, eb);
    // the chains of the state batch, cut into chain batches: consecutive chains while their slots, partial sums and tasks fit
    // what the environments leave, and at most QK_STRINGS_BATCH of them
    Chains ch = list_chains(z, s0, nb, n_strings, strings, supp);
    if (general)
      for (long long& w : ch.weight) w += max_chunks;  // a chunk sum is (Re, Im)
    const std::vector<size_t> cstart = chain_cut(ch.weight, budget - eb.tot, cap);
    const std::vector<ChainCol> cols{{ch.cent.data(), sizeof(int32_t), 1}, {ch.cstr.data(), sizeof(int32_t), 1}};
    const long long width = (long long)max_chunks * vals;  // of a chain's partial sums
    if (const int rc = env_run(c, set, what, rev.get<double>(), z, plan, eb, chain_stage_max(cols, ch, cstart, width))) return rc;
    qk_str_norms_kernel<<<dim3((nb + 255) / 256), dim3(256), 0, c->stream>>>(eb.g, nb, dnorm.get<double>());
    HIP_TRY_AS(what, hipGetLastError());
    OpArgs qa{};
    qa.ops = dops.get<double>();
    StrArgs& q = qa.s;
    q.e = eb.g;
    q.strings = dstr.get<uint8_t>();
    q.supp = reinterpret_cast<const int32_t*>(dstr.get<char>() + b_str);
    const int rc = chain_run(
        c, what, eb.base + eb.used(), cols, ch, cstart, width,
        [&](size_t c0, size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) { chain_lists(z, s0, ch, c0, nc, strings, supp, tasks, first); },
        [&](const ChainBatch& b) {
          q.cent = reinterpret_cast<const int32_t*>(b.base + b.st.col[0]);
          q.cstr = reinterpret_cast<const int32_t*>(b.base + b.st.col[1]);
          q.cbase = reinterpret_cast<const int64_t*>(b.base + b.st.col[2]);
          const int2* d_ctasks = reinterpret_cast<const int2*>(b.base + b.st.tasks);
          q.part = reinterpret_cast<double*>(b.base + b.st.part);
          q.slots = reinterpret_cast<double*>(b.base + b.st.slots);
          each_launch(b.first, [&](const size_t li, const long long t0, const dim3 grid) {
            const int kind = CHAIN_KINDS[li % 4];
            q.tasks = d_ctasks + t0;
            q.step = (int)(li / 4);
            if (kind == STR_T) qk_str_gemm_kernel<false><<<grid, dim3(512), 0, c->stream>>>(q);
            else if (kind == STR_X) qk_str_gemm_kernel<true><<<grid, dim3(512), 0, c->stream>>>(q);
            else if (kind == STR_PAULI && !general) qk_str_pauli_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(q);
            else if (kind == STR_PAULI) qk_str_op_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(qa);
            else if (!general) qk_str_close_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(q);
            else qk_str_closez_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(qa);
          });
          if (!general) qk_str_values_kernel<<<dim3((unsigned)((b.nc + 255) / 256)), dim3(256), 0, c->stream>>>(q, (int)b.nc, n_strings, dout.get<double>());
          else qk_str_valuesz_kernel<<<dim3((unsigned)((b.nc + 255) / 256)), dim3(256), 0, c->stream>>>(q, (int)b.nc, n_strings, dout.get<double>());
        });
    if (rc) return rc;
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  }
  if (general) {  // a value divides by <psi|psi> (a norm that is NaN marks its own row, as the Pauli strings do)
    std::vector<double> h_norm((size_t)ns);
    HIP_TRY_AS(what, hipMemcpy(h_norm.data(), dnorm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = 0; s < ns; ++s)
      if (h_norm[s] == 0.0) return qk_fail(QK_EDEVICE, "%s: state %d has norm 0: its expectation values are undefined", what, s);
  }
  HIP_TRY_AS(what, hipMemcpy(out, dout.get(), (size_t)ns * n_strings * vals * sizeof(double), hipMemcpyDeviceToHost));
  if (norms) HIP_TRY_AS(what, hipMemcpy(norms, dnorm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
  for (int m = 0; m < n_strings; ++m)  // an all-identity string is exactly 1
    if (supp[2 * m] < 0)
      for (int s = 0; s < ns; ++s) {
        out[((size_t)s * n_strings + m) * vals] = 1.0;
        if (general) out[((size_t)s * n_strings + m) * vals + 1] = 0.0;
      }
  return QK_OK;
}

// ---- MPO observables (qk_mpo_expectations_host) ---------------------------------------------------------------------------------
// value = <psi| H |psi> / <psi|psi> of a matrix-product operator H = sum_{u_1 .. u_{n-1}} (x)_k W_k[u_k][u_{k+1}], W_k[u][v][s'][s] =
// <s'| . |s>, with support [a, b] (the hull of the sites whose tensor is not the exact 1 x 1 identity): the chain of the operator
// strings with w_k planes of E at the cut in front of site k,
//     E_a = L_a                                                                                  (w_a = 1)
//     T[u]  = E[u] . A_k                     one ring GEMM, the planes stacked along M = w_k pad_k                       (MPO_T)
//     T'[v][(a, s')] = sum_u sum_s W_k[u][v][s'][s] T[u][(a, s)]     out of place, over the listed blocks of plane v    (MPO_MIX)
//     E'[v] = T'[v] contracted with conj(A_k)  one ring GEMM launch, a plane per v, at column v pad_{k+1}              (MPO_X)
//     value = sum_{b', a'} E_{b+1}[0][b'][a'] R_{b+1}[b'][a'] / L_n[0][0]                          (w_{b+1} = 1, MPO_CLOSE)
// The environment pass, the chain driver and the closing kernels are those of the operator strings; the slot of a chain, the block
// lists and the task lists are in qk_local_plan.h.  A site of the support whose tensor is the exact 1 x 1 identity has no mix
// launch (the X-shaped product reads T).  The sum of a T' element runs over the listed blocks of its plane in ascending u, s = 0
// before s = 1, the imaginary factor before the real one, each component one chain of fused multiply-adds whose first term is a
// plain product -- with one block that is qk_str_op_kernel's expression, so a bond-1 MPO gives the bits of its operator string.  Every
// u plane goes through the first GEMM and every v plane through the second, whether a block reads or writes it: a plane without a
// block is written as zeros, so no element of a slot is read before this call wrote it.  4 launches per site of a chain batch,
// no atomics, no grid barrier, no spin wait; nothing of a chain depends on another chain.  QK_MPO_BATCH caps the chains of a batch.
struct MpoArgs {
  OpArgs o;               // o.s: the chain batch as the string kernels see it (cstr = the MPO, supp = the MPO supports); o.ops is not used
  const int32_t* bonds;   // [n_mpos][n_sites + 1]
  const int32_t* wmax;    // [n_mpos]
  const int32_t* vat;     // [n_mpos][n_sites]: first entry of the site in vfirst, -1: no mix launch
  const int32_t* vfirst;  // per site with a mix launch: w_{k+1} + 1 block indices
  const int32_t* blk_u;   // per listed block
  const double* blk_w;    // per listed block: (re, im) of W[u][v][s'][s]
};

// One 64 x 64 output block of one chain's GEMM at site k.  CONJB = false: MPO_T, the stacked planes as one matrix (a row's sums
// are those of its plane alone: the K order is fixed); true: MPO_X, block number = (v, block of the plane's product).
template <bool CONJB>
__global__ __launch_bounds__(512) void qk_mpo_gemm_kernel(const MpoArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[LOC_LDS_DOUBLES];
  const StrArgs& g = a.o.s;
  const int2 t = g.tasks[blockIdx.x];
  const int ch = __builtin_amdgcn_readfirstlane(t.x);
  int blk = __builtin_amdgcn_readfirstlane(t.y);
  const int i = __builtin_amdgcn_readfirstlane(g.cent[ch]);
  const int m = __builtin_amdgcn_readfirstlane(g.cstr[ch]);
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = __builtin_amdgcn_readfirstlane(g.e.states[i]);
  const int l = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k]), r = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k + 1]);
  const int lt = __builtin_amdgcn_readfirstlane(g.e.tru[st * n1 + k]);
  const int wl = __builtin_amdgcn_readfirstlane(a.bonds[(long long)m * n1 + k]), wr = __builtin_amdgcn_readfirstlane(a.bonds[(long long)m * n1 + k + 1]);
  const long long P = __builtin_amdgcn_readfirstlane(g.e.pmax[i]), P2 = P * P;
  const long long U = P2 * __builtin_amdgcn_readfirstlane(a.wmax[m]);
  double* const E = g.slots + uni64(g.cbase[ch]);
  double* const T = E + mpo_T() * U;
  const double* Bre = g.e.data + uni64(g.e.offs[st * n + k]);
  const double* Bim = Bre + (long long)l * 2 * r;
  const double *Are, *Aim;
  double *Cre, *Cim;
  int lda, ldb, ldc, M, N, K;
  if (!CONJB) {
    if (__builtin_amdgcn_readfirstlane(g.supp[2 * m]) == k) {  // the chain starts here: E_a = L_a, one plane
      Are = g.e.scratch + uni64(g.e.sbase[i]) + g.e.rmul * P2 + uni64(g.e.loff[(long long)i * n1 + k]);
      Aim = Are + (long long)l * l;
      lda = l;
    } else {
      Are = E, Aim = E + wl * P2;
      lda = wl * l;
    }
    Cre = T, Cim = T + 2 * U;
    ldb = 2 * r, ldc = 2 * r, M = wl * l, N = 2 * r, K = lt;
  } else {
    const int per = ((r + 63) / 64) * ((r + 63) / 64);
    const int v = blk / per;
    blk -= v * per;
    const double* const src = __builtin_amdgcn_readfirstlane(a.vat[(long long)m * n + k]) < 0 ? T : E + mpo_Tp() * U;
    Are = src + (long long)v * l * 2 * r, Aim = Are + 2 * U;
    Cre = E + (long long)v * r, Cim = Cre + wr * P2;
    lda = r, ldb = r, ldc = wr * r, M = r, N = r, K = 2 * lt;
  }
  const int npm = (M + 63) / 64;
  const int m0 = 64 * (blk % npm), n0 = 64 * (blk / npm);
  zgemm_ring3<CONJB, LOC_KTL, LOC_NSLOT, true, 8, 64, double, 12>(Cre + (long long)m0 * ldc + n0, Cim + (long long)m0 * ldc + n0, ldc, Are + m0, Aim + m0, lda,
                                                                   Bre + n0, Bim + n0, ldb, min(64, M - m0), min(64, N - n0), K, lds);
}

// The MPO tensor of site k on the ket index of T, out of place: rows a of one 16-row chunk of the plane T'[v], block number = (v,
// chunk).  The coefficients of the plane's listed blocks are staged in LDS once per workgroup (at most MPO_MAX_BOND blocks, 2 KiB)
// and read from there as broadcasts.  The first listed block starts each component with qk_str_op_kernel's expression, the others
// continue the chain of fused multiply-adds; a plane without a block is written as zeros.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_mpo_mix_kernel(const MpoArgs a) {
  __shared__ double cw[MPO_MAX_BOND * 8];
  __shared__ int cu[MPO_MAX_BOND];
  const StrArgs& g = a.o.s;
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x;
  const int i = g.cent[ch], m = g.cstr[ch];
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.e.states[i];
  const int l = g.e.dims[st * n1 + k], r = g.e.dims[st * n1 + k + 1];
  const int chunks = l / LOC_CHUNK;
  const int v = t.y / chunks, c = t.y % chunks;
  const int at = a.vat[(long long)m * n + k];  // >= 0: a chain has a task here only where the site has a mix launch
  const int f0 = a.vfirst[at + v], nblk = min(a.vfirst[at + v + 1] - f0, MPO_MAX_BOND);
  for (int e = threadIdx.x; e < 8 * nblk; e += LOC_RED_THREADS) cw[e] = a.blk_w[8ll * f0 + e];
  for (int e = threadIdx.x; e < nblk; e += LOC_RED_THREADS) cu[e] = a.blk_u[f0 + e];
  __syncthreads();
  const long long P = g.e.pmax[i], U = P * P * a.wmax[m], tpl = 2 * U, plane = (long long)l * 2 * r;
  const double* const T = g.slots + g.cbase[ch] + mpo_T() * U;
  double* const Tp = g.slots + g.cbase[ch] + mpo_Tp() * U + v * plane;
  const int cnt = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < cnt; e += LOC_RED_THREADS) {
    const long long q0 = (long long)(c * LOC_CHUNK + e / r) * 2 * r + e % r, q1 = q0 + r;
    double o0r = 0, o0i = 0, o1r = 0, o1i = 0;
    for (int j = 0; j < nblk; ++j) {
      const double* const Tu = T + cu[j] * plane;
      const double* const o = cw + 8 * j;
      const double ar = o[0], ai = o[1], br = o[2], bi = o[3], cr = o[4], ci = o[5], dr = o[6], di = o[7];  // W[u][v] = [[a, b], [c, d]]
      const double r0 = Tu[q0], i0 = Tu[q0 + tpl], r1 = Tu[q1], i1 = Tu[q1 + tpl];
      if (j == 0) {
        o0r = fma(br, r1, fma(-bi, i1, fma(ar, r0, -(ai * i0))));
        o0i = fma(br, i1, fma(bi, r1, fma(ar, i0, ai * r0)));
        o1r = fma(dr, r1, fma(-di, i1, fma(cr, r0, -(ci * i0))));
        o1i = fma(dr, i1, fma(di, r1, fma(cr, i0, ci * r0)));
      } else {
        o0r = fma(br, r1, fma(-bi, i1, fma(ar, r0, fma(-ai, i0, o0r))));
        o0i = fma(br, i1, fma(bi, r1, fma(ar, i0, fma(ai, r0, o0i))));
        o1r = fma(dr, r1, fma(-di, i1, fma(cr, r0, fma(-ci, i0, o1r))));
        o1i = fma(dr, i1, fma(di, r1, fma(cr, i0, fma(ci, r0, o1i))));
      }
    }
    Tp[q0] = o0r, Tp[q0 + tpl] = o0i, Tp[q1] = o1r, Tp[q1 + tpl] = o1i;
  }
}

int mpo_chains(qk_ctx* c, const qk_mps_set* set, const int32_t n_mpos, const int32_t* bonds, const double* tensors, double* out, double* norms) {
  static const char* what = "qk_mpo_expectations_host";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!set) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!bonds) return qk_fail(QK_EINVAL, "%s: bonds is null", what);
  if (!tensors) return qk_fail(QK_EINVAL, "%s: tensors is null", what);
  if (!out) return qk_fail(QK_EINVAL, "%s: out is null", what);
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; MPO observables need an fp64 set", what);
  if (n_mpos < 1) return qk_fail(QK_EINVAL, "%s: n_mpos must be >= 1 (got %d)", what, n_mpos);
  const int ns = set->n_states, n = set->n_sites, n1 = n + 1;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  if (const long long bad = mpo_bad_bond(bonds, n_mpos, n); bad >= 0)
    return qk_fail(QK_EINVAL, "%s: bonds[%d][%d] = %d is outside 1 .. %d (MPO %d, cut %d)", what, (int)(bad / n1), (int)(bad % n1), bonds[bad], MPO_MAX_BOND, (int)(bad / n1),
                   (int)(bad % n1));
  for (int m = 0; m < n_mpos; ++m)
    for (const int k : {0, n})
      if (bonds[(size_t)m * n1 + k] != 1) return qk_fail(QK_EINVAL, "%s: bonds[%d][%d] = %d must be 1 (the end of MPO %d)", what, m, k, bonds[(size_t)m * n1 + k], m);
  {
    long long e = 0;
    for (int m = 0; m < n_mpos; ++m)
      for (int k = 0; k < n; ++k) {
        const int wr = bonds[(size_t)m * n1 + k + 1];
        for (long long q = 0; q < 8ll * bonds[(size_t)m * n1 + k] * wr; ++q, ++e)
          if (!std::isfinite(tensors[e]))
            return qk_fail(QK_EINVAL, "%s: MPO %d, site %d: W[%d][%d][%d][%d] has a %s part that is not finite", what, m, k, (int)(q / 8 / wr), (int)(q / 8 % wr), (int)(q / 4 % 2),
                           (int)(q / 2 % 2), q % 2 ? "imaginary" : "real");
      }
  }
  long long cap = 0;  // chains per batch
  if (const int rc = batch_cap(what, "QK_MPO_BATCH", cap)) return rc;
  QkRangeGuard range_("qk:mpo_expectations");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  const MpoPlan mp = mpo_plan(bonds, tensors, n_mpos, n);
  EnvSizes z;
  env_sizes(set->dims_true.data(), ns, n, set->max_pad, LOC_RMUL, true, z);
  const int max_chunks = z.max_chunks;
  // the tables of the MPOs, uploaded once: bonds | wmax | supp | vat | vfirst | blk_u | blk_w (an empty region keeps one element)
  const std::vector<std::pair<const void*, size_t>> regions{{mp.bonds.data(), mp.bonds.size() * sizeof(int32_t)},   {mp.wmax.data(), mp.wmax.size() * sizeof(int32_t)},
                                                            {mp.supp.data(), mp.supp.size() * sizeof(int32_t)},     {mp.vat.data(), mp.vat.size() * sizeof(int32_t)},
                                                            {mp.vfirst.data(), mp.vfirst.size() * sizeof(int32_t)}, {mp.blk_u.data(), mp.blk_u.size() * sizeof(int32_t)},
                                                            {mp.blk_w.data(), mp.blk_w.size() * sizeof(double)}};
  std::vector<size_t> rat;
  size_t tab_bytes = 0;
  for (const auto& rg : regions) rat.push_back(tab_bytes), tab_bytes += al256(std::max<size_t>(rg.second, 8));
  std::vector<char> tab(tab_bytes, 0);
  for (size_t e = 0; e < regions.size(); ++e)
    if (regions[e].second) std::memcpy(tab.data() + rat[e], regions[e].first, regions[e].second);
  QkDevBuf rev, dout, dnorm, dtab;
  HIP_TRY_AS(what, rev.alloc((size_t)set->bytes));
  HIP_TRY_AS(what, dout.alloc((size_t)ns * n_mpos * 2 * sizeof(double)));
  HIP_TRY_AS(what, dnorm.alloc((size_t)ns * sizeof(double)));
  HIP_TRY_AS(what, dtab.alloc(tab_bytes));
  HIP_TRY_AS(what, hipMemcpy(dtab.get<char>(), tab.data(), tab_bytes, hipMemcpyHostToDevice));
  // the memory rule of the strings: a quarter of what is free; the environments of a state batch take at most half of it, the
  // chains of a chain batch the rest (at least one chain)
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const std::vector<int> bstart = batch_cut(z.need, 0, budget / 2);
  const Plan plan = env_plan(n);
  EnvBatch eb;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(z, plan, s0, nb, 0, eb);
    const Chains ch = list_mpo_chains(z, s0, nb, mp);
    const std::vector<size_t> cstart = chain_cut(ch.weight, budget - eb.tot, cap);
    const std::vector<ChainCol> cols{{ch.cent.data(), sizeof(int32_t), 1}, {ch.cstr.data(), sizeof(int32_t), 1}};
    const long long width = 2ll * max_chunks;  // a chunk sum is (Re, Im)
    if (const int rc = env_run(c, set, what, rev.get<double>(), z, plan, eb, chain_stage_max(cols, ch, cstart, width))) return rc;
    qk_str_norms_kernel<<<dim3((nb + 255) / 256), dim3(256), 0, c->stream>>>(eb.g, nb, dnorm.get<double>());
    HIP_TRY_AS(what, hipGetLastError());
    MpoArgs qm{};
    qm.bonds = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[0]);
    qm.wmax = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[1]);
    qm.vat = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[3]);
    qm.vfirst = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[4]);
    qm.blk_u = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[5]);
    qm.blk_w = reinterpret_cast<const double*>(dtab.get<char>() + rat[6]);
    StrArgs& q = qm.o.s;
    q.e = eb.g;
    q.supp = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[2]);
    const int rc = chain_run(
        c, what, eb.base + eb.used(), cols, ch, cstart, width,
        [&](size_t c0, size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) { mpo_lists(z, s0, ch, c0, nc, mp, tasks, first); },
        [&](const ChainBatch& b) {
          q.cent = reinterpret_cast<const int32_t*>(b.base + b.st.col[0]);
          q.cstr = reinterpret_cast<const int32_t*>(b.base + b.st.col[1]);
          q.cbase = reinterpret_cast<const int64_t*>(b.base + b.st.col[2]);
          const int2* d_ctasks = reinterpret_cast<const int2*>(b.base + b.st.tasks);
          q.part = reinterpret_cast<double*>(b.base + b.st.part);
          q.slots = reinterpret_cast<double*>(b.base + b.st.slots);
          each_launch(b.first, [&](const size_t li, const long long t0, const dim3 grid) {
            const int kind = MPO_KINDS[li % 4];
            q.tasks = d_ctasks + t0;
            q.step = (int)(li / 4);
            if (kind == MPO_T) qk_mpo_gemm_kernel<false><<<grid, dim3(512), 0, c->stream>>>(qm);
            else if (kind == MPO_X) qk_mpo_gemm_kernel<true><<<grid, dim3(512), 0, c->stream>>>(qm);
            else if (kind == MPO_MIX) qk_mpo_mix_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(qm);
            else qk_str_closez_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(qm.o);
          });
          qk_str_valuesz_kernel<<<dim3((unsigned)((b.nc + 255) / 256)), dim3(256), 0, c->stream>>>(q, (int)b.nc, n_mpos, dout.get<double>());
        });
    if (rc) return rc;
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  }
  std::vector<double> h_norm((size_t)ns);  // a value divides by <psi|psi> (a norm that is NaN marks its own row)
  HIP_TRY_AS(what, hipMemcpy(h_norm.data(), dnorm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
  for (int s = 0; s < ns; ++s)
    if (h_norm[s] == 0.0) return qk_fail(QK_EDEVICE, "%s: state %d has norm 0: its expectation values are undefined", what, s);
  HIP_TRY_AS(what, hipMemcpy(out, dout.get(), (size_t)ns * n_mpos * 2 * sizeof(double), hipMemcpyDeviceToHost));
  if (norms) std::memcpy(norms, h_norm.data(), (size_t)ns * sizeof(double));
  for (int m = 0; m < n_mpos; ++m)  // an all-identity MPO is exactly 1 + 0j
    if (mp.supp[2 * m] < 0)
      for (int s = 0; s < ns; ++s) out[((size_t)s * n_mpos + m) * 2] = 1.0, out[((size_t)s * n_mpos + m) * 2 + 1] = 0.0;
  return QK_OK;
}

// ---- applying an MPO to a set (qk_mps_set_apply_mpo) ------------------------------------------------------------------------------
// The new set O|psi> of one MPO and every state of a set, site by site:
//     B_k[(u, a)][s'][(v, b)] = sum_s W_k[u][v][s'][s] A_k[a][s][b],   row u chi_k + a, column v chi_{k+1} + b
// A write-bound expansion with no dependency between sites: one launch, no atomics, no grid barrier, no spin wait.  The bonds, the
// offsets, the row lists of the blocks and the tasks are apply_plan's (qk_local_plan.h).  A workgroup takes one (state, site, u,
// 16-row chunk of a): it stages the listed blocks of row W_k[u][.] in LDS (at most MPO_MAX_BOND blocks, 2 KiB, read as broadcasts),
// a thread holds the A values of two neighbouring b of one row in registers and streams the column blocks v = 0 .. w_{k+1} - 1 out
// with 16-byte stores where the column v chi_{k+1} + b is even, 8-byte stores where it is odd (odd chi_{k+1} and odd v) and for the
// last b of an odd chi_{k+1}.  A v without a listed block, the padding columns and the padding rows are written as zeros by the
// kernel: there is no memset, every double of the image is written once.  An element is qk_mpo_mix_kernel's expression of one
// block; a site marked as a copy passes the source bits through.
struct ApplyArgs {
  const double* src;      // the source set's planes and its tables
  const int32_t* spad;    // padded bonds [n_states][n_sites + 1]
  const int32_t* stru;    // true bonds
  const int64_t* soffs;   // re-plane offsets [n_states][n_sites]
  double* dst;            // the new set's planes and its tables
  const int32_t* dpad;
  const int64_t* doffs;
  const int32_t* wb;      // the MPO's bonds [n_sites + 1]
  const int32_t* copy;    // [n_sites]
  const int32_t* uat;     // [n_sites]
  const int32_t* ufirst;
  const int32_t* blk_v;
  const double* blk_w;
  const int2* tasks;
  int n_sites;
};

__device__ __forceinline__ void apply_store2(double* const p, const double x, const double y, const bool wide, const bool two) {
  if (wide) {
    *reinterpret_cast<double2*>(p) = make_double2(x, y);
  } else {
    p[0] = x;
    if (two) p[1] = y;
  }
}

__global__ __launch_bounds__(LOC_RED_THREADS) void qk_mpo_apply_kernel(const ApplyArgs g) {
  __shared__ double cw[MPO_MAX_BOND * 8];
  __shared__ int cj[MPO_MAX_BOND];  // v -> its staged block, -1: none
  const int2 t = g.tasks[blockIdx.x];
  const int n = g.n_sites, n1 = n + 1;
  const long long st = t.x / n;
  const int k = t.x % n, u = apply_task_u(t.y), c = apply_task_chunk(t.y);
  const int wl = g.wb[k], wr = min(g.wb[k + 1], MPO_MAX_BOND);
  const int l = g.stru[st * n1 + k], r = g.stru[st * n1 + k + 1];
  const long long pl = g.spad[st * n1 + k], pr = g.spad[st * n1 + k + 1];
  const long long PL = g.dpad[st * n1 + k], PR = g.dpad[st * n1 + k + 1];
  const bool copy = g.copy[k] != 0;
  const int f0 = g.ufirst[g.uat[k] + u], nblk = min(g.ufirst[g.uat[k] + u + 1] - f0, MPO_MAX_BOND);
  for (int e = threadIdx.x; e < MPO_MAX_BOND; e += LOC_RED_THREADS) cj[e] = -1;
  for (int e = threadIdx.x; e < 8 * nblk; e += LOC_RED_THREADS) cw[e] = g.blk_w[8ll * f0 + e];
  __syncthreads();
  for (int e = threadIdx.x; e < nblk; e += LOC_RED_THREADS) cj[g.blk_v[f0 + e] & (MPO_MAX_BOND - 1)] = e;
  __syncthreads();
  const double* const Are = g.src + g.soffs[st * n + k];
  const double* const Aim = Are + pl * 2 * pr;
  double* const Bre = g.dst + g.doffs[st * n + k];
  const long long dpl = PL * 2 * PR;  // the im plane lies dpl behind the re plane
  const int a0 = LOC_CHUNK * c, rows = min(LOC_CHUNK, l - a0), half = (r + 1) / 2;
  for (int e = threadIdx.x; e < rows * half; e += LOC_RED_THREADS) {
    const int a = a0 + e / half, b = 2 * (e % half);
    const bool two = b + 1 < r;
    const long long q0 = (long long)a * 2 * pr + b, q1 = q0 + pr;  // even: pr is a multiple of 16, so b + 1 lies inside the padded row
    const double2 r0 = *reinterpret_cast<const double2*>(Are + q0), i0 = *reinterpret_cast<const double2*>(Aim + q0);
    const double2 r1 = *reinterpret_cast<const double2*>(Are + q1), i1 = *reinterpret_cast<const double2*>(Aim + q1);
    double* const row = Bre + ((long long)u * l + a) * 2 * PR;
    for (int v = 0; v < wr; ++v) {
      const int j = cj[v], col = v * r + b;
      const bool wide = two && !(col & 1);
      double2 o0r = make_double2(0, 0), o0i = o0r, o1r = o0r, o1i = o0r;
      if (copy) {
        o0r = r0, o0i = i0, o1r = r1, o1i = i1;
      } else if (j >= 0) {
        const double* const o = cw + 8 * j;
        const double ar = o[0], ai = o[1], br = o[2], bi = o[3], cr = o[4], ci = o[5], dr = o[6], di = o[7];  // W[u][v] = [[a, b], [c, d]]
        o0r.x = fma(br, r1.x, fma(-bi, i1.x, fma(ar, r0.x, -(ai * i0.x))));
        o0i.x = fma(br, i1.x, fma(bi, r1.x, fma(ar, i0.x, ai * r0.x)));
        o1r.x = fma(dr, r1.x, fma(-di, i1.x, fma(cr, r0.x, -(ci * i0.x))));
        o1i.x = fma(dr, i1.x, fma(di, r1.x, fma(cr, i0.x, ci * r0.x)));
        o0r.y = fma(br, r1.y, fma(-bi, i1.y, fma(ar, r0.y, -(ai * i0.y))));
        o0i.y = fma(br, i1.y, fma(bi, r1.y, fma(ar, i0.y, ai * r0.y)));
        o1r.y = fma(dr, r1.y, fma(-di, i1.y, fma(cr, r0.y, -(ci * i0.y))));
        o1i.y = fma(dr, i1.y, fma(di, r1.y, fma(cr, i0.y, ci * r0.y)));
      }
      apply_store2(row + col, o0r.x, o0r.y, wide, two);
      apply_store2(row + col + dpl, o0i.x, o0i.y, wide, two);
      apply_store2(row + col + PR, o1r.x, o1r.y, wide, two);
      apply_store2(row + col + PR + dpl, o1i.x, o1i.y, wide, two);
    }
  }
  // the padding columns of the task's rows (both s')
  const int c0 = wr * r, npc = (int)PR - c0;
  for (int e = threadIdx.x; e < rows * 2 * npc; e += LOC_RED_THREADS) {
    double* const p = Bre + (((long long)u * l + a0) * 2 + e / npc) * PR + c0 + e % npc;
    p[0] = 0.0, p[dpl] = 0.0;
  }
  // the padding rows of the site, by the task of the last u and the last chunk: one even run of doubles per plane
  if (u == wl - 1 && a0 + LOC_CHUNK >= l) {
    const long long z0 = (long long)wl * l * 2 * PR, nz = (dpl - z0) / 2;
    for (long long e = threadIdx.x; e < nz; e += LOC_RED_THREADS) {
      *reinterpret_cast<double2*>(Bre + z0 + 2 * e) = make_double2(0, 0);
      *reinterpret_cast<double2*>(Bre + dpl + z0 + 2 * e) = make_double2(0, 0);
    }
  }
}

int apply_mpo(qk_ctx* c, const qk_mps_set* src, const int32_t* bonds, const double* tensors, qk_mps_set** out) {
  static const char* what = "qk_mps_set_apply_mpo";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!src) return qk_fail(QK_EINVAL, "%s: src is null", what);
  if (!bonds) return qk_fail(QK_EINVAL, "%s: bonds is null", what);
  if (!tensors) return qk_fail(QK_EINVAL, "%s: tensors is null", what);
  if (!out) return qk_fail(QK_EINVAL, "%s: out is null", what);
  *out = nullptr;
  if (src->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (src->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; applying an MPO needs an fp64 set", what);
  const int ns = src->n_states, n = src->n_sites, n1 = n + 1;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  if ((long long)ns * n > std::numeric_limits<int32_t>::max()) return qk_fail(QK_EINVAL, "%s: %d states of %d sites are more (state, site) pairs than a task holds", what, ns, n);
  if (const long long bad = mpo_bad_bond(bonds, 1, n); bad >= 0)
    return qk_fail(QK_EINVAL, "%s: bonds[%d] = %d is outside 1 .. %d (cut %d)", what, (int)bad, bonds[bad], MPO_MAX_BOND, (int)bad);
  for (const int k : {0, n})
    if (bonds[k] != 1) return qk_fail(QK_EINVAL, "%s: bonds[%d] = %d must be 1 (the end of the MPO)", what, k, bonds[k]);
  {
    long long e = 0;
    for (int k = 0; k < n; ++k) {
      const int wr = bonds[k + 1];
      for (long long q = 0; q < 8ll * bonds[k] * wr; ++q, ++e)
        if (!std::isfinite(tensors[e]))
          return qk_fail(QK_EINVAL, "%s: site %d: W[%d][%d][%d][%d] has a %s part that is not finite", what, k, (int)(q / 8 / wr), (int)(q / 8 % wr), (int)(q / 4 % 2), (int)(q / 2 % 2),
                         q % 2 ? "imaginary" : "real");
    }
  }
  const MpoPlan mp = mpo_plan(bonds, tensors, 1, n);
  const ApplyPlan ap = apply_plan(src->dims_true.data(), ns, n, mp);
  if (ap.bad_state >= 0)
    return qk_fail(QK_EINVAL, "%s: state %d, bond %d: the product bond %d x %d = %d is above %d", what, ap.bad_state, ap.bad_bond, bonds[ap.bad_bond],
                   (int)src->dims_true[(size_t)ap.bad_state * n1 + ap.bad_bond], bonds[ap.bad_bond] * (int)src->dims_true[(size_t)ap.bad_state * n1 + ap.bad_bond], APPLY_MAX_BOND);
  if (ap.tasks.size() > (size_t)std::numeric_limits<int32_t>::max()) return qk_fail(QK_EINVAL, "%s: %zu tasks are more than one launch holds", what, ap.tasks.size());
  QkRangeGuard range_("qk:apply_mpo");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  // the tables of the MPO and the tasks, uploaded once: bonds | copy | uat | ufirst | blk_v | blk_w | tasks
  const std::vector<std::pair<const void*, size_t>> regions{{mp.bonds.data(), mp.bonds.size() * sizeof(int32_t)},   {ap.copy.data(), ap.copy.size() * sizeof(int32_t)},
                                                            {ap.uat.data(), ap.uat.size() * sizeof(int32_t)},       {ap.ufirst.data(), ap.ufirst.size() * sizeof(int32_t)},
                                                            {ap.blk_v.data(), ap.blk_v.size() * sizeof(int32_t)},   {ap.blk_w.data(), ap.blk_w.size() * sizeof(double)},
                                                            {ap.tasks.data(), ap.tasks.size() * sizeof(Task2)}};
  std::vector<size_t> rat;
  size_t tab_bytes = 0;
  for (const auto& rg : regions) rat.push_back(tab_bytes), tab_bytes += al256(std::max<size_t>(rg.second, 8));
  QkDevBuf dtab;
  HIP_TRY_AS(what, dtab.alloc(tab_bytes));
  qk_mps_set* m = nullptr;
  if (const int rc = qk_mps_set_alloc(c, ns, n, ap.total * (long long)sizeof(double), 64, &m, what)) return rc;  // QK_EDEVICE names the bytes
  m->max_pad = ap.max_pad;
  m->dims_true = ap.tru;
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < regions.size() && e == hipSuccess; ++i)
    if (regions[i].second) e = hipMemcpyAsync(dtab.get<char>() + rat[i], regions[i].first, regions[i].second, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_dims.get(), ap.pad.data(), ap.pad.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_true.get(), ap.tru.data(), ap.tru.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->d_offs.get(), ap.offs.data(), ap.offs.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    ApplyArgs a{};
    a.src = src->d_data.get<double>(), a.spad = src->d_dims.get<int32_t>(), a.stru = src->d_true.get<int32_t>(), a.soffs = src->d_offs.get<int64_t>();
    a.dst = m->d_data.get<double>(), a.dpad = m->d_dims.get<int32_t>(), a.doffs = m->d_offs.get<int64_t>();
    a.wb = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[0]);
    a.copy = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[1]);
    a.uat = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[2]);
    a.ufirst = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[3]);
    a.blk_v = reinterpret_cast<const int32_t*>(dtab.get<char>() + rat[4]);
    a.blk_w = reinterpret_cast<const double*>(dtab.get<char>() + rat[5]);
    a.tasks = reinterpret_cast<const int2*>(dtab.get<char>() + rat[6]);
    a.n_sites = n;
    qk_mpo_apply_kernel<<<dim3((unsigned)ap.tasks.size()), dim3(LOC_RED_THREADS), 0, c->stream>>>(a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the host tables and dtab go when this returns
  if (e != hipSuccess) {
    qk_mps_set_destroy(m);
    return qk_fail(QK_EDEVICE, "%s: %s", what, hipGetErrorString(e));
  }
  *out = m;
  return QK_OK;
}

// ---- bond purities and entanglement spectra (qk_bond_purities_host, qk_bond_spectra_host) --------------------------------------
// Bond k (k = 1 .. n-1) cuts the chain between sites k-1 and k.  With the kept environments of the environment pass,
//     N_k = R_k L_k^T / <psi|psi>     (chi_k x chi_k, tr N_k = 1; its eigenvalues are the Schmidt weights of the cut)
//     purity_k = tr(N_k^2)
// L_k and R_k are Hermitian in the sweep's X[ket][bra] orientation, so the product the ring GEMM makes from them as they lie,
// M_k = L_k^T R_k, is N_k^H <psi|psi>: the same eigenvalues and the same tr(M^2).  Purities: per bond ONE GEMM launch (LOC_BOND_M,
// tasks (state, 64 x 64 block), into the T planes, which the pass no longer needs) and ONE reduction launch in 16-row chunks
// (qk_bond_trace_kernel); the chunk sums are added in a fixed order.  Spectra: one workgroup per (state, bond) of true bond >= 2
// factorises L_k^T and takes the eigenvalues of the Hermitian H_k = F R_k F^H / <psi|psi> (qk_build.hip: qk_bond_spectra_kernel).
// No atomics on values, no spin wait, no grid barrier: a value is the same bits whatever the other states, the batch cut and the run.
int bond_call(qk_ctx* c, const qk_mps_set* set, const char* what, const char* range, const int32_t max_values, double* out, double* norms) {
  const bool spectra = max_values != 0;
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!set) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!out) return qk_fail(QK_EINVAL, "%s: out is null", what);
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; bond spectra and purities need an fp64 set", what);
  if (spectra && max_values < 1) return qk_fail(QK_EINVAL, "%s: max_values must be >= 1 (got %d)", what, max_values);
  const int ns = set->n_states, n = set->n_sites, n1 = n + 1;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  QkRangeGuard range_(range);
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  const int32_t* tru = set->dims_true.data();
  EnvSizes z;
  env_sizes(tru, ns, n, set->max_pad, LOC_RMUL, true, z);
  const int m = spectra ? max_values : 1;
  const size_t n_out = (size_t)ns * (n - 1) * m;
  QkDevBuf rev, dout, dnorm, derr;
  if (spectra) HIP_TRY_AS(what, derr.alloc(32 * sizeof(int)));
  HIP_TRY_AS(what, rev.alloc((size_t)set->bytes));
  HIP_TRY_AS(what, dout.alloc(std::max<size_t>(1, n_out) * sizeof(double)));
  HIP_TRY_AS(what, dnorm.alloc((size_t)ns * sizeof(double)));
  HIP_TRY_AS(what, hipMemsetAsync(dout.get(), 0, std::max<size_t>(1, n_out) * sizeof(double), c->stream));
  // memory bound of a state batch: a quarter of what is free (at least one state per batch); with the spectra the environments take
  // at most half of it and the factorisation workspaces the rest (at least one workgroup)
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const long long part_per_state = spectra ? 0 : (long long)n * z.max_chunks;
  const std::vector<int> bstart = batch_cut(z.need, part_per_state, spectra ? budget / 2 : budget);
  Plan plan = env_plan(n);
  if (!spectra) {
    const Plan tail = bond_tail(n);
    plan.insert(plan.end(), tail.begin(), tail.end());
  }
  EnvBatch eb;
  std::vector<int2> stasks;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(z, plan, s0, nb, part_per_state, eb);
    size_t extra = 0;
    int grid = 0, qmax = 0;
    size_t per_wg = 0;
    if (spectra) {  // the (state, bond) tasks of the batch and the workspaces of the workgroups that take them in turn
      stasks.clear();
      for (int i = 0; i < nb; ++i)
        for (int k = 1; k < n; ++k) {
          const int q = tru[(size_t)(s0 + i) * n1 + k];
          if (q >= 2) stasks.push_back(int2{i, k}), qmax = std::max(qmax, q);
        }
      if (!stasks.empty()) {
        per_wg = qk_bond_spectra_work_bytes(qmax);
        const long long room = (budget - eb.tot) * (long long)sizeof(double);
        grid = (int)std::max<long long>(1, std::min<long long>({(long long)stasks.size(), 2ll * c->num_cus, room / (long long)per_wg}));
        extra = al256(stasks.size() * sizeof(int2)) + (size_t)grid * per_wg;
      }
    }
    if (const int rc = env_run(c, set, what, rev.get<double>(), z, plan, eb, extra)) return rc;
    const LocArgs& g = eb.g;
    qk_str_norms_kernel<<<dim3((nb + 255) / 256), dim3(256), 0, c->stream>>>(g, nb, dnorm.get<double>());
    if (!spectra && n > 1) qk_bond_purities_kernel<<<dim3((unsigned)(((long long)nb * (n - 1) + 255) / 256)), dim3(256), 0, c->stream>>>(g, nb, dout.get<double>());
    HIP_TRY_AS(what, hipGetLastError());
    if (grid > 0) {
      char* const x0 = eb.base + eb.used();
      HIP_TRY_AS(what, hipMemcpyAsync(x0, stasks.data(), stasks.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
      QkSpectraArgs a{};
      a.env = g.scratch, a.dims = g.dims, a.tru = g.tru, a.states = g.states, a.pmax = g.pmax, a.sbase = g.sbase, a.roff = g.roff, a.loff = g.loff;
      a.tasks = reinterpret_cast<const int2*>(x0), a.n_tasks = (int)stasks.size();
      a.work = x0 + al256(stasks.size() * sizeof(int2)), a.work_bytes = (long long)per_wg, a.qmax = qmax;
      a.out = dout.get<double>(), a.n_sites = n, a.max_values = m, a.rmul = z.rmul, a.error = derr.get<int>();
      if (const int rc = qk_bond_spectra_launch(c, a, grid, what)) return rc;  // synchronises and reads the error word
    }
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the staged tables are reused by the next batch
  }
  if (n_out) HIP_TRY_AS(what, hipMemcpy(out, dout.get(), n_out * sizeof(double), hipMemcpyDeviceToHost));
  if (norms) HIP_TRY_AS(what, hipMemcpy(norms, dnorm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
  if (spectra)  // a bond of true dimension 1 has the single weight 1 exactly
    for (int s = 0; s < ns; ++s)
      for (int k = 1; k < n; ++k)
        if (tru[(size_t)s * n1 + k] < 2) out[((size_t)s * (n - 1) + k - 1) * m] = 1.0;
  return QK_OK;
}

// ---- block kernels: reduced-state overlaps of the first or last w qubits (qk_block_values_host, qk_block_self_host) -------------
// A = the first w qubits (side 0, cut at bond w) or the last w (side 1, cut at bond m = n - w).  For a pair (x_i, y_j), with the
// mixed left environment E_w[b][a] = <l^x_a | l^y_b> of the fidelity sweep (X[ket][bra]) and the self right environments of the
// environment pass,
//     tr(rho_A(x) rho_A(y)) <x|x> <y|y> = sum_{a,a',b,b'} Rx_w[a][a'] Ry_w[b][b'] E_w[b][a'] conj(E_w[b'][a])
// and the mirror image for side 1: the same chain on the reversed images (LocArgs.rev) against the self LEFT environments L_m.
// Per call: the environment pass of each set in state batches (env_plan; every L_k and R_k of a batch), from which the
// environments of the chosen cuts are copied into one compact buffer (qk_local_plan.h: blk_kept_offsets) and the norms taken; then
// the pairs in pair batches.  A pair chain has the string chain's slot (E | T).  Per step ONE BLK_T and ONE BLK_X launch for every
// chain of the batch (the two GEMMs of the ring sweep, A_k of the y state then conj(A_k) of the x state); behind the step of a
// chosen width three more: V = Ry^T E and W = E^T conj(V) into the T region (dead between two steps) and the reduction
// Re sum Rx[a][a'] conj(W[a][a']) in 16-row chunks.  A chain starts from the unit matrix at the head of the kept buffer.  The chunk
// sums are added in a fixed order, nothing of a chain depends on another chain, no atomics, no grid barrier, no spin wait: a
// (pair, width) value is the same bits whatever the other pairs, the other widths, the cut into batches (QK_BLOCK_BATCH caps the
// chains of one) and the run.
struct BlkSet {
  const double* data;     // the set's planes (side 0) or their reversed image (side 1)
  const int32_t* dims;    // padded bonds [n_states][n_sites + 1]
  const int32_t* tru;     // true bonds
  const int64_t* offs;    // re-plane offsets [n_states][n_sites]
  const int64_t* koff;    // [n_states][n_widths]: the kept environment of (state, cut) in `kept`
  const double* norms;    // [n_states]: <psi|psi>
};
struct BlkArgs {
  BlkSet x, y;
  const int32_t* pairs;   // chain -> (x state, y state)
  const int32_t* cpm;     // chain -> P = max(P_x, P_y)
  const int64_t* cbase;   // chain -> first double of its slot
  const int32_t* widths;  // [n_widths]
  const int2* tasks;      // this launch: (chain, block)
  const double* kept;     // the unit matrix, then the environments of the chosen cuts
  double* slots;
  double* part;           // partial sums [chain][n_widths][max chunks]
  int n_sites, side, n_widths, max_chunks;
  int step;               // step j of the chain
  int cut;                // index of the width (BLK_V, BLK_W, BLK_RED)
};

// One 64 x 64 output block of one pair chain's GEMM.  CONJB = false: BLK_T, BLK_V; true: BLK_X, BLK_W.
template <bool CONJB>
__global__ __launch_bounds__(512) void qk_blk_gemm_kernel(const BlkArgs g, const int kind) {
  __shared__ __attribute__((aligned(16))) double lds[LOC_LDS_DOUBLES];
  const int2 t = g.tasks[blockIdx.x];
  const int ch = __builtin_amdgcn_readfirstlane(t.x);
  const int blk = __builtin_amdgcn_readfirstlane(t.y);
  const long long xi = __builtin_amdgcn_readfirstlane(g.pairs[2 * ch]), yj = __builtin_amdgcn_readfirstlane(g.pairs[2 * ch + 1]);
  const int n = g.n_sites, n1 = n + 1, j = g.step;
  const int site = blk_site(g.side, j, n), in = blk_in(g.side, j, n), out = blk_out(g.side, j, n);
  const int xl = __builtin_amdgcn_readfirstlane(g.x.dims[xi * n1 + in]), xr = __builtin_amdgcn_readfirstlane(g.x.dims[xi * n1 + out]);
  const int yl = __builtin_amdgcn_readfirstlane(g.y.dims[yj * n1 + in]), yr = __builtin_amdgcn_readfirstlane(g.y.dims[yj * n1 + out]);
  const long long P = __builtin_amdgcn_readfirstlane(g.cpm[ch]), P2 = P * P;
  double* const E = g.slots + uni64(g.cbase[ch]);
  double* const T = E + chain_T() * P2;
  const double *Are, *Aim, *Bre, *Bim;
  double *Cre, *Cim;
  int lda, ldb, ldc, M, N, K;
  if (kind == BLK_T) {
    if (j == 0) {  // the chain starts here: E = 1
      Are = g.kept, Aim = g.kept + 256;
    } else {
      Are = E, Aim = E + P2;
    }
    Bre = g.y.data + uni64(g.y.offs[yj * n + site]);
    Bim = Bre + (long long)yl * 2 * yr;
    Cre = T, Cim = T + 2 * P2;
    lda = xl, ldb = 2 * yr, ldc = 2 * yr, M = xl, N = 2 * yr, K = __builtin_amdgcn_readfirstlane(g.y.tru[yj * n1 + in]);
  } else if (kind == BLK_X) {
    Are = T, Aim = T + 2 * P2;
    Bre = g.x.data + uni64(g.x.offs[xi * n + site]);
    Bim = Bre + (long long)xl * 2 * xr;
    Cre = E, Cim = E + P2;
    lda = yr, ldb = xr, ldc = xr, M = yr, N = xr, K = 2 * __builtin_amdgcn_readfirstlane(g.x.tru[xi * n1 + in]);
  } else {
    double* const V = E + blk_V() * P2;
    const int yt = __builtin_amdgcn_readfirstlane(g.y.tru[yj * n1 + out]);
    if (kind == BLK_V) {  // V[b'][a'] = sum_b Ry[b][b'] E[b][a']
      Are = g.kept + uni64(g.y.koff[yj * g.n_widths + g.cut]);
      Aim = Are + (long long)yr * yr;
      Bre = E, Bim = E + P2;
      Cre = V, Cim = V + P2;
      lda = yr, ldb = xr, ldc = xr, M = yr, N = xr, K = yt;
    } else {  // W[a][a'] = sum_b' E[b'][a] conj(V[b'][a'])
      double* const W = E + blk_W() * P2;
      Are = E, Aim = E + P2;
      Bre = V, Bim = V + P2;
      Cre = W, Cim = W + P2;
      lda = xr, ldb = xr, ldc = xr, M = xr, N = xr, K = yt;
    }
  }
  const int npm = (M + 63) / 64;
  const int m0 = 64 * (blk % npm), n0 = 64 * (blk / npm);
  zgemm_ring3<CONJB, LOC_KTL, LOC_NSLOT, true, 8, 64, double, 9>(Cre + (long long)m0 * ldc + n0, Cim + (long long)m0 * ldc + n0, ldc, Are + m0, Aim + m0, lda,
                                                                  Bre + n0, Bim + n0, ldb, min(64, M - m0), min(64, N - n0), K, lds);
}

// Re sum_{a, a'} Rx[a][a'] conj(W[a][a']) over one 16-row chunk of a, unnormalised: part[(chain, cut, chunk)].
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_blk_reduce_kernel(const BlkArgs g) {
  __shared__ double red[1][LOC_RED_THREADS];
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const long long xi = g.pairs[2 * ch];
  const int n = g.n_sites;
  const int r = g.x.dims[xi * (n + 1) + blk_out(g.side, g.step, n)];
  const long long P = g.cpm[ch], P2 = P * P, rpl = (long long)r * r;
  const double* const W = g.slots + g.cbase[ch] + blk_W() * P2;
  const double* const R = g.kept + g.x.koff[xi * g.n_widths + g.cut];
  double acc[1] = {};
  const int rows = LOC_CHUNK * r;
  for (int e = threadIdx.x; e < rows; e += LOC_RED_THREADS) {
    const long long q = (long long)c * rows + e;
    acc[0] += R[q] * W[q] + R[q + rpl] * W[q + P2];
  }
  tree_sum(red, acc);
  if (threadIdx.x == 0) g.part[((long long)ch * g.n_widths + g.cut) * g.max_chunks + c] = red[0][0];
}

// The values of a pair batch: the chunk sums of each (chain, cut) in a fixed order, divided by the two norms.
__global__ __launch_bounds__(256) void qk_blk_values_kernel(const BlkArgs g, const int nc, const long long pair0, const long long n_pairs, double* out) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)nc * g.n_widths) return;
  const int ch = (int)(id / g.n_widths), ci = (int)(id % g.n_widths);
  const long long xi = g.pairs[2 * ch], yj = g.pairs[2 * ch + 1];
  const int n = g.n_sites;
  const int chunks = g.x.dims[xi * (n + 1) + blk_cut_bond(g.side, g.widths[ci], n)] / LOC_CHUNK;
  const double* p = g.part + ((long long)ch * g.n_widths + ci) * g.max_chunks;
  double v = 0;
  for (int c = 0; c < chunks; ++c) v += p[c];
  out[ci * n_pairs + pair0 + ch] = v / (g.x.norms[xi] * g.y.norms[yj]);
}

// The environments of the chosen cuts of a state batch, out of the environment pass into the kept buffer: R of the cut's bond
// (side 0) or L (side 1), both planes.
__global__ __launch_bounds__(256) void qk_blk_keep_kernel(const LocArgs g, const int side, const int n_widths, const int32_t* widths, const int64_t* koff, double* kept) {
  const int i = blockIdx.x, ci = blockIdx.y;
  const int n = g.n_sites, n1 = n + 1;
  const long long st = g.states[i];
  const int bond = blk_cut_bond(side, widths[ci], n);
  const long long d = g.dims[st * n1 + bond], P = g.pmax[i];
  const double* const src = g.scratch + g.sbase[i] + g.rmul * P * P + (side ? g.loff : g.roff)[(long long)i * n1 + bond];
  double* const dst = kept + koff[st * n_widths + ci];
  for (long long e = threadIdx.x; e < 2 * d * d; e += 256) dst[e] = src[e];
}

// what a set brings to a block call: its environment pass into `kept`, its norms and its reversed image
struct BlkHostSet {
  const qk_mps_set* set = nullptr;
  EnvSizes z;
  std::vector<int64_t> koff;
  QkDevBuf rev, dnorm;
  const int64_t* d_koff = nullptr;
};
int blk_env_pass(qk_ctx* c, const char* what, BlkHostSet& h, const int side, const int nw, const int32_t* d_widths, double* kept, const long long budget) {
  const int n = h.set->n_sites;
  const std::vector<int> bstart = batch_cut(h.z.need, 0, budget);
  const Plan plan = env_plan(n);
  EnvBatch eb;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(h.z, plan, s0, nb, 0, eb);
    if (const int rc = env_run(c, h.set, what, h.rev.get<double>(), h.z, plan, eb, 0)) return rc;
    qk_str_norms_kernel<<<dim3((nb + 255) / 256), dim3(256), 0, c->stream>>>(eb.g, nb, h.dnorm.get<double>());
    qk_blk_keep_kernel<<<dim3(nb, nw), dim3(256), 0, c->stream>>>(eb.g, side, nw, d_widths, h.d_koff, kept);
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the staged tables are reused by the next batch
  }
  return QK_OK;
}

// values_host[n_widths][n_pairs] = O_w of the pairs (x state, y state) as listed; norms_host (may be NULL) = <psi|psi> of the x set
int block_run(qk_ctx* c, const char* what, const qk_mps_set* xset, const qk_mps_set* yset, const long long n_pairs, const int32_t* pairs, const int side, const int nw,
              const int32_t* widths, double* values_host, double* norms_host) {
  const int n = xset->n_sites;
  long long cap = 0;  // pair chains per batch
  if (const int rc = batch_cap(what, "QK_BLOCK_BATCH", cap)) return rc;
  if (n_pairs == 0) return QK_OK;
  QkRangeGuard range_("qk:block_values");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  const bool sym = !yset || yset == xset;
  BlkHostSet hx, hy_;
  BlkHostSet& hy = sym ? hx : hy_;
  hx.set = xset, hy.set = sym ? xset : yset;
  long long kept_doubles = blk_kept_unit();
  for (BlkHostSet* h : {&hx, &hy_}) {
    if (h == &hy_ && sym) break;
    env_sizes(h->set->dims_true.data(), h->set->n_states, n, h->set->max_pad, LOC_RMUL, true, h->z);
    kept_doubles = blk_kept_offsets(h->z, side, nw, widths, kept_doubles, h->koff);
    HIP_TRY_AS(what, h->rev.alloc((size_t)h->set->bytes));
    HIP_TRY_AS(what, h->dnorm.alloc((size_t)h->set->n_states * sizeof(double)));
  }
  const int max_chunks = std::max(hx.z.max_chunks, hy.z.max_chunks);
  // the call's small tables: [widths | koff of x | koff of y]
  const size_t b_w = al256(nw * sizeof(int32_t)), b_kx = al256(hx.koff.size() * sizeof(int64_t)), b_ky = sym ? 0 : al256(hy.koff.size() * sizeof(int64_t));
  QkDevBuf dtab, dout, kept;
  HIP_TRY_AS(what, dtab.alloc(b_w + b_kx + b_ky));
  HIP_TRY_AS(what, dout.alloc((size_t)nw * n_pairs * sizeof(double)));
  HIP_TRY_AS(what, hipMemcpy(dtab.get<char>(), widths, nw * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY_AS(what, hipMemcpy(dtab.get<char>() + b_w, hx.koff.data(), hx.koff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  if (!sym) HIP_TRY_AS(what, hipMemcpy(dtab.get<char>() + b_w + b_kx, hy.koff.data(), hy.koff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  const int32_t* d_widths = dtab.get<int32_t>();
  hx.d_koff = reinterpret_cast<const int64_t*>(dtab.get<char>() + b_w);
  hy.d_koff = sym ? hx.d_koff : reinterpret_cast<const int64_t*>(dtab.get<char>() + b_w + b_kx);
  // the kept environments of the chosen cuts, for every state of both sets: they must fit a quarter of what is free
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  if (kept_doubles > budget)
    return qk_fail(QK_EDEVICE, "%s: the environments of the %d chosen cuts need %lld bytes, more than a quarter of the free device memory (%lld bytes)", what, nw,
                   kept_doubles * (long long)sizeof(double), budget * (long long)sizeof(double));
  HIP_TRY_AS(what, kept.alloc((size_t)kept_doubles * sizeof(double)));
  {
    std::vector<double> unit((size_t)blk_kept_unit(), 0.0);
    unit[0] = 1.0;
    HIP_TRY_AS(what, hipMemcpy(kept.get(), unit.data(), unit.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // memory bound of a state batch and of a pair batch: a quarter of what is free now (at least one state / one chain per batch)
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  if (const int rc = blk_env_pass(c, what, hx, side, nw, d_widths, kept.get<double>(), budget)) return rc;
  if (!sym)
    if (const int rc = blk_env_pass(c, what, hy, side, nw, d_widths, kept.get<double>(), budget)) return rc;

  const std::vector<BlkLaunch> plan = blk_plan(nw, widths);
  const BlkChains chains = list_blk_chains(hx.z, hy.z, n_pairs, pairs, side, plan, nw);
  const std::vector<size_t> cstart = chain_cut(chains.weight, budget, cap);
  BlkArgs q{};
  auto side_of = [&](const BlkHostSet& h) {
    return BlkSet{side ? h.rev.get<double>() : h.set->d_data.get<double>(), h.set->d_dims.get<int32_t>(), h.set->d_true.get<int32_t>(), h.set->d_offs.get<int64_t>(), h.d_koff,
                  h.dnorm.get<double>()};
  };
  q.x = side_of(hx), q.y = side_of(hy);
  q.widths = d_widths, q.kept = kept.get<double>();
  q.n_sites = n, q.side = side, q.n_widths = nw, q.max_chunks = max_chunks;
  std::vector<int32_t> h_cpm((size_t)n_pairs);  // P of every pair chain
  for (long long e = 0; e < n_pairs; ++e) h_cpm[e] = std::max(hx.z.pmax[pairs[2 * e]], hy.z.pmax[pairs[2 * e + 1]]);
  const std::vector<ChainCol> cols{{pairs, sizeof(int32_t), 2}, {h_cpm.data(), sizeof(int32_t), 1}};
  // no state batch is around a pair batch: its buffer is the start of the context's scratch
  const int rc = chain_run(
      c, what, nullptr, cols, chains, cstart, (long long)nw * max_chunks,
      [&](size_t c0, size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) { blk_lists(hx.z, hy.z, pairs, c0, nc, side, plan, tasks, first); },
      [&](const ChainBatch& b) {
        q.pairs = reinterpret_cast<const int32_t*>(b.base + b.st.col[0]);
        q.cpm = reinterpret_cast<const int32_t*>(b.base + b.st.col[1]);
        q.cbase = reinterpret_cast<const int64_t*>(b.base + b.st.col[2]);
        const int2* d_tasks = reinterpret_cast<const int2*>(b.base + b.st.tasks);
        q.part = reinterpret_cast<double*>(b.base + b.st.part);
        q.slots = reinterpret_cast<double*>(b.base + b.st.slots);
        each_launch(b.first, [&](const size_t li, const long long t0, const dim3 grid) {
          const int kind = plan[li].kind;
          q.tasks = d_tasks + t0;
          q.step = plan[li].step, q.cut = plan[li].cut;
          if (kind == BLK_RED) qk_blk_reduce_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(q);
          else if (conj_b(kind)) qk_blk_gemm_kernel<true><<<grid, dim3(512), 0, c->stream>>>(q, kind);
          else qk_blk_gemm_kernel<false><<<grid, dim3(512), 0, c->stream>>>(q, kind);
        });
        qk_blk_values_kernel<<<dim3((unsigned)((b.nc * nw + 255) / 256)), dim3(256), 0, c->stream>>>(q, (int)b.nc, (long long)b.c0, n_pairs, dout.get<double>());
      });
  if (rc) return rc;
  HIP_TRY_AS(what, hipMemcpy(values_host, dout.get(), (size_t)nw * n_pairs * sizeof(double), hipMemcpyDeviceToHost));
  if (norms_host) HIP_TRY_AS(what, hipMemcpy(norms_host, hx.dnorm.get(), (size_t)xset->n_states * sizeof(double), hipMemcpyDeviceToHost));
  return QK_OK;
}

// the checks both entry points share, before anything runs on the device
int block_check(qk_ctx* c, const char* what, const qk_mps_set* xset, const qk_mps_set* yset, const int side, const int nw, const int32_t* widths) {
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!xset) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!widths) return qk_fail(QK_EINVAL, "%s: widths is null", what);
  for (const qk_mps_set* s : {xset, yset}) {
    if (!s) continue;
    if (s->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
    if (s->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; block overlaps need an fp64 set", what);
    if (s->n_sites < 1 || s->n_states < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  }
  if (yset && yset->n_sites != xset->n_sites) return qk_fail(QK_EINVAL, "%s: site counts differ (%d, %d)", what, xset->n_sites, yset->n_sites);
  if (side != 0 && side != 1) return qk_fail(QK_EINVAL, "%s: side must be 0 (left) or 1 (right) (got %d)", what, side);
  if (nw < 1) return qk_fail(QK_EINVAL, "%s: n_widths must be >= 1 (got %d)", what, nw);
  if (const int bad = blk_bad_width(nw, widths, xset->n_sites); bad >= 0)
    return qk_fail(QK_EINVAL, "%s: widths[%d] = %d: widths must be strictly increasing in 1 .. n_sites = %d", what, bad, widths[bad], xset->n_sites);
  return QK_OK;
}

// ---- measurement shots (qk_sample_host) -----------------------------------------------------------------------------------------
// Perfect sampling of every state of a set, each shot and qubit in its own Pauli basis (codes 1..3 = X, Y, Z; outcome bit 0 =
// eigenvalue +1).  One shot, v = [1] a row vector over the left bond, for k = 0 .. n-1:
//     W_t[b']  = sum_b v[b] A_k[b][t][b']                                   t = 0, 1
//     Z: W'_0 = W_0, W'_1 = W_1;   X: W'_0 = (W_0 + W_1)/sqrt2, W'_1 = (W_0 - W_1)/sqrt2;   Y: W'_0 = (W_0 - i W_1)/sqrt2, W'_1 = (W_0 + i W_1)/sqrt2
//     p_o      = max(0, Re sum_{b',a'} W'_o[b'] R_{k+1}[b'][a'] conj(W'_o[a'])),   tot = p_0 + p_1
//     u        = smp_uniform(seed, global state index, shot, k)
//     bit      = 1 if (p_1 > 0 and u tot >= p_0) else 0;   logp += log(p_bit / tot);   v = W'_bit / sqrt(p_bit)
// exp(logp) is the probability of the drawn string in the drawn bases.  Per state batch the reversed chain keeps every R_k
// (sample_env_plan); a shot chain is one (state, tile of SMP_TILE shots) with its own slot (qk_local_plan.h).  At site k every chain
// of the chain batch goes through ONE launch of each of: SMP_W (GEMM, shot rows as M), SMP_ROT (the rotation by each row's code,
// written as the stacked K-major operand), SMP_Q (GEMM, the stacked rows as M) and SMP_DRAW (one wave per row: the two sums over
// the true bond in a fixed order, the uniform, the bit, log p and the next v).  4 n_sites launches per chain batch, whatever the
// number of shots.  A row of a GEMM is a sum over K in the ring GEMM's fixed order whatever its block, nothing of a row depends on
// another row, no atomics, no grid barrier: the bits and log p of a (state, shot) are the same whatever the other states and shots,
// the cut into batches and tiles (QK_SAMPLE_BATCH caps the chains of a batch) and the run.  Only the columns below the true bond
// enter a probability.
struct SmpArgs {
  LocArgs e;              // the set and the state batch of the environment pass: e.scratch holds every R_k
  const int32_t* cent;    // chain -> batch entry
  const int32_t* shot0;   // chain -> its first shot
  const int32_t* rows;    // chain -> its shots
  const int64_t* cbase;   // chain -> first double of its slot
  const uint8_t* bases;   // [n_shots][n_sites], NULL: all Z
  const int2* tasks;      // this launch: (chain, block)
  double* slots;
  uint8_t* bits;          // [n_states][n_shots][n_sites]
  double* logp;           // [n_states][n_shots]
  int32_t* bad;           // [chain]: 1 where a row's tot was 0 or not finite
  unsigned long long seed;
  long long first_state;  // global index of state 0 of the set
  int n_shots;
  int step;               // site k
};

// One 64 x 64 output block of one shot chain's GEMM at site k (SMP_W or SMP_Q).
__global__ __launch_bounds__(512) void qk_smp_gemm_kernel(const SmpArgs g, const int kind) {
  __shared__ __attribute__((aligned(16))) double lds[LOC_LDS_DOUBLES];
  const int2 t = g.tasks[blockIdx.x];
  const int ch = __builtin_amdgcn_readfirstlane(t.x);
  const int blk = __builtin_amdgcn_readfirstlane(t.y);
  const int i = __builtin_amdgcn_readfirstlane(g.cent[ch]);
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = __builtin_amdgcn_readfirstlane(g.e.states[i]);
  const int l = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k]), r = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k + 1]);
  const long long P = __builtin_amdgcn_readfirstlane(g.e.pmax[i]);
  const int R = smp_rows_pad(__builtin_amdgcn_readfirstlane(g.rows[ch]));
  const long long PR = P * R;
  double* const slot = g.slots + uni64(g.cbase[ch]);
  const double *Are, *Aim, *Bre, *Bim;
  double *Cre, *Cim;
  int lda, ldb, ldc, M, N, K;
  if (kind == SMP_W) {
    Are = slot + smp_V() * PR, Aim = Are + PR;
    Bre = g.e.data + uni64(g.e.offs[st * n + k]);
    Bim = Bre + (long long)l * 2 * r;
    Cre = slot + smp_W() * PR, Cim = Cre + 2 * PR;
    lda = R, ldb = 2 * r, ldc = 2 * r, M = R, N = 2 * r, K = __builtin_amdgcn_readfirstlane(g.e.tru[st * n1 + k]);
  } else {
    Are = slot + smp_Ws() * PR, Aim = Are + 2 * PR;
    Bre = g.e.scratch + uni64(g.e.sbase[i]) + g.e.rmul * P * P + uni64(g.e.roff[(long long)i * n1 + k + 1]);
    Bim = Bre + (long long)r * r;
    Cre = slot + smp_Q() * PR, Cim = Cre + 2 * PR;
    lda = 2 * R, ldb = r, ldc = r, M = 2 * R, N = r, K = __builtin_amdgcn_readfirstlane(g.e.tru[st * n1 + k + 1]);
  }
  const int npm = (M + 63) / 64;
  const int m0 = 64 * (blk % npm), n0 = 64 * (blk / npm);
  zgemm_ring3<false, LOC_KTL, LOC_NSLOT, true, 8, 64, double, 10>(Cre + (long long)m0 * ldc + n0, Cim + (long long)m0 * ldc + n0, ldc, Are + m0, Aim + m0, lda,
                                                                   Bre + n0, Bim + n0, ldb, min(64, M - m0), min(64, N - n0), K, lds);
}

// (W'_0, W'_1) of (W_0, W_1) in the basis `code` (1..3 = X, Y, Z)
__device__ __forceinline__ void smp_rotate(const int code, const double w0r, const double w0i, const double w1r, const double w1i, double& a0r, double& a0i, double& a1r,
                                           double& a1i) {
  constexpr double h = 0.70710678118654752440;
  if (code == 1) a0r = (w0r + w1r) * h, a0i = (w0i + w1i) * h, a1r = (w0r - w1r) * h, a1i = (w0i - w1i) * h;
  else if (code == 2) a0r = (w0r + w1i) * h, a0i = (w0i - w1r) * h, a1r = (w0r - w1i) * h, a1i = (w0i + w1r) * h;
  else a0r = w0r, a0i = w0i, a1r = w1r, a1i = w1i;
}
__device__ __forceinline__ int smp_code(const SmpArgs& g, const int ch, const int row) {
  return (g.bases && row < g.rows[ch]) ? g.bases[(long long)(g.shot0[ch] + row) * g.e.n_sites + g.step] : 3;
}

// v = [1] of every shot of a chain: V[0][row] = 1, the rest of the first 16 bond rows (pad_0 = 16) and the pad rows 0.
__global__ __launch_bounds__(256) void qk_smp_init_kernel(const SmpArgs g) {
  const int ch = blockIdx.x;
  const int rows = g.rows[ch], R = smp_rows_pad(rows);
  const long long PR = (long long)g.e.pmax[g.cent[ch]] * R;
  double* const V = g.slots + g.cbase[ch] + smp_V() * PR;
  for (int e = threadIdx.x; e < LOC_CHUNK * R; e += 256) V[e] = (e < rows) ? 1.0 : 0.0, V[PR + e] = 0.0;
  if (threadIdx.x == 0) g.bad[ch] = 0;
}

// The rotation of one 16-row chunk of shots: W[row][(t, b')] -> the stacked operand W'[b'][(o, row)], every padded column (zero
// from the true bond on).
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_smp_rotate_kernel(const SmpArgs g) {
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const int i = g.cent[ch];
  const int n1 = g.e.n_sites + 1, k = g.step;
  const long long st = g.e.states[i];
  const int r = g.e.dims[st * n1 + k + 1], rt = g.e.tru[st * n1 + k + 1];
  const int R = smp_rows_pad(g.rows[ch]);
  const long long PR = (long long)g.e.pmax[i] * R;
  double* const slot = g.slots + g.cbase[ch];
  const double* const W = slot + smp_W() * PR;
  double* const Ws = slot + smp_Ws() * PR;
  for (int e = threadIdx.x; e < LOC_CHUNK * r; e += LOC_RED_THREADS) {
    const int row = c * LOC_CHUNK + (e & (LOC_CHUNK - 1)), bp = e / LOC_CHUNK;
    double a0r = 0, a0i = 0, a1r = 0, a1i = 0;
    if (bp < rt) {
      const long long w = (long long)row * 2 * r + bp;
      smp_rotate(smp_code(g, ch, row), W[w], W[w + 2 * PR], W[w + r], W[w + r + 2 * PR], a0r, a0i, a1r, a1i);
    }
    const long long q = (long long)bp * 2 * R + row;
    Ws[q] = a0r, Ws[q + 2 * PR] = a0i, Ws[q + R] = a1r, Ws[q + R + 2 * PR] = a1i;
  }
}

// The draw of one 16-row chunk of shots, one wave per row (four rows each): p_o = Re sum_{a'} Q[(o, row)][a'] conj(W'_o[row][a'])
// over the true bond -- lane j adds a' = j, j + 64, .. in order, then the lanes in a fixed butterfly -- the uniform, the bit,
// log p, and the next v = W'_bit / sqrt(p_bit) into V (K-major; zero from the true bond on, and for a pad row).
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_smp_draw_kernel(const SmpArgs g) {
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const int i = g.cent[ch];
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.e.states[i];
  const int r = g.e.dims[st * n1 + k + 1], rt = g.e.tru[st * n1 + k + 1];
  const int rows = g.rows[ch], R = smp_rows_pad(rows);
  const long long PR = (long long)g.e.pmax[i] * R;
  double* const slot = g.slots + g.cbase[ch];
  const double* const W = slot + smp_W() * PR;
  const double* const Q = slot + smp_Q() * PR;
  double* const V = slot + smp_V() * PR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = 0; j < LOC_CHUNK / 4; ++j) {
    const int row = c * LOC_CHUNK + 4 * wave + j;
    const bool valid = row < rows;
    const int code = smp_code(g, ch, row);
    const double* const Wrow = W + (long long)row * 2 * r;
    const double* const Q0 = Q + (long long)row * r;
    const double* const Q1 = Q + (long long)(R + row) * r;
    double p0 = 0, p1 = 0;
    for (int a = lane; a < rt; a += 64) {
      double a0r, a0i, a1r, a1i;
      smp_rotate(code, Wrow[a], Wrow[a + 2 * PR], Wrow[a + r], Wrow[a + r + 2 * PR], a0r, a0i, a1r, a1i);
      p0 += Q0[a] * a0r + Q0[a + 2 * PR] * a0i;
      p1 += Q1[a] * a1r + Q1[a + 2 * PR] * a1i;
    }
    for (int m = 32; m > 0; m >>= 1) p0 += __shfl_xor(p0, m), p1 += __shfl_xor(p1, m);
    p0 = fmax(0.0, p0), p1 = fmax(0.0, p1);
    const double tot = p0 + p1;
    const bool ok = valid && tot > 0.0 && isfinite(tot);
    const long long shot = g.shot0[ch] + row;
    const double u = smp_uniform(g.seed, (uint32_t)(g.first_state + st), (uint32_t)shot, (uint32_t)k);
    const int bit = (ok && p1 > 0.0 && u * tot >= p0) ? 1 : 0;
    const double pb = bit ? p1 : p0;
    if (valid && lane == 0) {
      const long long o = st * g.n_shots + shot;
      g.bits[o * n + k] = (uint8_t)bit;
      g.logp[o] = (k ? g.logp[o] : 0.0) + (ok ? log(pb / tot) : 0.0);
      if (!ok) g.bad[ch] = 1;
    }
    if (k + 1 < n) {
      const double s = sqrt(pb);
      for (int a = lane; a < r; a += 64) {
        double vr = 0, vi = 0;
        if (ok && a < rt) {
          double a0r, a0i, a1r, a1i;
          smp_rotate(code, Wrow[a], Wrow[a + 2 * PR], Wrow[a + r], Wrow[a + r + 2 * PR], a0r, a0i, a1r, a1i);
          vr = (bit ? a1r : a0r) / s, vi = (bit ? a1i : a0i) / s;
        }
        V[(long long)a * R + row] = vr, V[(long long)a * R + row + PR] = vi;
      }
    }
  }
}

int sample_run(qk_ctx* c, const qk_mps_set* set, const int32_t n_shots, const uint8_t* bases, const uint64_t seed, const int64_t first_state, uint8_t* bits, double* logp) {
  static const char* what = "qk_sample_host";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!set) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!bits) return qk_fail(QK_EINVAL, "%s: bits is null", what);
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; sampling needs an fp64 set", what);
  if (n_shots < 1) return qk_fail(QK_EINVAL, "%s: n_shots must be >= 1 (got %d)", what, n_shots);
  const int ns = set->n_states, n = set->n_sites;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  if (first_state < 0 || first_state + ns > (1ll << 32))
    return qk_fail(QK_EINVAL, "%s: first_state must be >= 0 and first_state + n_states <= 2^32 (got %lld)", what, (long long)first_state);
  if (bases)
    if (const long long bad = smp_bad_basis(bases, (long long)n_shots * n); bad >= 0)
      return qk_fail(QK_EINVAL, "%s: bases[%lld][%lld] = %d is not a basis code (1..3 = X, Y, Z)", what, bad / n, bad % n, bases[bad]);
  long long cap = 0;  // shot chains per batch
  if (const int rc = batch_cap(what, "QK_SAMPLE_BATCH", cap)) return rc;
  QkRangeGuard range_("qk:sample");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  EnvSizes z;
  env_sizes(set->dims_true.data(), ns, n, set->max_pad, LOC_RMUL, false, z);
  const size_t n_rows = (size_t)ns * n_shots, b_bits = al256(n_rows * n), b_bases = bases ? al256((size_t)n_shots * n) : 0;
  QkDevBuf rev, dbits, dlogp, dbases;
  HIP_TRY_AS(what, rev.alloc((size_t)set->bytes));
  HIP_TRY_AS(what, dbits.alloc(b_bits));
  HIP_TRY_AS(what, dlogp.alloc(n_rows * sizeof(double)));
  if (bases) {
    HIP_TRY_AS(what, dbases.alloc(b_bases));
    HIP_TRY_AS(what, hipMemcpy(dbases.get(), bases, (size_t)n_shots * n, hipMemcpyHostToDevice));
  }
  // memory bound of a state batch (its right environments and the slots of its shot chains): a quarter of what is free; the
  // environments of a batch take at most half of that (at least one state per batch), the chains of a batch the rest (at least one)
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const std::vector<int> bstart = batch_cut(z.need, 0, budget / 2);
  const Plan plan = sample_env_plan(n);
  std::vector<int32_t> h_bad;
  EnvBatch eb;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(z, plan, s0, nb, 0, eb);
    const SmpChains ch = list_smp_chains(z, s0, nb, n_shots, SMP_TILE);
    const std::vector<size_t> cstart = chain_cut(ch.weight, budget - eb.tot, cap);
    // bad: the device raises a chain's entry where a shot has no outcome to draw, and the host reads the column back
    const std::vector<ChainCol> cols{{ch.cent.data(), sizeof(int32_t), 1}, {ch.shot0.data(), sizeof(int32_t), 1}, {ch.rows.data(), sizeof(int32_t), 1}, {nullptr, sizeof(int32_t), 1}};
    if (const int rc = env_run(c, set, what, rev.get<double>(), z, plan, eb, chain_stage_max(cols, ch, cstart, 0))) return rc;
    SmpArgs q{};
    q.e = eb.g;
    q.bases = bases ? dbases.get<uint8_t>() : nullptr;
    q.bits = dbits.get<uint8_t>(), q.logp = dlogp.get<double>();
    q.seed = seed, q.first_state = first_state, q.n_shots = n_shots;
    const int rc = chain_run(
        c, what, eb.base + eb.used(), cols, ch, cstart, 0,
        [&](size_t c0, size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) { smp_lists(z, s0, ch, c0, nc, tasks, first); },
        [&](const ChainBatch& b) {
          q.cent = reinterpret_cast<const int32_t*>(b.base + b.st.col[0]);
          q.shot0 = reinterpret_cast<const int32_t*>(b.base + b.st.col[1]);
          q.rows = reinterpret_cast<const int32_t*>(b.base + b.st.col[2]);
          q.bad = reinterpret_cast<int32_t*>(b.base + b.st.col[3]);
          q.cbase = reinterpret_cast<const int64_t*>(b.base + b.st.col[4]);
          const int2* d_ctasks = reinterpret_cast<const int2*>(b.base + b.st.tasks);
          q.slots = reinterpret_cast<double*>(b.base + b.st.slots);
          qk_smp_init_kernel<<<dim3((unsigned)b.nc), dim3(256), 0, c->stream>>>(q);
          each_launch(b.first, [&](const size_t li, const long long t0, const dim3 grid) {
            const int kind = SMP_KINDS[li % 4];
            q.tasks = d_ctasks + t0;
            q.step = (int)(li / 4);
            if (kind >= 0) qk_smp_gemm_kernel<<<grid, dim3(512), 0, c->stream>>>(q, kind);
            else if (kind == SMP_ROT) qk_smp_rotate_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(q);
            else qk_smp_draw_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(q);
          });
        },
        [&](const ChainBatch& b) {  // the device wrote the bad column: back to the host behind the launches
          h_bad.resize(b.nc);
          HIP_TRY_AS(what, hipMemcpyAsync(h_bad.data(), q.bad, b.nc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
          return (int)QK_OK;
        },
        [&](const ChainBatch& b) {
          for (size_t e = 0; e < b.nc; ++e)
            if (h_bad[e])
              return qk_fail(QK_EDEVICE, "%s: state %d has a shot whose outcome probabilities sum to 0 or are not finite (a state of norm 0?)", what, s0 + ch.cent[b.c0 + e]);
          return (int)QK_OK;
        });
    if (rc) return rc;
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  }
  HIP_TRY_AS(what, hipMemcpy(bits, dbits.get(), n_rows * n, hipMemcpyDeviceToHost));
  if (logp) HIP_TRY_AS(what, hipMemcpy(logp, dlogp.get(), n_rows * sizeof(double), hipMemcpyDeviceToHost));
  return QK_OK;
}

// ---- amplitudes of given strings (qk_amplitudes_host) -------------------------------------------------------------------------------
// The sampler's chain without the draw: the outcome of every site is given.  One string b in the bases c, v = [1], E = 0, for
// k = 0 .. n-1:
//     W_t[b']  = sum_b v[b] A_k[b][t][b']                                   t = 0, 1
//     W'       = smp_rotate(c[k], W)                                        (the sampler's rotation)
//     u        = W'_{b[k]} over the true bond, zero beyond it
//     m        = max_a max(|Re u[a]|, |Im u[a]|);   m > 0: m = f 2^e, 0.5 <= f < 1 (frexp), v = u 2^-e (exact), E += e
//                                                   m == 0: v = 0, E = 0 (the amplitude is zero whatever follows)
// <b| U_c |psi> = v_n[0] 2^E, returned as (Re, Im) of v_n[0] and E.  The rescale is a power of two and a maximum does not depend on
// the order it is taken in, so it costs no bits and amplitudes far below the smallest double survive.  An amplitude chain is one
// (state, tile of AMP_TILE strings) with a slot of its own (qk_local_plan.h); at site k every chain of the chain batch goes through
// ONE launch of AMP_W (GEMM, string rows as M, K = the true left bond in the ring GEMM's fixed order) and ONE of AMP_PICK (one wave
// per row): 2 n_sites + 1 launches per chain batch with the init kernel, whatever the number of strings.  Nothing of a row depends
// on another row, no atomics, no grid barrier, no spin wait: mantissa and exponent of a (state, string) are the same bits whatever
// the other states and strings, their order, a shared or a per-state table, the cut into batches (QK_AMP_BATCH caps the chains of
// one) and the run.
struct AmpArgs {
  LocArgs e;              // the set and the state batch (the environment pass only when <psi|psi> is asked for)
  const int32_t* cent;    // chain -> batch entry
  const int32_t* str0;    // chain -> its first string
  const int32_t* rows;    // chain -> its strings
  const int64_t* cbase;   // chain -> first double of its slot
  const uint8_t* bits;    // [n_strings][n_sites], or [n_states][n_strings][n_sites] with per_state
  const uint8_t* bases;   // [n_strings][n_sites], NULL: all Z
  const int2* tasks;      // this launch: (chain, block)
  double* slots;
  double* mant;           // [n_states][n_strings][2]
  int32_t* expo;          // [n_states][n_strings]
  int n_strings;
  int per_state;
  int step;               // site k
};

// One 64 x 64 output block of one amplitude chain's GEMM at site k: W = V^T A_k.
__global__ __launch_bounds__(512) void qk_amp_gemm_kernel(const AmpArgs g) {
  __shared__ __attribute__((aligned(16))) double lds[LOC_LDS_DOUBLES];
  const int2 t = g.tasks[blockIdx.x];
  const int ch = __builtin_amdgcn_readfirstlane(t.x);
  const int blk = __builtin_amdgcn_readfirstlane(t.y);
  const int i = __builtin_amdgcn_readfirstlane(g.cent[ch]);
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = __builtin_amdgcn_readfirstlane(g.e.states[i]);
  const int l = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k]), r = __builtin_amdgcn_readfirstlane(g.e.dims[st * n1 + k + 1]);
  const long long P = __builtin_amdgcn_readfirstlane(g.e.pmax[i]);
  const int R = smp_rows_pad(__builtin_amdgcn_readfirstlane(g.rows[ch]));
  const long long PR = P * R;
  double* const slot = g.slots + uni64(g.cbase[ch]);
  const double* const Are = slot + amp_V() * PR;
  const double* const Aim = Are + PR;
  const double* const Bre = g.e.data + uni64(g.e.offs[st * n + k]);
  const double* const Bim = Bre + (long long)l * 2 * r;
  double* const Cre = slot + amp_W() * PR;
  double* const Cim = Cre + 2 * PR;
  const int M = R, N = 2 * r, K = __builtin_amdgcn_readfirstlane(g.e.tru[st * n1 + k]);
  const int npm = (M + 63) / 64;
  const int m0 = 64 * (blk % npm), n0 = 64 * (blk / npm);
  zgemm_ring3<false, LOC_KTL, LOC_NSLOT, true, 8, 64, double, 10>(Cre + (long long)m0 * N + n0, Cim + (long long)m0 * N + n0, N, Are + m0, Aim + m0, R, Bre + n0, Bim + n0, N,
                                                                   min(64, M - m0), min(64, N - n0), K, lds);
}

// v = [1] and E = 0 of every string of a chain: V[0][row] = 1, the rest of the first 16 bond rows (pad_0 = 16) and the pad rows 0.
__global__ __launch_bounds__(256) void qk_amp_init_kernel(const AmpArgs g) {
  const int ch = blockIdx.x;
  const int rows = g.rows[ch], R = smp_rows_pad(rows);
  const int i = g.cent[ch];
  const long long PR = (long long)g.e.pmax[i] * R;
  double* const V = g.slots + g.cbase[ch] + amp_V() * PR;
  for (int e = threadIdx.x; e < LOC_CHUNK * R; e += 256) V[e] = (e < rows) ? 1.0 : 0.0, V[PR + e] = 0.0;
  const long long o = (long long)g.e.states[i] * g.n_strings + g.str0[ch];
  for (int e = threadIdx.x; e < rows; e += 256) g.expo[o + e] = 0;
}

// The pick of one 16-row chunk of strings, one wave per row (four rows each): u = W'_{bit} of the row in its basis over the true
// bond -- lane j takes a' = j, j + 64, .. --, the maximum of |Re u|, |Im u| over the lanes (a maximum has no order), its exponent e,
// the next v = u 2^-e into V (K-major; zero from the true bond on, and for a pad row) and E += e; at the last site v[0] and E are
// the result.
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_amp_pick_kernel(const AmpArgs g) {
  const int2 t = g.tasks[blockIdx.x];
  const int ch = t.x, c = t.y;
  const int i = g.cent[ch];
  const int n = g.e.n_sites, n1 = n + 1, k = g.step;
  const long long st = g.e.states[i];
  const int r = g.e.dims[st * n1 + k + 1], rt = g.e.tru[st * n1 + k + 1];
  const int rows = g.rows[ch], R = smp_rows_pad(rows);
  const long long PR = (long long)g.e.pmax[i] * R;
  double* const slot = g.slots + g.cbase[ch];
  const double* const W = slot + amp_W() * PR;
  double* const V = slot + amp_V() * PR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = 0; j < LOC_CHUNK / 4; ++j) {
    const int row = c * LOC_CHUNK + 4 * wave + j;
    const bool valid = row < rows;
    const long long str = g.str0[ch] + row;                  // of a valid row: below n_strings
    const long long o = st * g.n_strings + str;
    const long long brow = (g.per_state ? o : str) * n + k;  // read for a valid row only
    const int code = (valid && g.bases) ? g.bases[str * n + k] : 3;
    const int bit = valid ? g.bits[brow] : 0;
    const double* const Wrow = W + (long long)row * 2 * r;
    double m = 0.0;
    for (int a = lane; valid && a < rt; a += 64) {
      double a0r, a0i, a1r, a1i;
      smp_rotate(code, Wrow[a], Wrow[a + 2 * PR], Wrow[a + r], Wrow[a + r + 2 * PR], a0r, a0i, a1r, a1i);
      m = fmax(m, fmax(fabs(bit ? a1r : a0r), fabs(bit ? a1i : a0i)));
    }
    for (int s = 32; s > 0; s >>= 1) m = fmax(m, __shfl_xor(m, s));
    int e = 0;
    if (m > 0.0 && m < HUGE_VAL) (void)frexp(m, &e);
    for (int a = lane; a < r; a += 64) {
      double vr = 0, vi = 0;
      if (valid && a < rt) {
        double a0r, a0i, a1r, a1i;
        smp_rotate(code, Wrow[a], Wrow[a + 2 * PR], Wrow[a + r], Wrow[a + r + 2 * PR], a0r, a0i, a1r, a1i);
        vr = ldexp(bit ? a1r : a0r, -e), vi = ldexp(bit ? a1i : a0i, -e);
      }
      if (k + 1 < n) V[(long long)a * R + row] = vr, V[(long long)a * R + row + PR] = vi;
      else if (valid && a == 0) g.mant[2 * o] = vr, g.mant[2 * o + 1] = vi;
    }
    if (valid && lane == 0) g.expo[o] = (m == 0.0) ? 0 : g.expo[o] + e;  // a zero amplitude is (0, 0) with E = 0, whatever came before
  }
}

int amplitudes_run(qk_ctx* c, const qk_mps_set* set, const int32_t n_strings, const uint8_t* bits, const int32_t bits_per_state, const uint8_t* bases, double* mant,
                   int32_t* expo, double* logp, double* norms) {
  static const char* what = "qk_amplitudes_host";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!set) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!bits) return qk_fail(QK_EINVAL, "%s: bits is null", what);
  if (!mant) return qk_fail(QK_EINVAL, "%s: mant is null", what);
  if (!expo) return qk_fail(QK_EINVAL, "%s: expo is null", what);
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; amplitudes need an fp64 set", what);
  if (n_strings < 1) return qk_fail(QK_EINVAL, "%s: n_strings must be >= 1 (got %d)", what, n_strings);
  if (bits_per_state != 0 && bits_per_state != 1) return qk_fail(QK_EINVAL, "%s: bits_per_state must be 0 (shared) or 1 (a table per state) (got %d)", what, bits_per_state);
  const int ns = set->n_states, n = set->n_sites;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  const long long row_bytes = (long long)n_strings * n, n_bits = (bits_per_state ? ns : 1) * row_bytes;
  if (const long long bad = amp_bad_bit(bits, n_bits); bad >= 0) {
    if (bits_per_state) return qk_fail(QK_EINVAL, "%s: bits[%lld][%lld][%lld] = %d is not an outcome bit (0 or 1)", what, bad / row_bytes, bad % row_bytes / n, bad % n, bits[bad]);
    return qk_fail(QK_EINVAL, "%s: bits[%lld][%lld] = %d is not an outcome bit (0 or 1)", what, bad / n, bad % n, bits[bad]);
  }
  if (bases)
    if (const long long bad = smp_bad_basis(bases, row_bytes); bad >= 0)
      return qk_fail(QK_EINVAL, "%s: bases[%lld][%lld] = %d is not a basis code (1..3 = X, Y, Z)", what, bad / n, bad % n, bases[bad]);
  long long cap = 0;  // amplitude chains per batch
  if (const int rc = batch_cap(what, "QK_AMP_BATCH", cap)) return rc;
  QkRangeGuard range_("qk:amplitudes");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  // <psi|psi> = L_n[0][0] of the environment pass of the Pauli strings (the bits of qk_local_paulis_host), only when it is asked
  // for; otherwise a state batch is its tables alone (an empty plan)
  const bool want_norm = logp || norms;
  EnvSizes z;
  env_sizes(set->dims_true.data(), ns, n, set->max_pad, LOC_RMUL, want_norm, z);
  const size_t n_rows = (size_t)ns * n_strings;
  QkDevBuf rev, dbits, dbases, dmant, dexpo, dnorm;
  HIP_TRY_AS(what, rev.alloc((size_t)set->bytes));
  HIP_TRY_AS(what, dbits.alloc(al256((size_t)n_bits)));
  HIP_TRY_AS(what, hipMemcpy(dbits.get(), bits, (size_t)n_bits, hipMemcpyHostToDevice));
  if (bases) {
    HIP_TRY_AS(what, dbases.alloc(al256((size_t)row_bytes)));
    HIP_TRY_AS(what, hipMemcpy(dbases.get(), bases, (size_t)row_bytes, hipMemcpyHostToDevice));
  }
  HIP_TRY_AS(what, dmant.alloc(n_rows * 2 * sizeof(double)));
  HIP_TRY_AS(what, dexpo.alloc(al256(n_rows * sizeof(int32_t))));
  if (want_norm) HIP_TRY_AS(what, dnorm.alloc((size_t)ns * sizeof(double)));
  // memory bound of a state batch (its scratch and the slots of its chains): a quarter of what is free; the scratch of a batch
  // takes at most half of that (at least one state per batch), the chains of a batch the rest (at least one)
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const std::vector<int> bstart = batch_cut(z.need, 0, budget / 2);
  const Plan plan = want_norm ? env_plan(n) : Plan{};
  EnvBatch eb;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(z, plan, s0, nb, 0, eb);
    const SmpChains ch = list_amp_chains(z, s0, nb, n_strings, AMP_TILE);
    const std::vector<size_t> cstart = chain_cut(ch.weight, budget - eb.tot, cap);
    const std::vector<ChainCol> cols{{ch.cent.data(), sizeof(int32_t), 1}, {ch.shot0.data(), sizeof(int32_t), 1}, {ch.rows.data(), sizeof(int32_t), 1}};
    if (const int rc = env_run(c, set, what, rev.get<double>(), z, plan, eb, chain_stage_max(cols, ch, cstart, 0))) return rc;
    if (want_norm) qk_str_norms_kernel<<<dim3((nb + 255) / 256), dim3(256), 0, c->stream>>>(eb.g, nb, dnorm.get<double>());
    HIP_TRY_AS(what, hipGetLastError());
    AmpArgs q{};
    q.e = eb.g;
    q.bits = dbits.get<uint8_t>();
    q.bases = bases ? dbases.get<uint8_t>() : nullptr;
    q.mant = dmant.get<double>(), q.expo = dexpo.get<int32_t>();
    q.n_strings = n_strings, q.per_state = bits_per_state;
    const int rc = chain_run(
        c, what, eb.base + eb.used(), cols, ch, cstart, 0,
        [&](size_t c0, size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) { amp_lists(z, s0, ch, c0, nc, tasks, first); },
        [&](const ChainBatch& b) {
          q.cent = reinterpret_cast<const int32_t*>(b.base + b.st.col[0]);
          q.str0 = reinterpret_cast<const int32_t*>(b.base + b.st.col[1]);
          q.rows = reinterpret_cast<const int32_t*>(b.base + b.st.col[2]);
          q.cbase = reinterpret_cast<const int64_t*>(b.base + b.st.col[3]);
          const int2* d_ctasks = reinterpret_cast<const int2*>(b.base + b.st.tasks);
          q.slots = reinterpret_cast<double*>(b.base + b.st.slots);
          qk_amp_init_kernel<<<dim3((unsigned)b.nc), dim3(256), 0, c->stream>>>(q);
          each_launch(b.first, [&](const size_t li, const long long t0, const dim3 grid) {
            q.tasks = d_ctasks + t0;
            q.step = (int)(li / 2);
            if (AMP_KINDS[li % 2] == AMP_W) qk_amp_gemm_kernel<<<grid, dim3(512), 0, c->stream>>>(q);
            else qk_amp_pick_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(q);
          });
        });
    if (rc) return rc;
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  }
  HIP_TRY_AS(what, hipMemcpy(mant, dmant.get(), n_rows * 2 * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY_AS(what, hipMemcpy(expo, dexpo.get(), n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (!want_norm) return QK_OK;
  std::vector<double> h_norm(ns);
  HIP_TRY_AS(what, hipMemcpy(h_norm.data(), dnorm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
  if (norms) std::memcpy(norms, h_norm.data(), (size_t)ns * sizeof(double));
  if (logp)
    for (int s = 0; s < ns; ++s) {
      if (!(h_norm[s] > 0.0) || !std::isfinite(h_norm[s])) return qk_fail(QK_EDEVICE, "%s: state %d has norm 0 (or a norm that is not finite): logp is not defined", what, s);
      const double ln = std::log(h_norm[s]);
      for (int m = 0; m < n_strings; ++m) {
        const size_t o = (size_t)s * n_strings + m;
        logp[o] = amp_logp(mant[2 * o], mant[2 * o + 1], expo[o], ln);
      }
    }
  return QK_OK;
}

// ---- windows of k qubits (qk_window_rdms_host) ------------------------------------------------------------------------------------
// Window (a, w) = the qubits a .. a+w-1, b = a + w, 1 <= w <= min(n, 6), 0 <= a <= n - w; row index s = sum_j s_{a+j} 2^(w-1-j)
// (qubit a is the most significant bit).  Site k = qubit k, physical index 0 = |0>, states not necessarily normalised,
// environments X[ket][bra], L_0 = R_n = 1, L_n[0][0] = <psi|psi>:
//     rho_{a,w}[s][s'] = sum over all other sites of psi(.. s ..) conj(psi(.. s' ..)) / <psi|psi>
//     M^s[alpha][gamma] = (A_a^{s_a} A_{a+1}^{s_{a+1}} .. A_{b-1}^{s_{b-1}})[alpha][gamma]                              chi_a x chi_b
//     rho_{a,w}[s][s'] <psi|psi> = sum_{alpha,alpha',gamma,gamma'} L_a[alpha][alpha'] M^s[alpha][gamma] R_b[gamma][gamma'] conj(M^{s'}[alpha'][gamma'])
// The route (every product is the C = A^T B form of the ring GEMM, nothing is transposed): the product of the sites grows from the
// right, the new site's index most significant, from two seeds,
//     G_0 = 1 (chi_b x chi_b),   Gr_0 = R_b
//     G_{j+1}[beta][(t, sigma, gamma)] = sum_beta' A_c[beta][t][beta'] G_j[beta'][(sigma, gamma)]      c = b-1-j   (same for Gr)
// with the reversed image's site c, [beta'][(t, beta)], as the A operand; the rows (t, beta) of C are written with ldc = twice the
// stacked width at column offset t times the stacked width, so the next step reads its B operand as it lies.  G_1 is the site b-1
// itself and costs nothing.  Then
//     H[alpha'][(s, gamma)] = sum_alpha L_a[alpha][alpha'] G_w[alpha][(s, gamma)]
//     rho[s][s'] <psi|psi>  = sum_{alpha, gamma'} Gr_w[alpha][(s, gamma')] conj(H[alpha][(s', gamma')])          (L_a is Hermitian)
// About 5 2^w chi^3 complex multiply-adds per window in the GEMMs and 4^w chi^2 / 2 in the closing sum.  Per state batch the
// environment pass of the Pauli strings (every L_k and R_k kept, the norms the bits of qk_local_paulis_host), then its chains -- one
// per (state, window) -- in chain batches: per step j ONE GEMM launch for every chain of the batch (a task's block number also names
// the seed and t), one for H, one closing launch over (chain, 16-row chunk of alpha) that forms every s <= s' in a fixed order, and
// one kernel that adds the chunks in a fixed order, divides by L_n[0][0], mirrors the conjugate and writes rho: exactly Hermitian,
// the diagonal's imaginary part exactly 0.0.  Pad rows and columns are zeros that the GEMMs themselves made.  Nothing of a chain
// depends on another chain, no atomics, no grid barrier, no spin wait: a (state, window) value is the same bits whatever the other
// states, the other windows, the cut into batches (QK_WINDOW_BATCH caps the chains of one) and the run.
struct WinArgs {
  LocArgs e;              // the set and the state batch of the environment pass
  const int32_t* cent;    // chain -> batch entry
  const int32_t* cwin;    // chain -> window (index into starts)
  const int64_t* cbase;   // chain -> first double of its slot
  const int32_t* starts;  // [n_windows]
  const int2* tasks;      // this launch: (chain, block)
  double* slots;
  double* part;           // closing partial sums [chain][max chunks][win_vals(width)]
  int width, n_windows;
  int step;               // step j of WIN_G
};

// One 64 x 64 output block of one window chain's GEMM: a product of step j (WIN_G) or H (WIN_H).
__global__ __launch_bounds__(512) void qk_win_gemm_kernel(const WinArgs g, const int kind) {
  __shared__ __attribute__((aligned(16))) double lds[LOC_LDS_DOUBLES];
  const int2 tk = g.tasks[blockIdx.x];
  const int ch = __builtin_amdgcn_readfirstlane(tk.x);
  int blk = __builtin_amdgcn_readfirstlane(tk.y);
  const int i = __builtin_amdgcn_readfirstlane(g.cent[ch]);
  const int w = g.width, a = __builtin_amdgcn_readfirstlane(g.starts[__builtin_amdgcn_readfirstlane(g.cwin[ch])]), b = a + w;
  const int n = g.e.n_sites, n1 = n + 1;
  const long long st = __builtin_amdgcn_readfirstlane(g.e.states[i]);
  const int* pd = g.e.dims + st * n1;
  const int* td = g.e.tru + st * n1;
  const long long P = __builtin_amdgcn_readfirstlane(g.e.pmax[i]), P2 = P * P, U = win_unit(P, w);
  double* const slot = g.slots + uni64(g.cbase[ch]);
  const double* const env = g.e.scratch + uni64(g.e.sbase[i]) + g.e.rmul * P2;
  const int pb = __builtin_amdgcn_readfirstlane(pd[b]);
  const double *Are, *Aim, *Bre, *Bim;
  double *Cre, *Cim;
  int lda, ldb, ldc, M, N, K;
  if (kind == WIN_G) {
    const int j = g.step, c = b - 1 - j;
    const int pc = __builtin_amdgcn_readfirstlane(pd[c]), pc1 = __builtin_amdgcn_readfirstlane(pd[c + 1]);
    M = pc, N = pb << j, K = __builtin_amdgcn_readfirstlane(td[c + 1]);
    const int per = ((M + 63) / 64) * ((N + 63) / 64);
    const int q = blk / per, seed = q >> 1, t = q & 1;  // seed 0 = Gr, 1 = G
    blk -= q * per;
    Are = g.e.rev + uni64(g.e.offs[st * n + c]) + t * pc, Aim = Are + (long long)pc1 * 2 * pc, lda = 2 * pc;
    if (seed == 0 && j == 0) {  // Gr_0 = R_b
      Bre = env + uni64(g.e.roff[(long long)i * n1 + b]), Bim = Bre + (long long)pb * pb, ldb = pb;
    } else if (seed == 1 && j == 1) {  // G_1 = the site b-1
      Bre = g.e.data + uni64(g.e.offs[st * n + b - 1]), Bim = Bre + (long long)pc1 * 2 * pb, ldb = 2 * pb;
    } else {
      Bre = slot + (seed ? win_G(j) : win_Gr(j)) * U, Bim = Bre + U, ldb = N;
    }
    Cre = slot + (seed ? win_G(j + 1) : win_Gr(j + 1)) * U + (long long)t * N, Cim = Cre + U, ldc = 2 * N;
  } else {  // WIN_H
    const int pa = __builtin_amdgcn_readfirstlane(pd[a]);
    M = pa, N = pb << w, K = __builtin_amdgcn_readfirstlane(td[a]);
    Are = env + uni64(g.e.loff[(long long)i * n1 + a]), Aim = Are + (long long)pa * pa, lda = pa;
    if (w == 1) {  // G_1 = the site a
      Bre = g.e.data + uni64(g.e.offs[st * n + a]), Bim = Bre + (long long)pa * 2 * pb, ldb = 2 * pb;
    } else {
      Bre = slot + win_G(w) * U, Bim = Bre + U, ldb = N;
    }
    Cre = slot + win_H(w) * U, Cim = Cre + U, ldc = N;
  }
  const int npm = (M + 63) / 64;
  const int m0 = 64 * (blk % npm), n0 = 64 * (blk / npm);
  zgemm_ring3<false, LOC_KTL, LOC_NSLOT, true, 8, 64, double, 11>(Cre + (long long)m0 * ldc + n0, Cim + (long long)m0 * ldc + n0, ldc, Are + m0, Aim + m0, lda,
                                                                   Bre + n0, Bim + n0, ldb, min(64, M - m0), min(64, N - n0), K, lds);
}

// The closing sums of one 16-row chunk of alpha, unnormalised: for every s <= s'
//     part[(chain, chunk)][2 p], [2 p + 1] = (Re, Im) sum_{alpha in chunk, gamma'} Gr_w[alpha][(s, gamma')] conj(H[alpha][(s', gamma')]),   p = win_pair(s, s')
// The workgroup takes WIN_CLOSE_GROUP = 16 pairs at a time, 16 lanes per pair: lane l adds the columns gamma' = l, l + 16, .. of
// the chunk's rows in ascending (row, column) order (16 consecutive doubles per pair and row: whole 128-byte lines), then one
// thread per (pair, Re | Im) adds the 16 lane sums in ascending order -- a fixed order, on the vector ALU.
// LDS: red[2][16][17] doubles (4.3 KiB; the pad column keeps the 16 lanes of the final sums on different banks).
__global__ __launch_bounds__(LOC_RED_THREADS) void qk_win_close_kernel(const WinArgs g) {
  __shared__ double red[2][WIN_CLOSE_GROUP][17];
  static_assert(WIN_CLOSE_GROUP * 16 == LOC_RED_THREADS, "16 lanes per pair of a group");
  const int2 tk = g.tasks[blockIdx.x];
  const int ch = tk.x, c = tk.y;
  const int i = g.cent[ch];
  const int w = g.width, a = g.starts[g.cwin[ch]], b = a + w;
  const int n1 = g.e.n_sites + 1;
  const long long st = g.e.states[i];
  const int pb = g.e.dims[st * n1 + b];
  const long long P = g.e.pmax[i], U = win_unit(P, w), ld = (long long)pb << w;
  const double* const Gr = g.slots + g.cbase[ch] + win_Gr(w) * U + (long long)c * LOC_CHUNK * ld;
  const double* const H = g.slots + g.cbase[ch] + win_H(w) * U + (long long)c * LOC_CHUNK * ld;
  double* const out = g.part + ((long long)ch * g.e.max_chunks + c) * win_vals(w);
  const int np = win_pairs(w), lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
  for (int p0 = 0; p0 < np; p0 += WIN_CLOSE_GROUP) {
    double re = 0, im = 0;
    if (p0 + slot < np) {
      int s, sp;
      win_pair_of(p0 + slot, w, s, sp);
      const double* const gs = Gr + (long long)s * pb;
      const double* const hs = H + (long long)sp * pb;
      for (int r = 0; r < LOC_CHUNK; ++r)
        for (int col = lane; col < pb; col += 16) {
          const long long q = r * ld + col;
          const double gr = gs[q], gi = gs[q + U], hr = hs[q], hi = hs[q + U];
          re += gr * hr + gi * hi;
          im += gi * hr - gr * hi;
        }
    }
    red[0][slot][lane] = re, red[1][slot][lane] = im;
    __syncthreads();
    if (threadIdx.x < 2 * WIN_CLOSE_GROUP) {
      const int pp = threadIdx.x >> 1, comp = threadIdx.x & 1;
      double v = 0;
      for (int l = 0; l < 16; ++l) v += red[comp][pp][l];
      if (p0 + pp < np) out[2 * (p0 + pp) + comp] = v;
    }
    __syncthreads();
  }
}

// rho of a chain batch: the chunk sums of each (chain, s <= s') in ascending order, divided by L_n[0][0]; the entry and its mirror
// image, the conjugate; the imaginary part of a diagonal entry is written as exactly 0.0.
__global__ __launch_bounds__(256) void qk_win_rho_kernel(const WinArgs g, const long long nc, double* rho) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const int w = g.width, np = win_pairs(w), D = win_dim(w);
  if (id >= nc * np) return;
  const int ch = (int)(id / np), p = (int)(id % np);
  const int i = g.cent[ch], m = g.cwin[ch];
  const long long st = g.e.states[i];
  const int chunks = g.e.dims[st * (g.e.n_sites + 1) + g.starts[m]] / LOC_CHUNK;
  const double nrm = g.e.scratch[g.e.sbase[i]];  // L_n[0][0]
  const double* q = g.part + (long long)ch * g.e.max_chunks * win_vals(w) + 2 * p;
  double re = 0, im = 0;
  for (int c = 0; c < chunks; ++c) re += q[(long long)c * win_vals(w)], im += q[(long long)c * win_vals(w) + 1];
  int s, sp;
  win_pair_of(p, w, s, sp);
  double* const R = rho + (st * g.n_windows + m) * 2ll * D * D;
  R[2 * (s * D + sp)] = re / nrm;
  R[2 * (s * D + sp) + 1] = (s == sp) ? 0.0 : im / nrm;
  if (s != sp) R[2 * (sp * D + s)] = re / nrm, R[2 * (sp * D + s) + 1] = -(im / nrm);
}

int window_rdms(qk_ctx* c, const qk_mps_set* set, const int32_t width, const int32_t n_starts, const int32_t* starts_in, double* rho, double* norms) {
  static const char* what = "qk_window_rdms_host";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!set) return qk_fail(QK_EINVAL, "%s: set is null", what);
  if (!rho) return qk_fail(QK_EINVAL, "%s: rho is null", what);
  if (set->ctx != c) return qk_fail(QK_EINVAL, "%s: set belongs to another context", what);
  if (set->precision != 64) return qk_fail(QK_EINVAL, "%s: set is complex64; window RDMs need an fp64 set", what);
  const int ns = set->n_states, n = set->n_sites, w = width;
  if (n < 1 || ns < 1) return qk_fail(QK_EINVAL, "%s: set is empty", what);
  if (win_bad_width(w, n)) return qk_fail(QK_EINVAL, "%s: width must be in 1 .. min(n_sites, %d) = %d (got %d)", what, WIN_MAX_WIDTH, std::min(n, WIN_MAX_WIDTH), w);
  std::vector<int32_t> starts;
  if (starts_in) {
    if (n_starts < 1) return qk_fail(QK_EINVAL, "%s: n_starts must be >= 1 when starts are given (got %d)", what, n_starts);
    starts.assign(starts_in, starts_in + n_starts);
    if (const int bad = win_bad_start(n_starts, starts_in, n, w); bad >= 0)
      return qk_fail(QK_EINVAL, "%s: starts[%d] = %d: starts must be strictly increasing in 0 .. n_sites - width = %d", what, bad, starts_in[bad], n - w);
  } else {
    for (int a = 0; a + w <= n; ++a) starts.push_back(a);
  }
  const int nw = (int)starts.size();
  long long cap = 0;  // window chains per batch
  if (const int rc = batch_cap(what, "QK_WINDOW_BATCH", cap)) return rc;
  QkRangeGuard range_("qk:window_rdms");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  EnvSizes z;
  env_sizes(set->dims_true.data(), ns, n, set->max_pad, LOC_RMUL, true, z);
  const int max_chunks = z.max_chunks, nvals = win_vals(w);
  const size_t n_out = (size_t)ns * nw * 2 * win_dim(w) * win_dim(w);
  QkDevBuf rev, dout, dnorm, dstarts;
  HIP_TRY_AS(what, rev.alloc((size_t)set->bytes));
  HIP_TRY_AS(what, dout.alloc(n_out * sizeof(double)));
  HIP_TRY_AS(what, dnorm.alloc((size_t)ns * sizeof(double)));
  HIP_TRY_AS(what, dstarts.alloc(al256((size_t)nw * sizeof(int32_t))));
  HIP_TRY_AS(what, hipMemcpy(dstarts.get<char>(), starts.data(), (size_t)nw * sizeof(int32_t), hipMemcpyHostToDevice));
  // memory bound of a state batch (environments and the slots of its live chains): a quarter of what is free; the environments
  // of a batch take at most half of that (at least one state per batch), the chains of a batch the rest (at least one chain)
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const std::vector<int> bstart = batch_cut(z.need, 0, budget / 2);
  const Plan plan = env_plan(n), wplan = win_plan(w);
  EnvBatch eb;
  for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
    const int s0 = bstart[bi], nb = bstart[bi + 1] - s0;
    env_tables(z, plan, s0, nb, 0, eb);
    const WinChains ch = list_win_chains(z, s0, nb, w, nw, starts.data());
    const std::vector<size_t> cstart = chain_cut(ch.weight, budget - eb.tot, cap);
    const std::vector<ChainCol> cols{{ch.cent.data(), sizeof(int32_t), 1}, {ch.cwin.data(), sizeof(int32_t), 1}};
    const long long width = (long long)max_chunks * nvals;  // of a chain's partial sums
    if (const int rc = env_run(c, set, what, rev.get<double>(), z, plan, eb, chain_stage_max(cols, ch, cstart, width))) return rc;
    qk_str_norms_kernel<<<dim3((nb + 255) / 256), dim3(256), 0, c->stream>>>(eb.g, nb, dnorm.get<double>());
    HIP_TRY_AS(what, hipGetLastError());
    WinArgs q{};
    q.e = eb.g;
    q.starts = dstarts.get<int32_t>();
    q.width = w, q.n_windows = nw;
    const int rc = chain_run(
        c, what, eb.base + eb.used(), cols, ch, cstart, width,
        [&](size_t c0, size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) { win_lists(z, s0, ch, c0, nc, w, starts.data(), tasks, first); },
        [&](const ChainBatch& b) {
          q.cent = reinterpret_cast<const int32_t*>(b.base + b.st.col[0]);
          q.cwin = reinterpret_cast<const int32_t*>(b.base + b.st.col[1]);
          q.cbase = reinterpret_cast<const int64_t*>(b.base + b.st.col[2]);
          const int2* d_ctasks = reinterpret_cast<const int2*>(b.base + b.st.tasks);
          q.part = reinterpret_cast<double*>(b.base + b.st.part);
          q.slots = reinterpret_cast<double*>(b.base + b.st.slots);
          each_launch(b.first, [&](const size_t li, const long long t0, const dim3 grid) {
            const int kind = wplan[li].first;
            q.tasks = d_ctasks + t0;
            q.step = wplan[li].second;
            if (kind >= 0) qk_win_gemm_kernel<<<grid, dim3(512), 0, c->stream>>>(q, kind);
            else qk_win_close_kernel<<<grid, dim3(LOC_RED_THREADS), 0, c->stream>>>(q);
          });
          const long long nv = (long long)b.nc * win_pairs(w);
          qk_win_rho_kernel<<<dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, c->stream>>>(q, (long long)b.nc, dout.get<double>());
        });
    if (rc) return rc;
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  }
  std::vector<double> h_norm((size_t)ns);
  HIP_TRY_AS(what, hipMemcpy(h_norm.data(), dnorm.get(), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
  for (int s = 0; s < ns; ++s)
    if (!(h_norm[s] > 0.0) || !std::isfinite(h_norm[s])) return qk_fail(QK_EDEVICE, "%s: state %d has norm 0 (or a norm that is not finite): its reduced density matrices are undefined", what, s);
  HIP_TRY_AS(what, hipMemcpy(rho, dout.get(), n_out * sizeof(double), hipMemcpyDeviceToHost));
  if (norms) std::memcpy(norms, h_norm.data(), (size_t)ns * sizeof(double));
  return QK_OK;
}

// ---- block overlaps from measurement shots (qk_shot_block_sums_host) -----------------------------------------------------------------
// The randomised-measurement overlap (Elben et al., PRL 124, 010504 (2020)) of outcome tables bits[state][u M + a][site], U settings
// of M shots: all integer arithmetic, definitions in include/qkgram.h, host side in qk_local_plan.h (sbk_*).
//   qk_sbk_pack_kernel  one lane per (state, shot): the block's bytes into one word (sbk_pack); a byte that is neither 0 nor 1 raises *bad.
//   qk_sbk_sums_kernel  one workgroup (four waves) per task = (pair, chunk of settings).  The y words of the chunk are staged in
//       LDS, a row per setting.  Inside a setting a wave takes (block of 64 x words, piece of the y row) units: each lane keeps its
//       x word in a register and every lane reads the same y words (ds_read_b128 of one address: a broadcast, conflict-free).
//       Per (a, b, width): one bit operation for the agreeing bits, v_bcnt (which adds the exponent bias), two more for the high word
//       of the term as a double (sbk_agree_hi) and one v_add_f64 -- exact, because a lane's partial sum is moved into its int64
//       total before 2^20 terms of at most 2^32 have gone into it.  Accumulating int64 terms instead (a 64-bit shift, a select and
//       a two-instruction add) measured 1.44 times slower on the MI355X at M = 64 and four widths, with the same sums.  At the end of a
//       setting the lane totals are added across the wave (shuffles), the four wave sums meet in LDS, and after the chunk one
//       thread per (setting, width) adds them and writes S_u, less M 2^w for a self pair.
//   qk_sbk_total_kernel one thread per (width, pair): the sum of its S_u over the settings.
// Integer sums are exact and order-free; nothing is atomic, no workgroup waits for another.
constexpr int SBK_THREADS = 256, SBK_WAVES = SBK_THREADS / 64;
struct SbkArgs {
  const uint32_t* xw;    // packed words [nx][U M]
  const uint32_t* yw;    // [ny][U M]; the x words when Y is X
  const int32_t* pairs;  // the batch's pairs (x index, y index)
  long long* S;          // per-setting sums of the batch [n_widths][nb][U]
  uint32_t mask[SBK_GROUP];  // of this launch's widths
  int32_t width[SBK_GROUP];
  int w0;                // index of the launch's first width in the call's list
  int self;              // Y is X: a pair (i, i) is a self pair
  int U, M, chunk;
  long long nb, task0;   // pairs of the batch; first task of the launch
};

__global__ __launch_bounds__(256) void qk_sbk_pack_kernel(const uint8_t* bits, const long long count, const int n, const int side, uint32_t* words, int32_t* bad) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  bool b = false;
  words[e] = sbk_pack(bits + e * n, n, side, b);
  if (b) *bad = 1;
}

template <int NW>
__global__ __launch_bounds__(SBK_THREADS) void qk_sbk_sums_kernel(const SbkArgs g) {
  __shared__ __attribute__((aligned(16))) uint32_t ys[SBK_STAGE_WORDS];
  __shared__ long long red[SBK_MAX_CHUNK][SBK_WAVES][NW];
  long long pair;
  int u0, u1;
  sbk_task(g.task0 + blockIdx.x, g.U, g.chunk, pair, u0, u1);
  const int M = g.M, nset = u1 - u0;
  const long long UM = (long long)g.U * M;
  const int xi = g.pairs[2 * pair], yj = g.pairs[2 * pair + 1];
  const uint32_t* const X = g.xw + xi * UM;
  const uint32_t* const Y = g.yw + yj * UM;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = min(M, SBK_STAGE_WORDS), ldr = sbk_round4(row);  // staged words of a setting at a time (nset == 1 when M is longer)
  const int parts = sbk_parts(M), units = sbk_a_blocks(M) * parts;
  long long tot[NW];
  double acc[NW];
  int since = 0;  // terms in acc since it was last moved into tot (the same for every lane of the wave)
  for (int b0 = 0; b0 < M; b0 += SBK_STAGE_WORDS) {
    const int bn = min(SBK_STAGE_WORDS, M - b0);
    __syncthreads();
    for (int e = threadIdx.x; e < nset * bn; e += SBK_THREADS) ys[(e / bn) * ldr + e % bn] = Y[(long long)(u0 + e / bn) * M + b0 + e % bn];
    __syncthreads();
    for (int s = 0; s < nset; ++s) {
      if (b0 == 0) {
#pragma unroll
        for (int v = 0; v < NW; ++v) tot[v] = 0, acc[v] = 0.0;
      }
      const uint32_t* const yr = ys + s * ldr;
      for (int unit = wv; unit < units; unit += SBK_WAVES) {
        const int a = (unit / parts) * 64 + lane, pc = unit % parts;
        const int lo = sbk_part_lo(pc, parts, bn), hi = sbk_part_lo(pc + 1, parts, bn);
        if (since + SBK_STAGE_WORDS > (1 << 20)) {
#pragma unroll
          for (int v = 0; v < NW; ++v) tot[v] += (long long)acc[v], acc[v] = 0.0;
          since = 0;
        }
        since += hi - lo;
        if (a < M) {
          const uint32_t x = X[(long long)(u0 + s) * M + a];
          auto add = [&](const uint32_t y) {
            const uint32_t same = ~(x ^ y);
#pragma unroll
            for (int v = 0; v < NW; ++v) acc[v] += __hiloint2double((int)sbk_agree_hi(__popc(same & g.mask[v]) + 1023u), 0);
          };
          int b = lo;
          for (; b + 4 <= hi; b += 4) {
            const uint4 y4 = *reinterpret_cast<const uint4*>(yr + b);
            add(y4.x), add(y4.y), add(y4.z), add(y4.w);
          }
          for (; b < hi; ++b) add(yr[b]);
        }
      }
      if (b0 + bn == M) {  // the setting is complete: lane totals -> wave sum
#pragma unroll
        for (int v = 0; v < NW; ++v) {
          long long t = tot[v] + (long long)acc[v];
          for (int h = 32; h > 0; h >>= 1) t += __shfl_xor(t, h, 64);
          if (lane == 0) red[s][wv][v] = sbk_agree_sign(g.width[v]) * t;
        }
        since = 0;
      }
    }
  }
  __syncthreads();
  const bool self_pair = g.self && xi == yj;
  for (int e = threadIdx.x; e < nset * NW; e += SBK_THREADS) {
    const int s = e / NW, v = e % NW;
    long long t = 0;
    for (int k = 0; k < SBK_WAVES; ++k) t += red[s][k][v];
    if (self_pair) t -= (long long)M << g.width[v];
    g.S[((long long)(g.w0 + v) * g.nb + pair) * g.U + u0 + s] = t;
  }
}

__global__ __launch_bounds__(256) void qk_sbk_total_kernel(const long long* S, const int nw, const long long nb, const int U, const long long pair0, const long long n_pairs,
                                                           long long* sums) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nw * nb) return;
  const long long v = e / nb, p = e % nb;
  const long long* s = S + e * U;
  long long t = 0;
  for (int u = 0; u < U; ++u) t += s[u];
  sums[v * n_pairs + pair0 + p] = t;
}

template <int NW>
void sbk_launch(const SbkArgs& q, const unsigned grid, hipStream_t stream) {
  qk_sbk_sums_kernel<NW><<<dim3(grid), dim3(SBK_THREADS), 0, stream>>>(q);
}

// the packed words of one outcome table, uploaded in pieces of whole states that fit `room` bytes (at least one state)
int sbk_pack_table(qk_ctx* c, const char* what, const char* name, const uint8_t* bits, const int ns, const long long UM, const int n, const int side, const long long room,
                   uint32_t* words, int32_t* d_bad) {
  const long long per_state = UM * n, piece = std::max(1ll, std::min((long long)ns, room / per_state));
  QkDevBuf stage;
  HIP_TRY_AS(what, stage.alloc((size_t)(piece * per_state)));
  for (long long s0 = 0; s0 < ns; s0 += piece) {
    const long long cnt = std::min(piece, ns - s0) * UM;
    HIP_TRY_AS(what, hipMemcpyAsync(stage.get(), bits + s0 * per_state, (size_t)(cnt * n), hipMemcpyHostToDevice, c->stream));
    qk_sbk_pack_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, c->stream>>>(stage.get<uint8_t>(), cnt, n, side, words + s0 * UM, d_bad);
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the stage is reused by the next piece
  }
  int32_t bad = 0;
  HIP_TRY_AS(what, hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
  if (bad) return qk_fail(QK_EINVAL, "%s: %s holds a bit other than 0 or 1 among the block's qubits", what, name);
  return QK_OK;
}

int shot_block_sums(qk_ctx* c, const int32_t n, const int32_t U, const int32_t M, const int32_t nx, const uint8_t* bits_x, const int32_t ny, const uint8_t* bits_y,
                    const int64_t n_pairs, const int32_t* pairs, const int32_t side, const int32_t nw, const int32_t* widths, int64_t* sums, int64_t* per_setting) {
  static const char* what = "qk_shot_block_sums_host";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!bits_x) return qk_fail(QK_EINVAL, "%s: bits_x is null", what);
  if (!pairs) return qk_fail(QK_EINVAL, "%s: pairs is null", what);
  if (!widths) return qk_fail(QK_EINVAL, "%s: widths is null", what);
  if (!sums) return qk_fail(QK_EINVAL, "%s: sums is null", what);
  if (n < 1) return qk_fail(QK_EINVAL, "%s: n_sites must be >= 1 (got %d)", what, n);
  if (U < 1) return qk_fail(QK_EINVAL, "%s: n_settings must be >= 1 (got %d)", what, U);
  if (M < 1) return qk_fail(QK_EINVAL, "%s: shots_per_setting must be >= 1 (got %d)", what, M);
  if (nx < 1) return qk_fail(QK_EINVAL, "%s: nx must be >= 1 (got %d)", what, nx);
  if (ny < 1) return qk_fail(QK_EINVAL, "%s: ny must be >= 1 (got %d)", what, ny);
  if (!bits_y && ny != nx) return qk_fail(QK_EINVAL, "%s: Y is X (bits_y is null) but ny %d != nx %d", what, ny, nx);
  if (n_pairs < 1) return qk_fail(QK_EINVAL, "%s: n_pairs must be >= 1 (got %lld)", what, (long long)n_pairs);
  if (side != 0 && side != 1) return qk_fail(QK_EINVAL, "%s: side must be 0 (left) or 1 (right) (got %d)", what, side);
  if (nw < 1) return qk_fail(QK_EINVAL, "%s: n_widths must be >= 1 (got %d)", what, nw);
  if (const int bad = sbk_bad_width(nw, widths, n); bad >= 0)
    return qk_fail(QK_EINVAL, "%s: widths[%d] = %d: widths must be strictly increasing in 1 .. min(n_sites, 32) = %d", what, bad, widths[bad], std::min(n, SBK_MAX_WIDTH));
  if (!sbk_fits(U, M, widths[nw - 1]))
    return qk_fail(QK_EINVAL, "%s: n_settings %d x shots_per_setting %d ^2 x 2^%d (the largest of widths) exceeds 2^62: the sums would not fit an int64", what, U, M,
                   widths[nw - 1]);
  const bool self = !bits_y;
  for (long long e = 0; e < n_pairs; ++e) {
    const int i = pairs[2 * e], j = pairs[2 * e + 1];
    if (i < 0 || i >= nx || j < 0 || j >= ny) return qk_fail(QK_EINVAL, "%s: pairs[%lld] is (%d, %d), the tables hold %d x %d states", what, e, i, j, nx, ny);
    if (self && i == j && M < 2) return qk_fail(QK_EINVAL, "%s: pairs[%lld] is the self pair (%d, %d): it needs shots_per_setting >= 2", what, e, i, j);
  }
  QkRangeGuard range_("qk:shot_block_sums");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  const long long UM = (long long)U * M;
  QkDevBuf words, dsums, dbad;
  HIP_TRY_AS(what, words.alloc((size_t)((long long)(nx + (self ? 0 : ny)) * UM) * sizeof(uint32_t)));
  HIP_TRY_AS(what, dsums.alloc((size_t)nw * n_pairs * sizeof(int64_t)));
  HIP_TRY_AS(what, dbad.alloc(sizeof(int32_t)));
  HIP_TRY_AS(what, hipMemset(dbad.get(), 0, sizeof(int32_t)));
  // memory bound of the staged outcome bytes and of a pair batch: a quarter of what is free once the words and the sums exist
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const long long room = budget * (long long)sizeof(double);
  uint32_t* const xw = words.get<uint32_t>();
  uint32_t* const yw = self ? xw : xw + (long long)nx * UM;
  if (const int rc = sbk_pack_table(c, what, "bits_x", bits_x, nx, UM, n, side, room, xw, dbad.get<int32_t>())) return rc;
  if (!self)
    if (const int rc = sbk_pack_table(c, what, "bits_y", bits_y, ny, UM, n, side, room, yw, dbad.get<int32_t>())) return rc;

  const int chunk = sbk_chunk(U, M, n_pairs), nchunks = sbk_n_chunks(U, chunk);
  const long long batch = std::min((long long)n_pairs, sbk_batch_pairs(room, nw, U));
  SbkArgs q{};
  q.xw = xw, q.yw = yw, q.self = self, q.U = U, q.M = M, q.chunk = chunk;
  for (long long p0 = 0; p0 < n_pairs; p0 += batch) {
    const long long nb = std::min(batch, n_pairs - p0);
    // one device buffer for the pair batch: [pairs | per-setting sums]
    const size_t b_pairs = al256((size_t)(2 * nb) * sizeof(int32_t)), b_S = (size_t)nw * nb * U * sizeof(int64_t);
    HIP_TRY_AS(what, c->local_scratch.ensure(b_pairs + b_S));
    char* const base = c->local_scratch.get<char>();
    q.pairs = reinterpret_cast<const int32_t*>(base);
    q.S = reinterpret_cast<long long*>(base + b_pairs);
    q.nb = nb;
    HIP_TRY_AS(what, hipMemcpyAsync(base, pairs + 2 * p0, (size_t)(2 * nb) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    for (int at = 0; at < nw; at += sbk_group(nw, at)) {
      const int cnt = sbk_group(nw, at);
      q.w0 = at;
      for (int v = 0; v < cnt; ++v) q.mask[v] = sbk_mask(widths[at + v]), q.width[v] = widths[at + v];
      for (long long t0 = 0; t0 < nb * nchunks; t0 += SBK_LAUNCH_TASKS) {
        q.task0 = t0;
        const unsigned grid = (unsigned)std::min((long long)SBK_LAUNCH_TASKS, nb * nchunks - t0);
        if (cnt == 8) sbk_launch<8>(q, grid, c->stream);
        else if (cnt == 4) sbk_launch<4>(q, grid, c->stream);
        else if (cnt == 2) sbk_launch<2>(q, grid, c->stream);
        else sbk_launch<1>(q, grid, c->stream);
      }
      HIP_TRY_AS(what, hipGetLastError());
    }
    qk_sbk_total_kernel<<<dim3((unsigned)((nw * nb + 255) / 256)), dim3(256), 0, c->stream>>>(q.S, nw, nb, U, p0, n_pairs, dsums.get<long long>());
    HIP_TRY_AS(what, hipGetLastError());
    if (per_setting)
      for (int v = 0; v < nw; ++v)
        HIP_TRY_AS(what, hipMemcpyAsync(per_setting + ((long long)v * n_pairs + p0) * U, q.S + (long long)v * nb * U, (size_t)(nb * U) * sizeof(int64_t), hipMemcpyDeviceToHost,
                                        c->stream));
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the batch's buffer is reused by the next batch
  }
  HIP_TRY_AS(what, hipMemcpy(sums, dsums.get(), (size_t)nw * n_pairs * sizeof(int64_t), hipMemcpyDeviceToHost));
  return QK_OK;
}

// ---- the shadow kernel's shot-pair histograms (qk_shadow_hist_host) -------------------------------------------------------------------
// The classical-shadow kernel of Huang et al. (Science 377, eabk3333 (2022)) needs of a pair of states only the histogram of
// d = (qubits measured in the same basis with the same outcome) - (same basis, other outcome) over all its shot pairs: all integer
// arithmetic, definitions in include/qkgram.h, host side in qk_local_plan.h (shk_*).
//   qk_shk_pack_kernel  one lane per (state, shot): bits and bases into the record of three planes per 32 qubits (shk_pack); a bit
//       that is neither 0 nor 1 raises bad[0], a code outside 1 .. 3 bad[1].
//   qk_shk_hist_kernel  one workgroup per task = (pair, range of blocks of 64 x shots).  The y records are staged in LDS, 256 at a
//       time, rows of 16-byte multiples.  A wave takes (x block, piece of the staged records) units: each lane keeps its x record in
//       registers (3 to 12 words) and every lane reads the same y record (ds_read_b128 of one address: a broadcast, conflict-free).
//       Per shot pair and group: three XORs, an OR, an AND-NOT and an AND, and two v_bcnt that add up over the groups (shk_d); then
//       one increment, ds_add_u32 without a return value, so nothing waits for it.  Where it lands is the layout (shk_layout):
//       private counters [bin][thread] -- the lanes of a wave hit 64 consecutive words, no two lanes ever share one, the LDS does
//       the add in one pass -- or, for few shots, where clearing and adding up 256 copies of the histogram would cost more than the
//       shot pairs themselves, one histogram per wave, the lanes that meet in a bin serialised by the LDS.  At the end of the task
//       the copies of each bin are added into an int64 and written to the task's row.
//   qk_shk_total_kernel one thread per (pair, bin): the sum of the rows of the pair's tasks.
//   qk_shk_equal_kernel one workgroup per pair: the histogram of the shot pairs t = t' alone, one LDS histogram.
// Counts are exact and order-free; no global atomic, no workgroup waits for another.
struct ShkArgs {
  const uint32_t* xr;    // records [nx][shots_x][3 groups]
  const uint32_t* yr;    // [ny][shots_y][3 groups]; the x records when Y is X
  const int32_t* pairs;  // the batch's pairs (x index, y index)
  long long* rows;       // per-task histograms of the batch [nb pair_tasks][bins]
  int n, shots_x, shots_y, task_blocks;
  long long task0;       // first task of the launch
};

__global__ __launch_bounds__(256) void qk_shk_pack_kernel(const uint8_t* bits, const uint8_t* bases, const int per_state, const long long count, const int shots, const int n,
                                                          uint32_t* recs, int32_t* bad) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  bool bad_bit = false, bad_code = false;
  uint32_t rec[3 * SHK_MAX_GROUPS];
  shk_pack(bits + e * n, bases + (per_state ? e : e % shots) * n, n, rec, bad_bit, bad_code);
  const int words = shk_words(n);
  for (int k = 0; k < words; ++k) recs[e * words + k] = rec[k];
  if (bad_bit) bad[0] = 1;
  if (bad_code) bad[1] = 1;
}

template <int G, int LAYOUT>
__global__ __launch_bounds__(256) void qk_shk_hist_kernel(const ShkArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint32_t shk_lds[];
  constexpr int W = 3 * G, LD = shk_stride(G);
  uint32_t* const ys = shk_lds;                        // staged y records, LD words each
  uint32_t* const cnt = shk_lds + SHK_STAGE_SHOTS * LD;  // the counters
  const int threads = blockDim.x, waves = threads >> 6, lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: the loops over a wave's units run on the scalar unit
  const int bins = shk_bins(g.n);
  long long pair;
  int b0, b1;
  shk_task(g.task0 + blockIdx.x, g.shots_x, g.task_blocks, pair, b0, b1);
  const int xi = g.pairs[2 * pair], yj = g.pairs[2 * pair + 1];
  const uint32_t* const X = g.xr + (long long)xi * g.shots_x * W;
  const uint32_t* const Y = g.yr + (long long)yj * g.shots_y * W;
  const int ncnt = LAYOUT == SHK_PRIVATE ? bins * threads : bins * waves;
  for (int e = threadIdx.x; e < ncnt; e += threads) cnt[e] = 0;
  // this lane's counter of d = 0, and the words from one bin to the next
  uint32_t* const mine = LAYOUT == SHK_PRIVATE ? cnt + g.n * threads + threadIdx.x : cnt + wv * bins + g.n;
  const int step = LAYOUT == SHK_PRIVATE ? threads : 1;
  const int parts = shk_parts(b1 - b0, waves), units = (b1 - b0) * parts;
  for (int y0 = 0; y0 < g.shots_y; y0 += SHK_STAGE_SHOTS) {
    const int bn = min(SHK_STAGE_SHOTS, g.shots_y - y0);
    __syncthreads();  // the counters are cleared; the last pass's records are no longer read
    for (int e = threadIdx.x; e < bn * W; e += threads) ys[(e / W) * LD + e % W] = Y[(long long)y0 * W + e];
    __syncthreads();
    for (int unit = wv; unit < units; unit += waves) {
      const long long a = (long long)(b0 + unit / parts) * SHK_BLOCK + lane;  // this lane's x shot
      const int pc = unit % parts;
      const int lo = shk_part_lo(pc, parts, bn), hi = shk_part_lo(pc + 1, parts, bn);
      if (a >= g.shots_x) continue;
      uint32_t x[W];
#pragma unroll
      for (int k = 0; k < W; ++k) x[k] = X[a * W + k];
      // four y records at a time, read before the four increments: the reads of one round are in flight together
      auto count = [&](const uint32_t* y) { __hip_atomic_fetch_add(mine + shk_d(x, y, G) * step, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
      auto fetch = [&](uint32_t* y, const int b) {
#pragma unroll
        for (int k = 0; k < LD; k += 4) {
          const uint4 v = *reinterpret_cast<const uint4*>(ys + b * LD + k);
          y[k] = v.x, y[k + 1] = v.y, y[k + 2] = v.z, y[k + 3] = v.w;
        }
      };
      int b = lo;
      for (; b + 4 <= hi; b += 4) {
        uint32_t y[4][LD];
#pragma unroll
        for (int u = 0; u < 4; ++u) fetch(y[u], b + u);
#pragma unroll
        for (int u = 0; u < 4; ++u) count(y[u]);
      }
      for (; b < hi; ++b) {
        uint32_t y[LD];
        fetch(y, b);
        count(y);
      }
    }
  }
  __syncthreads();
  long long* const row = g.rows + (g.task0 + blockIdx.x) * bins;
  if (LAYOUT == SHK_PRIVATE) {
    for (int bin = wv; bin < bins; bin += waves) {  // a wave per bin: consecutive words, then across the lanes
      long long t = 0;
      for (int k = lane; k < threads; k += 64) t += cnt[bin * threads + k];
      for (int h = 32; h > 0; h >>= 1) t += __shfl_xor(t, h, 64);
      if (lane == 0) row[bin] = t;
    }
  } else {
    for (int bin = threadIdx.x; bin < bins; bin += threads) {
      long long t = 0;
      for (int k = 0; k < waves; ++k) t += cnt[k * bins + bin];
      row[bin] = t;
    }
  }
}

__global__ __launch_bounds__(256) void qk_shk_total_kernel(const long long* rows, const long long nb, const int pair_tasks, const int bins, long long* hist) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nb * bins) return;
  const long long p = e / bins, bin = e % bins;
  long long t = 0;
  for (int k = 0; k < pair_tasks; ++k) t += rows[(p * pair_tasks + k) * bins + bin];
  hist[e] = t;
}

template <int G>
__global__ __launch_bounds__(256) void qk_shk_equal_kernel(const uint32_t* xr, const uint32_t* yr, const int32_t* pairs, const long long pair0, const int n, const int shots,
                                                           long long* equal) {
  __shared__ uint32_t h[shk_bins(SHK_MAX_QUBITS)];
  constexpr int W = 3 * G;
  const long long pair = pair0 + blockIdx.x;
  const int bins = shk_bins(n);
  const uint32_t* const X = xr + (long long)pairs[2 * pair] * shots * W;
  const uint32_t* const Y = yr + (long long)pairs[2 * pair + 1] * shots * W;
  for (int e = threadIdx.x; e < bins; e += 256) h[e] = 0;
  __syncthreads();
  for (int t = threadIdx.x; t < shots; t += 256) {
    uint32_t x[W], y[W];
#pragma unroll
    for (int k = 0; k < W; ++k) x[k] = X[(long long)t * W + k], y[k] = Y[(long long)t * W + k];
    __hip_atomic_fetch_add(h + n + shk_d(x, y, G), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < bins; e += 256) equal[pair * bins + e] = h[e];
}

template <int G, int LAYOUT>
int shk_launch(const ShkArgs& q, const unsigned grid, const int waves, const int lds, hipStream_t stream) {
  if (q.task0 == 0 &&  // once per batch: the private counters may take most of a CU's LDS
      hipFuncSetAttribute(reinterpret_cast<const void*>(qk_shk_hist_kernel<G, LAYOUT>), hipFuncAttributeMaxDynamicSharedMemorySize, SHK_LDS_BYTES) != hipSuccess)
    return 1;
  qk_shk_hist_kernel<G, LAYOUT><<<dim3(grid), dim3(64 * waves), lds, stream>>>(q);
  return 0;
}
template <int G>
int shk_launch_g(const ShkLayout layout, const ShkArgs& q, const unsigned grid, const int waves, const int lds, hipStream_t stream) {
  return layout == SHK_PRIVATE ? shk_launch<G, SHK_PRIVATE>(q, grid, waves, lds, stream) : shk_launch<G, SHK_SHARED>(q, grid, waves, lds, stream);
}

// the records of one outcome table, uploaded in pieces of whole states that fit `room` bytes (at least one state)
int shk_pack_table(qk_ctx* c, const char* what, const char* bits_name, const char* bases_name, const uint8_t* bits, const uint8_t* bases, const int per_state, const int ns,
                   const long long shots, const int n, const long long room, uint32_t* recs, int32_t* d_bad) {
  const long long per = shots * n, piece = std::max(1ll, std::min((long long)ns, room / (per * (per_state ? 2 : 1))));
  QkDevBuf stage, bstage;
  HIP_TRY_AS(what, stage.alloc((size_t)(piece * per)));
  HIP_TRY_AS(what, bstage.alloc((size_t)((per_state ? piece : 1) * per)));
  if (!per_state) HIP_TRY_AS(what, hipMemcpyAsync(bstage.get(), bases, (size_t)per, hipMemcpyHostToDevice, c->stream));
  for (long long s0 = 0; s0 < ns; s0 += piece) {
    const long long cnt = std::min(piece, ns - s0) * shots;
    HIP_TRY_AS(what, hipMemcpyAsync(stage.get(), bits + s0 * per, (size_t)(cnt * n), hipMemcpyHostToDevice, c->stream));
    if (per_state) HIP_TRY_AS(what, hipMemcpyAsync(bstage.get(), bases + s0 * per, (size_t)(cnt * n), hipMemcpyHostToDevice, c->stream));
    qk_shk_pack_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, c->stream>>>(stage.get<uint8_t>(), bstage.get<uint8_t>(), per_state, cnt, (int)shots, n,
                                                                                         recs + s0 * shots * shk_words(n), d_bad);
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the stages are reused by the next piece
  }
  int32_t bad[2] = {0, 0};
  HIP_TRY_AS(what, hipMemcpy(bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
  if (bad[0]) return qk_fail(QK_EINVAL, "%s: %s holds a bit other than 0 or 1", what, bits_name);
  if (bad[1]) return qk_fail(QK_EINVAL, "%s: %s holds a basis code outside 1 .. 3 (1 = X, 2 = Y, 3 = Z)", what, bases_name);
  return QK_OK;
}

int shadow_hist(qk_ctx* c, const int32_t n, const int32_t nx, const int32_t shots_x, const uint8_t* bits_x, const uint8_t* bases_x, const int32_t xps, const int32_t ny,
                const int32_t shots_y, const uint8_t* bits_y, const uint8_t* bases_y, const int32_t yps, const int64_t n_pairs, const int32_t* pairs, int64_t* hist,
                int64_t* equal) {
  static const char* what = "qk_shadow_hist_host";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!bits_x) return qk_fail(QK_EINVAL, "%s: bits_x is null", what);
  if (!bases_x) return qk_fail(QK_EINVAL, "%s: bases_x is null", what);
  if (!pairs) return qk_fail(QK_EINVAL, "%s: pairs is null", what);
  if (!hist) return qk_fail(QK_EINVAL, "%s: hist is null", what);
  if (n < 1) return qk_fail(QK_EINVAL, "%s: n_sites must be >= 1 (got %d)", what, n);
  if (n > SHK_MAX_QUBITS) return qk_fail(QK_EINVAL, "%s: n_sites must be <= %d (got %d)", what, SHK_MAX_QUBITS, n);
  if (nx < 1) return qk_fail(QK_EINVAL, "%s: nx must be >= 1 (got %d)", what, nx);
  if (shots_x < 1) return qk_fail(QK_EINVAL, "%s: shots_x must be >= 1 (got %d)", what, shots_x);
  if (ny < 1) return qk_fail(QK_EINVAL, "%s: ny must be >= 1 (got %d)", what, ny);
  if (shots_y < 1) return qk_fail(QK_EINVAL, "%s: shots_y must be >= 1 (got %d)", what, shots_y);
  if (n_pairs < 1) return qk_fail(QK_EINVAL, "%s: n_pairs must be >= 1 (got %lld)", what, (long long)n_pairs);
  if (xps != 0 && xps != 1) return qk_fail(QK_EINVAL, "%s: bases_x_per_state must be 0 or 1 (got %d)", what, xps);
  if (yps != 0 && yps != 1) return qk_fail(QK_EINVAL, "%s: bases_y_per_state must be 0 or 1 (got %d)", what, yps);
  const bool self = !bits_y;
  if (self && ny != nx) return qk_fail(QK_EINVAL, "%s: Y is X (bits_y is null) but ny %d != nx %d", what, ny, nx);
  if (self && shots_y != shots_x) return qk_fail(QK_EINVAL, "%s: Y is X (bits_y is null) but shots_y %d != shots_x %d", what, shots_y, shots_x);
  if (self && bases_y) return qk_fail(QK_EINVAL, "%s: Y is X (bits_y is null) but bases_y is given", what);
  if (!self && !bases_y) return qk_fail(QK_EINVAL, "%s: bits_y is given but bases_y is null", what);
  if (equal && shots_x != shots_y) return qk_fail(QK_EINVAL, "%s: equal needs shots_x == shots_y (got %d and %d)", what, shots_x, shots_y);
  for (long long e = 0; e < n_pairs; ++e) {
    const int i = pairs[2 * e], j = pairs[2 * e + 1];
    if (i < 0 || i >= nx || j < 0 || j >= ny) return qk_fail(QK_EINVAL, "%s: pairs[%lld] is (%d, %d), the tables hold %d x %d states", what, e, i, j, nx, ny);
  }
  long long cap = 0;  // pairs per batch
  if (const int rc = batch_cap(what, "QK_SHADOW_BATCH", cap)) return rc;
  QkRangeGuard range_("qk:shadow_hist");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  const int groups = shk_groups(n), words = shk_words(n), bins = shk_bins(n);
  const long long nrx = (long long)nx * shots_x, nry = self ? 0 : (long long)ny * shots_y;
  QkDevBuf recs, dbad;
  HIP_TRY_AS(what, recs.alloc((size_t)((nrx + nry) * words) * sizeof(uint32_t)));
  HIP_TRY_AS(what, dbad.alloc(2 * sizeof(int32_t)));
  HIP_TRY_AS(what, hipMemset(dbad.get(), 0, 2 * sizeof(int32_t)));
  // memory bound of the staged outcome bytes and of a pair batch: a quarter of what is free once the records exist
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const long long room = budget * (long long)sizeof(double);
  uint32_t* const xr = recs.get<uint32_t>();
  uint32_t* const yr = self ? xr : xr + nrx * words;
  if (const int rc = shk_pack_table(c, what, "bits_x", "bases_x", bits_x, bases_x, xps, nx, shots_x, n, room, xr, dbad.get<int32_t>())) return rc;
  if (!self)
    if (const int rc = shk_pack_table(c, what, "bits_y", "bases_y", bits_y, bases_y, yps, ny, shots_y, n, room, yr, dbad.get<int32_t>())) return rc;

  const ShkLayout layout = shk_layout(n, shots_x, shots_y);
  const int waves = shk_waves(n, layout), lds = shk_lds_bytes(n, layout);
  const int task_blocks = shk_task_blocks(layout, shots_x, shots_y, n_pairs), pair_tasks = shk_pair_tasks(shots_x, task_blocks);
  long long batch = std::min((long long)n_pairs, shk_batch_pairs(room, n, pair_tasks));
  if (cap) batch = std::min(batch, cap);
  ShkArgs q{};
  q.xr = xr, q.yr = yr, q.n = n, q.shots_x = shots_x, q.shots_y = shots_y, q.task_blocks = task_blocks;
  for (long long p0 = 0; p0 < n_pairs; p0 += batch) {
    const long long nb = std::min(batch, n_pairs - p0), tasks = nb * pair_tasks;
    // one device buffer for the pair batch: [pairs | per-task rows | histograms | equal-shot histograms]
    const size_t b_pairs = al256((size_t)(2 * nb) * sizeof(int32_t)), b_rows = (size_t)tasks * bins * sizeof(int64_t), b_hist = (size_t)nb * bins * sizeof(int64_t);
    HIP_TRY_AS(what, c->local_scratch.ensure(b_pairs + b_rows + 2 * b_hist));
    char* const base = c->local_scratch.get<char>();
    q.pairs = reinterpret_cast<const int32_t*>(base);
    q.rows = reinterpret_cast<long long*>(base + b_pairs);
    long long* const d_hist = reinterpret_cast<long long*>(base + b_pairs + b_rows);
    long long* const d_equal = reinterpret_cast<long long*>(base + b_pairs + b_rows + b_hist);
    HIP_TRY_AS(what, hipMemcpyAsync(base, pairs + 2 * p0, (size_t)(2 * nb) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    for (long long t0 = 0; t0 < tasks; t0 += SHK_LAUNCH_TASKS) {
      q.task0 = t0;
      const unsigned grid = (unsigned)std::min((long long)SHK_LAUNCH_TASKS, tasks - t0);
      const int rc = groups == 1 ? shk_launch_g<1>(layout, q, grid, waves, lds, c->stream)
                   : groups == 2 ? shk_launch_g<2>(layout, q, grid, waves, lds, c->stream)
                   : groups == 3 ? shk_launch_g<3>(layout, q, grid, waves, lds, c->stream)
                                 : shk_launch_g<4>(layout, q, grid, waves, lds, c->stream);
      if (rc) return qk_fail(QK_EDEVICE, "%s: the histogram kernel was refused %d bytes of LDS", what, lds);
    }
    HIP_TRY_AS(what, hipGetLastError());
    qk_shk_total_kernel<<<dim3((unsigned)((nb * bins + 255) / 256)), dim3(256), 0, c->stream>>>(q.rows, nb, pair_tasks, bins, d_hist);
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipMemcpyAsync(hist + p0 * bins, d_hist, b_hist, hipMemcpyDeviceToHost, c->stream));
    if (equal) {
      for (long long e0 = 0; e0 < nb; e0 += 32 * SHK_LAUNCH_TASKS) {
        const unsigned grid = (unsigned)std::min((long long)32 * SHK_LAUNCH_TASKS, nb - e0);
        if (groups == 1) qk_shk_equal_kernel<1><<<dim3(grid), dim3(256), 0, c->stream>>>(xr, yr, q.pairs, e0, n, shots_x, d_equal);
        else if (groups == 2) qk_shk_equal_kernel<2><<<dim3(grid), dim3(256), 0, c->stream>>>(xr, yr, q.pairs, e0, n, shots_x, d_equal);
        else if (groups == 3) qk_shk_equal_kernel<3><<<dim3(grid), dim3(256), 0, c->stream>>>(xr, yr, q.pairs, e0, n, shots_x, d_equal);
        else qk_shk_equal_kernel<4><<<dim3(grid), dim3(256), 0, c->stream>>>(xr, yr, q.pairs, e0, n, shots_x, d_equal);
      }
      HIP_TRY_AS(what, hipGetLastError());
      HIP_TRY_AS(what, hipMemcpyAsync(equal + p0 * bins, d_equal, b_hist, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));  // the batch's buffer is reused by the next batch
  }
  return QK_OK;
}

// ---- Pauli strings estimated from shots (qk_shot_strings_host) -----------------------------------------------------------------------
// For every (state, Pauli string): the number of shots whose bases equal the string on its support, and the sum of their signs.  All
// integer arithmetic on the shadow kernel's shot records; definitions in include/qkgram.h, host side in qk_local_plan.h (sst_*).
//   qk_sst_kernel        one workgroup of four waves per task = (state, block of 64 strings, range of shots).
//       Layout: one string per lane, its record (two planes per group) and its support in registers for the whole task; the shot
//       records staged in LDS, 256 at a time, rows of 16-byte multiples, and read as a broadcast (ds_read_b128 of one address in
//       every lane: conflict-free) -- the shadow kernel's pattern.  It was taken over the other layout (a shot per lane, the strings
//       wave-uniform, the match mask of a wave counted twice on the scalar unit) because a lane's count and sum then stay in two of
//       its own registers for the whole task: no cross-lane step per (string, wave of shots), no scalar instruction per 64 tests --
//       at one group that layout spends about as many scalar instructions as vector ones, and the scalar unit is shared by the
//       waves of a CU -- and a ragged number of shots costs nothing (a ragged number of strings idles lanes of one wave instead).
//       Per (shot, string, group): two XORs, an OR, an AND and an OR into the mismatch word, an AND and an XOR into the parity word
//       (sst_test); per (shot, string) one compare, one v_bcnt and the two conditional adds.  The waves of the workgroup take the
//       staged shots in turn; at the end the four partial (sum, count) of a lane are added through LDS and written to the task's row.
//   qk_sst_total_kernel  one thread per (state, string): the sum of the rows of its tasks, int64.
// Sums and counts are exact and order-free; no global atomic, no workgroup waits for another.
struct SstArgs {
  const uint32_t* recs;  // shot records [n_states][shots][3 groups]
  const uint32_t* strs;  // string records of the batch [blocks * 64][2 groups], zero (identity) beyond the batch's strings
  int32_t* rows;         // per-task rows of the batch [tasks][SST_ROW]
  int shots, blocks, task_chunks;
  long long task0;       // first task of the launch
};

template <int G>
__global__ __launch_bounds__(256) void qk_sst_kernel(const SstArgs g) {
  constexpr int W = 3 * G, LD = shk_stride(G);
  __shared__ __attribute__((aligned(16))) uint32_t ys[SST_STAGE_SHOTS * LD];  // staged shot records, LD words each
  __shared__ int32_t part[4][SST_ROW];                                        // the waves' partial sums and counts
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: the loop over the staged shots runs on the scalar unit
  long long state;
  int block, t0, t1;
  sst_task(g.task0 + blockIdx.x, g.blocks, g.shots, g.task_chunks, state, block, t0, t1);
  const uint32_t* const X = g.recs + state * g.shots * W;
  uint32_t s[2 * G];
#pragma unroll
  for (int k = 0; k < 2 * G; ++k) s[k] = g.strs[((long long)block * SST_BLOCK + lane) * (2 * G) + k];
  int sum = 0, cnt = 0;
  for (int y0 = t0; y0 < t1; y0 += SST_STAGE_SHOTS) {
    const int bn = min(SST_STAGE_SHOTS, t1 - y0);
    __syncthreads();  // the last pass's records are no longer read
    for (int e = threadIdx.x; e < bn * W; e += 256) ys[(e / W) * LD + e % W] = X[(long long)y0 * W + e];
    __syncthreads();
#pragma unroll 4
    for (int b = wv; b < bn; b += 4) {
      uint32_t y[LD];
#pragma unroll
      for (int k = 0; k < LD; k += 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(ys + b * LD + k);
        y[k] = v.x, y[k + 1] = v.y, y[k + 2] = v.z, y[k + 3] = v.w;
      }
      bool match;
      int sign;
      sst_test(y, s, G, match, sign);
      cnt += match ? 1 : 0, sum += match ? sign : 0;
    }
  }
  part[wv][lane] = sum, part[wv][SST_BLOCK + lane] = cnt;
  __syncthreads();
  if (threadIdx.x < SST_ROW)
    g.rows[(g.task0 + blockIdx.x) * SST_ROW + threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// rows [(state, block, range)][SST_ROW] of a batch of mb strings -> sums, counts [n_states][mb]
__global__ __launch_bounds__(256) void qk_sst_total_kernel(const int32_t* rows, const long long count, const int mb, const int blocks, const int ranges, long long* sums,
                                                           long long* counts) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  const long long state = e / mb;
  const int j = (int)(e % mb);
  const int32_t* const r = rows + ((state * blocks + j / SST_BLOCK) * ranges) * SST_ROW + j % SST_BLOCK;
  long long a = 0, b = 0;
  for (int k = 0; k < ranges; ++k) a += r[(long long)k * SST_ROW], b += r[(long long)k * SST_ROW + SST_BLOCK];
  sums[e] = a, counts[e] = b;
}

int shot_strings(qk_ctx* c, const int32_t n, const int32_t ns, const int32_t shots, const uint8_t* bits, const uint8_t* bases, const int32_t per_state, const int32_t m,
                 const uint8_t* strings, int64_t* sums, int64_t* counts) {
  static const char* what = "qk_shot_strings_host";
  if (!c) return qk_fail(QK_EINVAL, "%s: ctx is null", what);
  if (!bits) return qk_fail(QK_EINVAL, "%s: bits is null", what);
  if (!bases) return qk_fail(QK_EINVAL, "%s: bases is null", what);
  if (!strings) return qk_fail(QK_EINVAL, "%s: strings is null", what);
  if (!sums) return qk_fail(QK_EINVAL, "%s: sums is null", what);
  if (!counts) return qk_fail(QK_EINVAL, "%s: counts is null", what);
  if (n < 1) return qk_fail(QK_EINVAL, "%s: n_sites must be >= 1 (got %d)", what, n);
  if (n > SHK_MAX_QUBITS) return qk_fail(QK_EINVAL, "%s: n_sites must be <= %d (got %d)", what, SHK_MAX_QUBITS, n);
  if (ns < 1) return qk_fail(QK_EINVAL, "%s: n_states must be >= 1 (got %d)", what, ns);
  if (shots < 1) return qk_fail(QK_EINVAL, "%s: shots must be >= 1 (got %d)", what, shots);
  if (m < 1) return qk_fail(QK_EINVAL, "%s: n_strings must be >= 1 (got %d)", what, m);
  if (per_state != 0 && per_state != 1) return qk_fail(QK_EINVAL, "%s: bases_per_state must be 0 or 1 (got %d)", what, per_state);
  long long cap = 0;  // strings per batch
  if (const int rc = batch_cap(what, "QK_SHOT_STRINGS_BATCH", cap)) return rc;
  const int groups = shk_groups(n), words = shk_words(n), sw = sst_words(n);
  // the string records, whole blocks of them: what lies beyond the last string is the identity
  std::vector<uint32_t> srec((size_t)sst_blocks(m) * SST_BLOCK * sw, 0u);
  for (int j = 0; j < m; ++j) {
    bool bad = false;
    sst_pack_string(strings + (size_t)j * n, n, srec.data() + (size_t)j * sw, bad);
    if (bad) return qk_fail(QK_EINVAL, "%s: strings[%d] holds a code above 3 (0 .. 3 = I, X, Y, Z)", what, j);
  }
  QkRangeGuard range_("qk:shot_strings");
  HIP_TRY_AS(what, hipSetDevice(c->device));
  HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
  QkDevBuf recs, dbad;
  HIP_TRY_AS(what, recs.alloc((size_t)ns * shots * words * sizeof(uint32_t)));
  HIP_TRY_AS(what, dbad.alloc(2 * sizeof(int32_t)));
  HIP_TRY_AS(what, hipMemset(dbad.get(), 0, 2 * sizeof(int32_t)));
  // memory bound of the staged outcome bytes and of a string batch: a quarter of what is free once the records exist
  long long budget = 0;
  if (const int rc = quarter_of_free(c, what, budget)) return rc;
  const long long room = budget * (long long)sizeof(double);
  if (const int rc = shk_pack_table(c, what, "bits", "bases", bits, bases, per_state, ns, shots, n, room, recs.get<uint32_t>(), dbad.get<int32_t>())) return rc;

  const int task_chunks = sst_task_chunks(shots, (long long)ns * sst_blocks(m)), ranges = sst_ranges(shots, task_chunks);
  const long long batch = std::min((long long)m, sst_batch_strings(room, n, ns, ranges, cap));
  SstArgs q{};
  q.recs = recs.get<uint32_t>(), q.shots = shots, q.task_chunks = task_chunks;
  for (long long m0 = 0; m0 < m; m0 += batch) {
    const int mb = (int)std::min(batch, m - m0), blocks = sst_blocks(mb);
    const long long tasks = (long long)ns * blocks * ranges, cells = (long long)ns * mb;
    // one device buffer for the string batch: [string records | per-task rows | sums | counts]
    const size_t b_strs = al256((size_t)blocks * SST_BLOCK * sw * sizeof(uint32_t)), b_rows = al256((size_t)tasks * SST_ROW * sizeof(int32_t)),
                 b_out = al256((size_t)cells * sizeof(int64_t));
    HIP_TRY_AS(what, c->local_scratch.ensure(b_strs + b_rows + 2 * b_out));
    char* const base = c->local_scratch.get<char>();
    q.strs = reinterpret_cast<const uint32_t*>(base);
    q.rows = reinterpret_cast<int32_t*>(base + b_strs);
    q.blocks = blocks;
    long long* const d_sums = reinterpret_cast<long long*>(base + b_strs + b_rows);
    long long* const d_counts = reinterpret_cast<long long*>(base + b_strs + b_rows + b_out);
    // the batch's records and, where its last block is ragged, the identity behind them (srec is zero beyond string m)
    HIP_TRY_AS(what, hipMemsetAsync(base, 0, b_strs, c->stream));
    HIP_TRY_AS(what, hipMemcpyAsync(base, srec.data() + (size_t)m0 * sw, (size_t)mb * sw * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    for (long long t0 = 0; t0 < tasks; t0 += SST_LAUNCH_TASKS) {
      q.task0 = t0;
      const dim3 grid((unsigned)std::min((long long)SST_LAUNCH_TASKS, tasks - t0));
      if (groups == 1) qk_sst_kernel<1><<<grid, dim3(256), 0, c->stream>>>(q);
      else if (groups == 2) qk_sst_kernel<2><<<grid, dim3(256), 0, c->stream>>>(q);
      else if (groups == 3) qk_sst_kernel<3><<<grid, dim3(256), 0, c->stream>>>(q);
      else qk_sst_kernel<4><<<grid, dim3(256), 0, c->stream>>>(q);
    }
    HIP_TRY_AS(what, hipGetLastError());
    qk_sst_total_kernel<<<dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream>>>(q.rows, cells, mb, blocks, ranges, d_sums, d_counts);
    HIP_TRY_AS(what, hipGetLastError());
    HIP_TRY_AS(what, hipStreamSynchronize(c->stream));
    // the batch is the columns m0 .. m0 + mb of the caller's tables
    HIP_TRY_AS(what, hipMemcpy2D(sums + m0, (size_t)m * sizeof(int64_t), d_sums, (size_t)mb * sizeof(int64_t), (size_t)mb * sizeof(int64_t), (size_t)ns, hipMemcpyDeviceToHost));
    HIP_TRY_AS(what, hipMemcpy2D(counts + m0, (size_t)m * sizeof(int64_t), d_counts, (size_t)mb * sizeof(int64_t), (size_t)mb * sizeof(int64_t), (size_t)ns, hipMemcpyDeviceToHost));
  }
  return QK_OK;
}

}  // namespace

extern "C" int qk_shot_strings_host(qk_ctx* c, int32_t n_sites, int32_t n_states, int32_t shots, const uint8_t* bits, const uint8_t* bases, int32_t bases_per_state,
                                    int32_t n_strings, const uint8_t* strings, int64_t* sums, int64_t* counts) {
  return shot_strings(c, n_sites, n_states, shots, bits, bases, bases_per_state, n_strings, strings, sums, counts);
}

extern "C" int qk_shadow_hist_host(qk_ctx* c, int32_t n_sites, int32_t nx, int32_t shots_x, const uint8_t* bits_x, const uint8_t* bases_x, int32_t bases_x_per_state, int32_t ny,
                                   int32_t shots_y, const uint8_t* bits_y, const uint8_t* bases_y, int32_t bases_y_per_state, int64_t n_pairs, const int32_t* pairs, int64_t* hist,
                                   int64_t* equal) {
  return shadow_hist(c, n_sites, nx, shots_x, bits_x, bases_x, bases_x_per_state, ny, shots_y, bits_y, bases_y, bases_y_per_state, n_pairs, pairs, hist, equal);
}

extern "C" int qk_window_rdms_host(qk_ctx* c, const qk_mps_set* set, int32_t width, int32_t n_starts, const int32_t* starts, double* rho, double* norms) {
  return window_rdms(c, set, width, n_starts, starts, rho, norms);
}

extern "C" int qk_shot_block_sums_host(qk_ctx* c, int32_t n_sites, int32_t n_settings, int32_t shots_per_setting, int32_t nx, const uint8_t* bits_x, int32_t ny,
                                       const uint8_t* bits_y, int64_t n_pairs, const int32_t* pairs, int32_t side, int32_t n_widths, const int32_t* widths, int64_t* sums,
                                       int64_t* per_setting) {
  return shot_block_sums(c, n_sites, n_settings, shots_per_setting, nx, bits_x, ny, bits_y, n_pairs, pairs, side, n_widths, widths, sums, per_setting);
}

extern "C" int qk_amplitudes_host(qk_ctx* c, const qk_mps_set* set, int32_t n_strings, const uint8_t* bits, int32_t bits_per_state, const uint8_t* bases, double* mant,
                                  int32_t* expo, double* logp, double* norms) {
  return amplitudes_run(c, set, n_strings, bits, bits_per_state, bases, mant, expo, logp, norms);
}

extern "C" int qk_sample_host(qk_ctx* c, const qk_mps_set* set, int32_t n_shots, const uint8_t* bases, uint64_t seed, int64_t first_state, uint8_t* bits, double* logp) {
  return sample_run(c, set, n_shots, bases, seed, first_state, bits, logp);
}

extern "C" int qk_block_values_host(qk_ctx* c, const qk_mps_set* xset, const qk_mps_set* yset, const qk_plan* plan, int32_t side, int32_t n_widths, const int32_t* widths,
                                    double* values_host) {
  static const char* what = "qk_block_values_host";
  if (!plan) return qk_fail(QK_EINVAL, "%s: plan is null", what);
  if (!values_host) return qk_fail(QK_EINVAL, "%s: values_host is null", what);
  if (const int rc = block_check(c, what, xset, yset, side, n_widths, widths)) return rc;
  const long long np = (long long)plan->pairs.size() / 2;
  const int nx = xset->n_states, ny = yset ? yset->n_states : nx;
  for (long long e = 0; e < np; ++e) {
    const int i = plan->pairs[2 * e], j = plan->pairs[2 * e + 1];
    if (i < 0 || i >= nx || j < 0 || j >= ny) return qk_fail(QK_EINVAL, "%s: pair %lld of the plan is (%d, %d), the sets hold %d x %d states", what, e, i, j, nx, ny);
  }
  return block_run(c, what, xset, yset, np, plan->pairs.data(), side, n_widths, widths, values_host, nullptr);
}

extern "C" int qk_block_self_host(qk_ctx* c, const qk_mps_set* set, int32_t side, int32_t n_widths, const int32_t* widths, double* out, double* norms) {
  static const char* what = "qk_block_self_host";
  if (!out) return qk_fail(QK_EINVAL, "%s: out is null", what);
  if (const int rc = block_check(c, what, set, nullptr, side, n_widths, widths)) return rc;
  std::vector<int32_t> pairs((size_t)2 * set->n_states);
  for (int s = 0; s < set->n_states; ++s) pairs[2 * s] = pairs[2 * s + 1] = s;
  return block_run(c, what, set, nullptr, set->n_states, pairs.data(), side, n_widths, widths, out, norms);
}

extern "C" int qk_bond_purities_host(qk_ctx* c, const qk_mps_set* set, double* out, double* norms) {
  return bond_call(c, set, "qk_bond_purities_host", "qk:bond_purities", 0, out, norms);
}

extern "C" int qk_bond_spectra_host(qk_ctx* c, const qk_mps_set* set, int32_t max_values, double* out, double* norms) {
  static const char* what = "qk_bond_spectra_host";
  if (max_values < 1) return qk_fail(QK_EINVAL, "%s: max_values must be >= 1 (got %d)", what, max_values);
  return bond_call(c, set, what, "qk:bond_spectra", max_values, out, norms);
}

extern "C" int qk_pauli_strings_host(qk_ctx* c, const qk_mps_set* set, int32_t n_strings, const uint8_t* strings, double* out, double* norms) {
  return string_chains(c, set, "qk_pauli_strings_host", "qk:pauli_strings", "QK_STRINGS_BATCH", 0, nullptr, n_strings, strings, out, norms);
}
extern "C" int qk_operator_strings_host(qk_ctx* c, const qk_mps_set* set, int32_t n_ops, const double* ops, int32_t n_strings, const uint8_t* strings, double* out,
                                        double* norms) {
  if (!ops) return qk_fail(QK_EINVAL, "qk_operator_strings_host: ops is null");
  return string_chains(c, set, "qk_operator_strings_host", "qk:operator_strings", "QK_OPSTR_BATCH", n_ops, ops, n_strings, strings, out, norms);
}
extern "C" int qk_mpo_expectations_host(qk_ctx* c, const qk_mps_set* set, int32_t n_mpos, const int32_t* bonds, const double* tensors, double* out, double* norms) {
  return mpo_chains(c, set, n_mpos, bonds, tensors, out, norms);
}
extern "C" int qk_mps_set_apply_mpo(qk_ctx* c, const qk_mps_set* src, const int32_t* bonds, const double* tensors, qk_mps_set** out) {
  return apply_mpo(c, src, bonds, tensors, out);
}

extern "C" int qk_feature_gram_host(qk_ctx* c, int32_t n_features, int32_t nx, const double* fx, int32_t ny, const double* fy, double g, double* out, int64_t ld) {
  static const char* what = "qk_feature_gram_host";
  if (n_features < 1) return qk_fail(QK_EINVAL, "%s: n_features must be >= 1 (got %d)", what, n_features);
  return projected_gram(c, what, "qk:feature_gram", 1, 1, n_features, 1.0, nx, fx, ny, fy, g, out, ld);
}

extern "C" int qk_local_paulis_host(qk_ctx* c, const qk_mps_set* set, double* out, double* norms) {
  static const char* what = "qk_local_paulis_host";
  if (!out) return qk_fail(QK_EINVAL, "%s: null argument", what);
  return local_sweep(c, set, what, "qk:local_paulis", out, norms, nullptr, 1);
}

extern "C" int qk_local_pair_paulis_host(qk_ctx* c, const qk_mps_set* set, double* out2, double* out1, double* norms) {
  static const char* what = "qk_local_pair_paulis_host";
  if (!out2) return qk_fail(QK_EINVAL, "%s: null argument", what);
  return local_sweep(c, set, what, "qk:local_pair_paulis", out1, norms, out2, 1);
}

extern "C" int qk_local_pair_paulis_dist_host(qk_ctx* c, const qk_mps_set* set, int32_t max_dist, double* out2, double* out1, double* norms) {
  static const char* what = "qk_local_pair_paulis_dist_host";
  if (!out2) return qk_fail(QK_EINVAL, "%s: null argument", what);
  return local_sweep(c, set, what, "qk:local_pair_paulis_dist", out1, norms, out2, max_dist);
}

extern "C" int qk_projected_gram_host(qk_ctx* c, int32_t n_sites, int32_t nx, const double* fx, int32_t ny, const double* fy, double g, double* out, int64_t ld) {
  return projected_gram(c, "qk_projected_gram_host", "qk:projected_gram", n_sites, 1, 3 * n_sites, 0.5, nx, fx, ny, fy, g, out, ld);
}

extern "C" int qk_projected_pair_gram_host(qk_ctx* c, int32_t n_sites, int32_t nx, const double* tx, int32_t ny, const double* ty, double g, double* out, int64_t ld) {
  return projected_gram(c, "qk_projected_pair_gram_host", "qk:projected_pair_gram", n_sites, 2, 16 * (n_sites - 1), 0.25, nx, tx, ny, ty, g, out, ld);
}

extern "C" int qk_projected_pair_gram_dist_host(qk_ctx* c, int32_t n_sites, int32_t max_dist, int32_t nx, const double* tx, int32_t ny, const double* ty, double g, double* out,
                                                int64_t ld) {
  static const char* what = "qk_projected_pair_gram_dist_host";
  if (n_sites >= 2 && (max_dist < 1 || max_dist > n_sites - 1))
    return qk_fail(QK_EINVAL, "%s: max_dist must be in 1 .. n_sites - 1 = %d (got %d)", what, n_sites - 1, max_dist);
  const int np = n_sites >= 2 ? n_pairs(max_dist, n_sites) : 0;
  return projected_gram(c, what, "qk:projected_pair_gram_dist", n_sites, 2, 16 * np, 0.25, nx, tx, ny, ty, g, out, ld);
}
