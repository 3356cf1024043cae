// qk_local_plan.h -- the host-side plan of the local sweeps (qk_local.hip): the launch kinds, the scratch layout, the pair index, the
// sizes and the cut into state batches, the tables and task lists of a batch, the plans of the entry points, the chain side of the
// Pauli strings, of the block kernels, of the sampler, of the amplitude chains, of the k-qubit windows and of the MPO observables, the device buffer of a chain
// batch (chain_stage, tests/host_san/chain_stage_main.cpp) and the batch cap of the environment (batch_cap), the integer side of the shot-based block overlaps , of the shadow kernel's shot-pair histograms and of the Pauli strings estimated from shots.  Plain C++: no HIP type appears here, so all of it is tested on the CPU (tests/host_san/local_plan_main.cpp,
// -fsanitize=address,undefined); the few functions the kernels also call are QK_HD.
#pragma once
#include "qk_plan.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

namespace qkl {

constexpr int LOC_CHUNK = 16;  // rows per reduction task

// Every launch kind of qk_local.hip.  Kinds >= 0 are GEMM launches (64 x 64 output blocks), the others elementwise or reductions
// in 16-row chunks.  LOC_*: tasks (batch entry, block), qk_local_gemm_kernel; STR_*: tasks (chain, block), qk_str_gemm_kernel;
// BLK_*: tasks (pair chain, block), qk_blk_gemm_kernel; SMP_*: tasks (shot chain, block), qk_smp_gemm_kernel; WIN_*: tasks (window
// chain, block), qk_win_gemm_kernel; AMP_*: tasks (amplitude chain, block), qk_amp_gemm_kernel; MPO_*: tasks (MPO chain, block),
// qk_mpo_gemm_kernel.
enum LocKind : int {
  LOC_REV_T = 0,   // reversed chain: T = Lr^T Ar_j              (Lr_j = R_{o+1}, o = n-1-j)
  LOC_REV_X = 1,   // reversed chain: R_o = T^T conj(Ar_j)
  LOC_FWD_T = 2,   // T_k = L_k^T A_k
  LOC_FWD_W = 3,   // W_{k,s} = T_k[(., s)]^T conj(A_k), both s in one launch
  LOC_PAIR_T = 4,  // pair sweep, site o = k+1 of the reversed image: T' = R_{o+1}^T Ar_o
  LOC_PAIR_V = 5,  // pair sweep: V_{o,t} = T'[(., t)]^T conj(Ar_o), both t in one launch
  LOC_DIST_T = 6,  // distant pairs, site k: T''_(o,s,s') = E_{o->k}[s][s']^T A_k for every live origin o, in one launch
  LOC_DIST_X = 7,  // distant pairs: E_{o->k+1}[s][s'] = T''_(o,s,s')^T conj(A_k) over K = (a, u), back into the origin's slot
  LOC_BOND_M = 8,  // bond purities: M_k = L_k^T R_k (= N_k^H) of bond k = step, from the kept environments into the T planes
  STR_T = 9,       // T[a][(s, b')] = sum_b E_k[b][a] A_k[b][(s, b')] of every live chain (the LOC_DIST_T shape); E_a is read from the kept L_a
  STR_X = 10,      // E_{k+1}[b'][a'] = sum_{(a,u)} T[(a, u)][b'] conj(A_k[(a, u)][a']) over K = 2 chi_k (the LOC_DIST_X shape)
  BLK_T = 11,      // pair chain (x_i, y_j), step j: T[a][(s, b')] = sum_b E[b][a] Ay[b][(s, b')] (the STR_T shape, A from the y state)
  BLK_X = 12,      // pair chain: E'[b'][a'] = sum_{(a,u)} T[(a, u)][b'] conj(Ax[(a, u)][a']) (the STR_X shape, A from the x state)
  BLK_V = 13,      // pair chain at a chosen cut: V = Ry^T E
  BLK_W = 14,      // pair chain at a chosen cut: W = E^T conj(V)
  LOC_RHO = -1,       // qk_local_rho_kernel
  LOC_PAIR_RHO = -2,  // qk_local_pair_rho_kernel<false>
  LOC_DIST_RHO = -3,  // qk_local_pair_rho_kernel<true>: rho_{o,k+1} of every live origin from its window slot
  LOC_ADMIT = -4,     // qk_local_admit_kernel: W_k into the window
  LOC_BOND_TR = -5,   // qk_bond_trace_kernel: tr(M_k^2) of bond k = step in 16-row chunks
  STR_LNEXT = -6,     // qk_str_lnext_kernel (environment pass): L_{k+1} = W_0[.][(0, .)] + W_1[.][(1, .)], kept
  STR_PAULI = -7,     // qk_str_pauli_kernel: T[a][(s ^ f, b')] <- i^e(s) T[a][(s, b')] of the chains whose code at site k is not I
                      // (operator strings: qk_str_op_kernel, T[a][(s', b')] <- sum_s O[s'][s] T[a][(s, b')], on the same tasks)
  STR_CLOSE = -8,     // qk_str_close_kernel: sum E_{b+1} R_{b+1} of the chains whose support ends at site k (operator strings:
                      // qk_str_closez_kernel, Re and Im, on the same tasks)
  BLK_RED = -9,       // qk_blk_reduce_kernel: Re sum Rx[a][a'] conj(W[a][a']) of a chosen cut in 16-row chunks
  SMP_W = 15,         // shot chain (state, shot tile), site k: W[row][(t, b')] = sum_b V[b][row] A_k[b][(t, b')], shot rows as M
  SMP_Q = 16,         // shot chain: Q[(o, row)][a'] = sum_b' W'_o[row][b'] R_{k+1}[b'][a'], the stacked operand [W'_0 ; W'_1] as M
  SMP_ROT = -10,      // qk_smp_rotate_kernel: W -> the stacked operand by each row's basis code, in 16-row chunks
  SMP_DRAW = -11,     // qk_smp_draw_kernel: p_0, p_1 of a row, its uniform, its bit, log p and the next V, one wave per row
  WIN_G = 17,         // window chain (state, window [a, b)), step j, site c = b-1-j: G_{j+1}[beta][(t, sigma, gamma)] = sum_beta' A_c[beta][t][beta'] G_j[beta'][(sigma, gamma)]
                      // of both seeds (G_0 = 1, Gr_0 = R_b) and both t in one launch; the reversed image's site c is the A operand
  WIN_H = 18,         // window chain: H[alpha'][(s, gamma)] = sum_alpha L_a[alpha][alpha'] G_w[alpha][(s, gamma)] (the LOC_FWD_T shape, N = 2^w chi_b)
  WIN_CLOSE = -12,    // qk_win_close_kernel: sum Gr_w[alpha][(s, gamma')] conj(H[alpha][(s', gamma')]) of every s <= s' in 16-row chunks of alpha
  AMP_W = 19,         // amplitude chain (state, string tile), site k: W[row][(t, b')] = sum_b V[b][row] A_k[b][(t, b')] (the SMP_W shape)
  AMP_PICK = -13,     // qk_amp_pick_kernel: W'_{bit} of a row in its basis, its maximum, its exponent and the scaled next V, one wave per row
  MPO_T = 20,         // MPO chain (state, MPO), site k: T[(u, a)][(s, b')] = sum_b E[u][b][a] A_k[b][(s, b')], the w_k planes of E stacked along M
  MPO_X = 21,         // MPO chain: E'[v][b'][a'] = sum_{(a,s')} T'[v][(a, s')][b'] conj(A_k[(a, s')][a']) of every plane v (the STR_X shape), at column v pad_{k+1}
  MPO_MIX = -14,      // qk_mpo_mix_kernel: T'[v][(a, s')] = sum_u sum_s W_k[u][v][s'][s] T[u][(a, s)] over the listed blocks, one 16-row chunk of one v plane
  MPO_CLOSE = -15,    // qk_str_closez_kernel on the chains whose support ends at site k
};
QK_HD constexpr bool conj_b(const int kind) { return kind == LOC_REV_X || kind == LOC_FWD_W || kind == LOC_PAIR_V || kind == LOC_DIST_X || kind == STR_X || kind == BLK_X || kind == BLK_W || kind == MPO_X; }

// ---- the scratch layout ---------------------------------------------------------------------------------------------------------
// Per-state scratch (doubles, every matrix as a re plane then an im plane), P = the state's largest padded bond, offsets in units
// of P^2:
//   L [P x P] at at_L() = 0 | T [P x 2P] at at_T() = 2 | W_s [P x 2P] at at_W(s) = 6 + 4s | kept environments from rmul on
// The pair sweep has T' at at_Tp() = 14 and V_t at at_V(t) = 18 + 4t before the kept environments.  Pairs up to distance D add the
// window -- D - 1 slots of 8, origin o in window_slot(o, D) = 26 + 8 (o mod (D - 1)), holding (W_0 | W_1) of its origin carried to
// the current bond -- and the 4 (D - 1) intermediates T'' of 4 at window_tmp(w, D) = 26 + 8 (D - 1) + 4w, w = 4 (k - 1 - o) + 2s + s'.
// The kept environments start at rmul(pair, D) = 14 (one-qubit sweep and the environment pass), 26 + 24 (D - 1) (pair sweeps):
// R_k (k = 1 .. n) at rmul P^2 + roff[k], pad_k^2 per plane, and -- where the L_k are kept -- L_k (k = 0 .. n-1) at rmul P^2 + loff[k].
// A chain of the Pauli strings has a slot of chain_size() = 6: E [P x P] at chain_E() = 0 (ld = the current padded bond) | T [P x 2P]
// at chain_T() = 2.
QK_HD constexpr int at_L() { return 0; }
QK_HD constexpr int at_T() { return 2; }
QK_HD constexpr int at_W(const int s) { return 6 + 4 * s; }
QK_HD constexpr int at_Tp() { return 14; }
QK_HD constexpr int at_V(const int t) { return 18 + 4 * t; }
QK_HD constexpr int window_slot(const int o, const int D) { return 26 + 8 * (o % (D - 1)); }
QK_HD constexpr int window_tmp(const int w, const int D) { return 26 + 8 * (D - 1) + 4 * w; }
QK_HD constexpr int rmul(const bool pair, const int D) { return pair ? 26 + 24 * (D - 1) : 14; }
constexpr int LOC_RMUL = rmul(false, 1);  // the environment pass
QK_HD constexpr int chain_E() { return 0; }
QK_HD constexpr int chain_T() { return 2; }
QK_HD constexpr int chain_size() { return 6; }

// ---- the pairs (k, k + d), d = 1 .. D, listed distance-major -----------------------------------------------------------------------
QK_HD constexpr long long pair_index(const int d, const int k, const int n) { return (long long)(d - 1) * n - (d - 1) * d / 2 + k; }
QK_HD constexpr int n_pairs(const int D, const int n) { return D * n - D * (D + 1) / 2; }
// the second qubit k + d of the pair with this index: the distance-d block has n - d pairs, second qubits d .. n-1
QK_HD constexpr int pair_second(const int index, const int n) {
  int second = index + 1;
  for (int d = 1; second > n - 1; ++d) second -= n - d - 1;
  return second;
}

// ---- sizes and state batches ----------------------------------------------------------------------------------------------------
inline long long blocks64(const long long m, const long long n) { return ((m + 63) / 64) * ((n + 63) / 64); }
inline size_t al256(const size_t b) { return (b + 255) / 256 * 256; }

struct EnvSizes {
  int n_states = 0, n_sites = 0;
  int rmul = LOC_RMUL;          // start of the kept environments
  bool keep_l = false;          // the L_k are kept behind the R_k
  int max_dist = 1, n_pairs = 0;  // the pair sweeps (set by local_sweep)
  std::vector<int32_t> pad;     // padded bonds [n_states][n_sites + 1]
  std::vector<int> pmax;        // P of each state
  std::vector<long long> need;  // scratch doubles of each state: rmul P^2, R_1 .. R_n and, if kept, L_0 .. L_{n-1}
  int max_chunks = 0;
};
inline void env_sizes(const int32_t* tru, const int ns, const int n, const int max_pad, const int rmul, const bool keep_l, EnvSizes& z) {
  const int n1 = n + 1;
  z.n_states = ns, z.n_sites = n, z.rmul = rmul, z.keep_l = keep_l;
  z.pad.resize((size_t)ns * n1), z.pmax.resize(ns), z.need.resize(ns);
  for (int s = 0; s < ns; ++s) {
    int p = 16;
    long long esum = 0;
    for (int k = 0; k <= n; ++k) {
      const int d = z.pad[(size_t)s * n1 + k] = qk_pad16(tru[(size_t)s * n1 + k]);
      p = std::max(p, d);
      esum += (k >= 1 ? 2ll * d * d : 0) + (keep_l && k < n ? 2ll * d * d : 0);
    }
    z.pmax[s] = p;
    z.need[s] = (long long)rmul * p * p + esum;
  }
  z.max_chunks = max_pad / LOC_CHUNK;
}

// The cut into batches: consecutive states while their weights (weight[s] + each) fit the budget, at least one state per batch.
// Returns the first state of every batch, then the number of states.
inline std::vector<int> batch_cut(const std::vector<long long>& weight, const long long each, const long long budget) {
  std::vector<int> bstart{0};
  long long acc = 0;
  for (size_t s = 0; s < weight.size(); ++s) {
    const long long w = weight[s] + each;
    if (acc > 0 && acc + w > budget) bstart.push_back((int)s), acc = 0;
    acc += w;
  }
  bstart.push_back((int)weight.size());
  return bstart;
}

// ---- plans: the launches of a batch as (kind, step), in stream order ------------------------------------------------------------------
using Plan = std::vector<std::pair<int, int>>;
// the reversed chain, steps j = 0 .. n-2: R_{n-1} .. R_1 (R_0 is not needed)
inline void plan_reverse(const int n, Plan& plan) {
  for (int j = 0; j < n - 1; ++j) plan.push_back({LOC_REV_T, j}), plan.push_back({LOC_REV_X, j});
}
// the environment pass: the reversed chain, then per site forward T / W and L_{k+1}
inline Plan env_plan(const int n) {
  Plan plan;
  plan_reverse(n, plan);
  for (int k = 0; k < n; ++k) plan.push_back({LOC_FWD_T, k}), plan.push_back({LOC_FWD_W, k}), plan.push_back({STR_LNEXT, k});
  return plan;
}
// the local sweep: the reversed chain, then per site forward T / W, the pair sweep's T' / V of site k+1, rho (which also makes
// L_{k+1}) and the pair rho; with D > 1 then the live origins k-D+1 .. k-1 through site k, their rho_{o,k+1}, and W_k into the
// window for the sites after k+1
inline Plan local_plan(const int n, const bool pair, const int D) {
  Plan plan;
  plan_reverse(n, plan);
  for (int k = 0; k < n; ++k) {
    plan.push_back({LOC_FWD_T, k}), plan.push_back({LOC_FWD_W, k});
    if (pair && k + 1 < n) plan.push_back({LOC_PAIR_T, k}), plan.push_back({LOC_PAIR_V, k});
    plan.push_back({LOC_RHO, k});
    if (pair && k + 1 < n) plan.push_back({LOC_PAIR_RHO, k});
    if (D > 1 && k >= 1 && k + 1 < n) plan.push_back({LOC_DIST_T, k}), plan.push_back({LOC_DIST_X, k}), plan.push_back({LOC_DIST_RHO, k});
    if (D > 1 && k + 2 < n) plan.push_back({LOC_ADMIT, k});
  }
  return plan;
}
// the bond purities, after the environment pass: per bond k = 1 .. n-1 the product M_k and its trace
inline Plan bond_tail(const int n) {
  Plan plan;
  for (int k = 1; k < n; ++k) plan.push_back({LOC_BOND_M, k}), plan.push_back({LOC_BOND_TR, k});
  return plan;
}

// ---- tasks and tables of a batch ----------------------------------------------------------------------------------------------------
// The blocks of one state (p = its padded bonds [n + 1]) in a launch: 64 x 64 output blocks of a GEMM kind, 16-row chunks otherwise.
// step = reversed-chain step j (LOC_REV_*: site o = n-1-j), site k (forward, STR_*; LOC_PAIR_*: the pair (k, k+1)) or bond k
// (LOC_BOND_*).  The STR_* counts are those of a chain that takes part in the launch (chain_lists decides which do).
inline int task_count(const int kind, const int step, const int32_t* p, const int n, const int D) {
  const int o = n - 1 - step, k = step;
  const int live = std::min(k, D - 1);  // origins in the window at site k
  switch (kind) {
    case LOC_REV_T: return (int)blocks64(p[o + 1], 2ll * p[o]);
    case LOC_REV_X: return (int)blocks64(p[o], p[o]);
    case LOC_FWD_T: case STR_T: return (int)blocks64(p[k], 2ll * p[k + 1]);
    case LOC_FWD_W: case LOC_PAIR_V: return (int)(2 * blocks64(p[k + 1], 2ll * p[k + 1]));
    case LOC_PAIR_T: return (int)blocks64(p[k + 2], 2ll * p[k + 1]);
    case LOC_DIST_T: return (int)(4 * live * blocks64(p[k], 2ll * p[k + 1]));
    case LOC_DIST_X: return (int)(4 * live * blocks64(p[k + 1], p[k + 1]));
    case LOC_DIST_RHO: return live * (p[k + 1] / LOC_CHUNK);
    case LOC_BOND_M: return (int)blocks64(p[k], p[k]);
    case STR_X: return (int)blocks64(p[k + 1], p[k + 1]);
    case LOC_BOND_TR: case STR_PAULI: return p[k] / LOC_CHUNK;
    default: return p[k + 1] / LOC_CHUNK;  // LOC_RHO, LOC_PAIR_RHO, LOC_ADMIT, STR_LNEXT, STR_CLOSE
  }
}

struct Task2 {  // int2 of the device: (batch entry or chain, block)
  int x, y;
};
struct EnvTables {
  int s0 = 0, nb = 0;
  long long tot = 0;  // scratch doubles of the batch
  std::vector<int32_t> h_states, h_pmax;   // batch entry -> state of the set, P
  std::vector<int64_t> h_sbase;            // batch entry -> first double of its scratch
  std::vector<int64_t> h_roff, h_loff;     // [batch][n_sites + 1]: R_k, L_k behind rmul P^2 (h_loff empty unless the L_k are kept)
  std::vector<Task2> tasks;                // of every launch of the plan, in launch order
  std::vector<long long> first;            // per launch: first task; then the number of tasks
  // the batch's device buffer: [tables | tasks | partial sums | scratch | `extra` bytes of the caller]
  size_t b_states = 0, b_pmax = 0, b_sbase = 0, b_roff = 0, b_tasks = 0, b_part = 0, b_tab = 0, b_env = 0;
  size_t used() const { return b_tab + b_part + b_env; }
};
// host tables and task lists of the states [s0, s0 + nb) for `plan`
inline void env_tables(const EnvSizes& z, const Plan& plan, const int s0, const int nb, const long long part_per_state, EnvTables& eb) {
  const int n = z.n_sites, n1 = n + 1;
  eb.s0 = s0, eb.nb = nb, eb.tot = 0;
  eb.h_states.resize(nb), eb.h_pmax.resize(nb), eb.h_sbase.resize(nb), eb.h_roff.resize((size_t)nb * n1), eb.h_loff.resize(z.keep_l ? (size_t)nb * n1 : 0);
  for (int i = 0; i < nb; ++i) {
    const int s = s0 + i;
    const int32_t* p = &z.pad[(size_t)s * n1];
    eb.h_states[i] = s, eb.h_pmax[i] = z.pmax[s], eb.h_sbase[i] = eb.tot;
    long long ro = 0;
    for (int k = 0; k <= n; ++k) {
      eb.h_roff[(size_t)i * n1 + k] = ro;
      if (k >= 1) ro += 2ll * p[k] * p[k];
    }
    for (int k = 0; z.keep_l && k <= n; ++k) {  // the L_k behind the R_k
      eb.h_loff[(size_t)i * n1 + k] = ro;
      ro += 2ll * p[k] * p[k];
    }
    eb.tot += z.need[s];
  }
  eb.tasks.clear(), eb.first.clear();
  for (const auto& [kind, step] : plan) {
    eb.first.push_back((long long)eb.tasks.size());
    for (int i = 0; i < nb; ++i) {
      const int nbk = task_count(kind, step, &z.pad[(size_t)(s0 + i) * n1], n, z.max_dist);
      for (int b = 0; b < nbk; ++b) eb.tasks.push_back(Task2{i, b});
    }
  }
  eb.first.push_back((long long)eb.tasks.size());
  eb.b_states = al256(nb * sizeof(int32_t)), eb.b_pmax = al256(nb * sizeof(int32_t)), eb.b_sbase = al256(nb * sizeof(int64_t));
  eb.b_roff = al256(eb.h_roff.size() * sizeof(int64_t)), eb.b_tasks = al256(eb.tasks.size() * sizeof(Task2));
  eb.b_part = al256((size_t)nb * part_per_state * sizeof(double));
  eb.b_tab = eb.b_states + eb.b_pmax + eb.b_sbase + (z.keep_l ? 2 : 1) * eb.b_roff + eb.b_tasks, eb.b_env = al256((size_t)eb.tot * sizeof(double));
}

// ---- the chains of the Pauli strings --------------------------------------------------------------------------------------------------
// A string is codes[0 .. n-1], 0..3 = I, X, Y, Z; its support [a, b] = its first and last non-identity sites.  A chain is one
// (state, string) with a non-identity site.
// supp[2m], supp[2m + 1] = a, b of string m (-1, -1: all identity).  Returns -1, or the index m n + k of the first code above 3.
// operator_supports is the same for the strings of single-site operators (qk_operator_strings_host): code c = 1 .. n_ops names the
// 2 x 2 matrix ops[c] of the call's table, 0 the identity; it returns -1, or the index m n + k of the first code above n_ops.  The
// chains below ask only whether a code is 0, so they serve both kinds of string.
inline long long operator_supports(const uint8_t* strings, const int n_strings, const int n, const int n_ops, std::vector<int32_t>& supp) {
  supp.assign((size_t)2 * n_strings, -1);
  for (int m = 0; m < n_strings; ++m)
    for (int k = 0; k < n; ++k) {
      const int code = strings[(size_t)m * n + k];
      if (code > n_ops) return (long long)m * n + k;
      if (code && supp[2 * m] < 0) supp[2 * m] = k;
      if (code) supp[2 * m + 1] = k;
    }
  return -1;
}
inline long long string_supports(const uint8_t* strings, const int n_strings, const int n, std::vector<int32_t>& supp) {
  return operator_supports(strings, n_strings, n, 3, supp);
}
constexpr int OPSTR_MAX_OPS = 255;  // operators of a table: the codes of a string are bytes
constexpr int CHAIN_KINDS[4] = {STR_T, STR_PAULI, STR_X, STR_CLOSE};  // the launches of a site of the chain pass, in stream order
// the blocks of a chain (p = its state's padded bonds, codes = its string, [a, b] its support) in the launch `kind` of site k
inline int chain_task_count(const int kind, const int k, const int32_t* p, const uint8_t* codes, const int a, const int b, const int n) {
  if (k < a || k > b || (kind == STR_PAULI && !codes[k]) || (kind == STR_CLOSE && k != b)) return 0;
  return task_count(kind, k, p, n, 1);
}
struct ChainCore {  // what every chain list has, per chain
  std::vector<long long> slot, ntasks, weight;  // doubles of its slot; its tasks over all launches; its doubles: slot, partial sums, tasks and table entries
};
struct Chains : ChainCore {  // the chains of a state batch, state-major in string order
  std::vector<int32_t> cent, cstr;  // chain -> batch entry, string
};
inline Chains list_chains(const EnvSizes& z, const int s0, const int nb, const int n_strings, const uint8_t* strings, const std::vector<int32_t>& supp) {
  const int n = z.n_sites;
  Chains c;
  for (int i = 0; i < nb; ++i)
    for (int m = 0; m < n_strings; ++m)
      if (supp[2 * m] >= 0) {
        long long nt = 0;
        for (int k = supp[2 * m]; k <= supp[2 * m + 1]; ++k)
          for (const int kind : CHAIN_KINDS) nt += chain_task_count(kind, k, &z.pad[(size_t)(s0 + i) * (n + 1)], strings + (size_t)m * n, supp[2 * m], supp[2 * m + 1], n);
        c.cent.push_back(i), c.cstr.push_back(m), c.ntasks.push_back(nt);
        c.slot.push_back((long long)chain_size() * z.pmax[s0 + i] * z.pmax[s0 + i]);
        c.weight.push_back(c.slot.back() + z.max_chunks + nt + 2);
      }
  return c;
}
// The cut into chain batches: consecutive chains while their weights fit `room`, and at most `cap` of them (cap 0: the room
// alone); at least one chain per batch.  Returns the first chain of every batch, then the number of chains.
inline std::vector<size_t> chain_cut(const std::vector<long long>& weight, const long long room, const long long cap) {
  std::vector<size_t> cstart{0};
  long long acc = 0;
  for (size_t ch = 0; ch < weight.size(); ++ch) {
    if (acc > 0 && (acc + weight[ch] > room || (cap > 0 && (long long)(ch - cstart.back()) >= cap))) cstart.push_back(ch), acc = 0;
    acc += weight[ch];
  }
  cstart.push_back(weight.size());
  return cstart;
}
// Task lists (chain of the batch, block) of the chains [c0, c0 + nc): launch 4k + j is CHAIN_KINDS[j] at site k -- the live chains'
// T blocks, the Pauli chunks of those with a code at k, the X blocks, the closing chunks of those that end at k.
inline void chain_lists(const EnvSizes& z, const int s0, const Chains& c, const size_t c0, const size_t nc, const uint8_t* strings, const std::vector<int32_t>& supp,
                        std::vector<Task2>& tasks, std::vector<long long>& first) {
  const int n = z.n_sites;
  tasks.clear(), first.clear();
  for (int k = 0; k < n; ++k)
    for (const int kind : CHAIN_KINDS) {
      first.push_back((long long)tasks.size());
      for (size_t e = 0; e < nc; ++e) {
        const int m = c.cstr[c0 + e];
        const int nbk = chain_task_count(kind, k, &z.pad[(size_t)(s0 + c.cent[c0 + e]) * (n + 1)], strings + (size_t)m * n, supp[2 * m], supp[2 * m + 1], n);
        for (int b = 0; b < nbk; ++b) tasks.push_back(Task2{(int)e, b});
      }
    }
  first.push_back((long long)tasks.size());
}

// ---- the device buffer of a chain batch -------------------------------------------------------------------------------------------
// [the family's table columns, in the order listed | slot bases (int64) | tasks | partial sums | slots], every region but the slots
// rounded up with al256; the part before the partial sums is staged on the host and uploaded.  The families:
//   strings    cent, cstr                      | cbase | tasks | part  | slots
//   block      pairs (2 per chain), cpm        | cbase | tasks | part  | slots
//   sample     cent, shot0, rows, bad (zeros)  | cbase | tasks |       | slots     (no partial sums: width 0)
//   amplitude  cent, str0, rows                | cbase | tasks |       | slots
//   window     cent, cwin                      | cbase | tasks | part  | slots
//   MPO        cent, cstr (the MPO)            | cbase | tasks | part  | slots
// A column holds `per` elements of `elem` bytes per chain; src points at the element of chain 0 of the whole list (a range takes
// its own part), NULL: the column is staged as zeros (the device writes it).
struct ChainCol {
  const void* src;
  size_t elem, per;
};
struct ChainStage {
  std::vector<size_t> col;    // byte offset of every column, then of the slot bases
  size_t tasks = 0, part = 0, slots = 0, total = 0;  // byte offsets; part is also the size of the table part, total the end of the slots
  std::vector<int64_t> cbase;  // chain of the range -> first double of its slot
  std::vector<char> image;     // host image of the table part, pad bytes zero: alive until the stream has taken it
};
// the offsets of the chains [c0, c1), `width` doubles of partial sums per chain; returns the total
inline size_t chain_offsets(const std::vector<ChainCol>& cols, const ChainCore& c, const size_t c0, const size_t c1, const long long width, ChainStage& st) {
  const size_t nc = c1 - c0;
  long long nt = 0, sl = 0;
  for (size_t e = c0; e < c1; ++e) nt += c.ntasks[e], sl += c.slot[e];
  st.col.clear();
  size_t at = 0;
  for (const ChainCol& k : cols) st.col.push_back(at), at += al256(nc * k.per * k.elem);
  st.col.push_back(at), at += al256(nc * sizeof(int64_t));
  st.tasks = at, at += al256((size_t)nt * sizeof(Task2));
  st.part = at, at += al256(nc * (size_t)width * sizeof(double));
  st.slots = at;
  return st.total = at + (size_t)sl * sizeof(double);
}
// offsets, slot bases and the filled image of the chains [c0, c1) with their task list
inline void chain_stage(const std::vector<ChainCol>& cols, const ChainCore& c, const size_t c0, const size_t c1, const long long width, const std::vector<Task2>& tasks, ChainStage& st) {
  chain_offsets(cols, c, c0, c1, width, st);
  const size_t nc = c1 - c0;
  st.cbase.resize(nc);
  long long sl = 0;
  for (size_t e = 0; e < nc; ++e) st.cbase[e] = sl, sl += c.slot[c0 + e];
  st.image.assign(st.part, 0);
  auto put = [&](const size_t at, const void* src, const size_t bytes) {
    if (bytes) std::memcpy(st.image.data() + at, src, bytes);
  };
  for (size_t k = 0; k < cols.size(); ++k)
    if (cols[k].src) put(st.col[k], static_cast<const char*>(cols[k].src) + c0 * cols[k].per * cols[k].elem, nc * cols[k].per * cols[k].elem);
  put(st.col[cols.size()], st.cbase.data(), nc * sizeof(int64_t));
  put(st.tasks, tasks.data(), std::min(tasks.size() * sizeof(Task2), st.part - st.tasks));  // the lists hold the chains' ntasks tasks (tested on the CPU)
}
// the largest total over the chain batches of a cut (cstart of chain_cut): what a state batch's buffer must have behind its own part
inline size_t chain_stage_max(const std::vector<ChainCol>& cols, const ChainCore& c, const std::vector<size_t>& cstart, const long long width) {
  ChainStage st;
  size_t most = 0;
  for (size_t cb = 0; cb + 1 < cstart.size(); ++cb) most = std::max(most, chain_offsets(cols, c, cstart[cb], cstart[cb + 1], width, st));
  return most;
}
// The chains (pairs, strings) of a batch at most, from the environment: unset gives 0, the memory rule alone.
inline int batch_cap(const char* what, const char* variable, long long& cap) {
  cap = 0;
  if (const char* v = std::getenv(variable)) {
    cap = std::atoll(v);
    if (cap < 1) return qk_fail(QK_EINVAL, "%s: %s must be >= 1 (got \"%s\")", what, variable, v);
  }
  return QK_OK;
}

// ---- the pair chains of the block kernels (qk_block_values_host) ------------------------------------------------------------------
// side 0 (left): the block is qubits 0 .. w-1; step j takes site j, enters by bond j and leaves by bond j + 1.  side 1 (right): the
// block is qubits n-w .. n-1; step j takes site n-1-j of the reversed image, enters by bond n - j and leaves by bond n-1-j.  After
// step j the chain's E is the mixed environment at the bond it left by: the cut of width j + 1.
QK_HD constexpr int blk_site(const int side, const int j, const int n) { return side ? n - 1 - j : j; }
QK_HD constexpr int blk_in(const int side, const int j, const int n) { return side ? n - j : j; }
QK_HD constexpr int blk_out(const int side, const int j, const int n) { return side ? n - 1 - j : j + 1; }
QK_HD constexpr int blk_cut_bond(const int side, const int width, const int n) { return side ? n - width : width; }
// A pair chain is one (x state i, y state j); its slot is the string chain's, P = max(P_x, P_y): E [pad_y x pad_x] at chain_E()
// (ld = the padded x bond) | T [pad_x x 2 pad_y] at chain_T().  Between two sites T is dead, so the products of a cut live there:
// V [pad_y x pad_x] at blk_V() and W [pad_x x pad_x] at blk_W(), each a re plane then an im plane of P^2.
QK_HD constexpr int blk_V() { return chain_T(); }
QK_HD constexpr int blk_W() { return chain_T() + 2; }
static_assert(blk_V() >= chain_T() && blk_W() + 2 <= chain_size() && blk_V() + 2 <= blk_W(), "V and W lie inside T and do not overlap");

// the blocks of a pair chain (px, py = the padded bonds [n + 1] of its two states) in the launch `kind` of step j
inline int blk_task_count(const int kind, const int side, const int j, const int32_t* px, const int32_t* py, const int n) {
  const int in = blk_in(side, j, n), out = blk_out(side, j, n);
  switch (kind) {
    case BLK_T: return (int)blocks64(px[in], 2ll * py[out]);
    case BLK_X: case BLK_V: return (int)blocks64(py[out], px[out]);
    case BLK_W: return (int)blocks64(px[out], px[out]);
    default: return px[out] / LOC_CHUNK;  // BLK_RED
  }
}
struct BlkLaunch {
  int kind, step, cut;  // cut: index into the width list (BLK_V, BLK_W, BLK_RED), else -1
};
// The launches of a pair batch in stream order: per step T and X, and behind the step whose width was asked for V, W and the
// reduction.  The chain stops at the largest width: 2 widths[n_widths - 1] + 3 n_widths launches.
inline std::vector<BlkLaunch> blk_plan(const int n_widths, const int32_t* widths) {
  std::vector<BlkLaunch> plan;
  int ci = 0;
  for (int j = 0; ci < n_widths; ++j) {
    plan.push_back({BLK_T, j, -1}), plan.push_back({BLK_X, j, -1});
    if (widths[ci] == j + 1) {
      plan.push_back({BLK_V, j, ci}), plan.push_back({BLK_W, j, ci}), plan.push_back({BLK_RED, j, ci});
      ++ci;
    }
  }
  return plan;
}
// widths must be strictly increasing in 1 .. n: returns -1, or the index of the first offender
inline int blk_bad_width(const int n_widths, const int32_t* widths, const int n) {
  for (int i = 0; i < n_widths; ++i)
    if (widths[i] < 1 || widths[i] > n || (i > 0 && widths[i] <= widths[i - 1])) return i;
  return -1;
}

// The kept environments: a compact buffer of doubles that starts with the 16 x 16 unit matrix (blk_kept_unit() doubles: E of a
// chain before its first step), then for every state of a set and every chosen cut, state-major in width order, the self environment
// of the cut (R of the bond, or L for side 1), pad^2 per plane.  koff[s * n_widths + ci] = its first double.  `at` = where the
// set's environments start; returns where they end.
constexpr long long blk_kept_unit() { return 2 * 16 * 16; }
inline long long blk_kept_offsets(const EnvSizes& z, const int side, const int n_widths, const int32_t* widths, long long at, std::vector<int64_t>& koff) {
  const int n = z.n_sites;
  koff.resize((size_t)z.n_states * n_widths);
  for (int s = 0; s < z.n_states; ++s)
    for (int ci = 0; ci < n_widths; ++ci) {
      const long long d = z.pad[(size_t)s * (n + 1) + blk_cut_bond(side, widths[ci], n)];
      koff[(size_t)s * n_widths + ci] = at;
      at += 2 * d * d;
    }
  return at;
}

using BlkChains = ChainCore;  // the pair chains of a call, in the order of its pair list
inline BlkChains list_blk_chains(const EnvSizes& zx, const EnvSizes& zy, const long long n_pairs, const int32_t* pairs, const int side,
                                 const std::vector<BlkLaunch>& plan, const int n_widths) {
  const int n = zx.n_sites, max_chunks = std::max(zx.max_chunks, zy.max_chunks);
  BlkChains c;
  c.slot.resize(n_pairs), c.ntasks.resize(n_pairs), c.weight.resize(n_pairs);
  for (long long e = 0; e < n_pairs; ++e) {
    const int i = pairs[2 * e], j = pairs[2 * e + 1];
    const long long P = std::max(zx.pmax[i], zy.pmax[j]);
    long long nt = 0;
    for (const BlkLaunch& l : plan) nt += blk_task_count(l.kind, side, l.step, &zx.pad[(size_t)i * (n + 1)], &zy.pad[(size_t)j * (n + 1)], n);
    c.slot[e] = chain_size() * P * P, c.ntasks[e] = nt;
    c.weight[e] = c.slot[e] + (long long)n_widths * max_chunks + nt + 4;
  }
  return c;
}
// Task lists (chain of the batch, block) of the pair chains [c0, c0 + nc) for every launch of `plan`
inline void blk_lists(const EnvSizes& zx, const EnvSizes& zy, const int32_t* pairs, const size_t c0, const size_t nc, const int side, const std::vector<BlkLaunch>& plan,
                      std::vector<Task2>& tasks, std::vector<long long>& first) {
  const int n = zx.n_sites;
  tasks.clear(), first.clear();
  for (const BlkLaunch& l : plan) {
    first.push_back((long long)tasks.size());
    for (size_t e = 0; e < nc; ++e) {
      const int i = pairs[2 * (c0 + e)], j = pairs[2 * (c0 + e) + 1];
      const int nbk = blk_task_count(l.kind, side, l.step, &zx.pad[(size_t)i * (n + 1)], &zy.pad[(size_t)j * (n + 1)], n);
      for (int b = 0; b < nbk; ++b) tasks.push_back(Task2{(int)e, b});
    }
  }
  first.push_back((long long)tasks.size());
}

// ---- measurement shots (qk_sample_host) -----------------------------------------------------------------------------------------
// Philox4x32-10, counter (site, shot, global state index, stream), key = the two halves of the seed.  Stream 0 draws outcomes,
// stream 1 the random bases.  The device and the host mirror run this text, so they agree bit for bit.
struct Philox4 {
  uint32_t x[4];
};
QK_HD inline Philox4 smp_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    if (r > 0) k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
  }
  return Philox4{{c0, c1, c2, c3}};
}
// the uniform of (seed, state, shot, site) in [0, 1): 53 bits from the first two words
QK_HD inline double smp_uniform(const uint64_t seed, const uint32_t state, const uint32_t shot, const uint32_t site) {
  const Philox4 r = smp_philox(site, shot, state, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (double)(((uint64_t)(r.x[0] >> 5) << 26) + (uint64_t)(r.x[1] >> 6)) * (1.0 / 9007199254740992.0);
}

// A shot chain is one (state, shot tile): `tile` = 16 m consecutive shots of a state, the last tile of a state ragged.  Its rows
// are padded to R = a multiple of 16 and its slot is smp_size() P R doubles, P = the state's largest padded bond, every matrix as a
// re plane then an im plane, offsets in units of P R:
//   V  [P][R]   at smp_V()  = 0   the row vectors of the shots, K-major (bond index first): the A operand of SMP_W, ld = R
//   W  [R][2P]  at smp_W()  = 2   (W_0 | W_1) of the rows, ld = 2 pad_{k+1}
//   W' [P][2R]  at smp_Ws() = 6   the stacked operand [W'_0 ; W'_1], K-major: the A operand of SMP_Q, ld = 2 R
//   Q  [2R][P]  at smp_Q()  = 10  ld = pad_{k+1}
constexpr int SMP_TILE = 64;  // shots per tile (m = 4): one 64-row block of the ring GEMM
QK_HD constexpr int smp_rows_pad(const int rows) { return (rows + LOC_CHUNK - 1) / LOC_CHUNK * LOC_CHUNK; }
QK_HD constexpr int smp_V() { return 0; }
QK_HD constexpr int smp_W() { return 2; }
QK_HD constexpr int smp_Ws() { return 6; }
QK_HD constexpr int smp_Q() { return 10; }
QK_HD constexpr int smp_size() { return 14; }
inline int smp_tiles(const int n_shots, const int tile) { return (n_shots + tile - 1) / tile; }
// the environment pass of a sampling call: the reversed chain alone, every R_k kept (env_sizes with keep_l = false)
inline Plan sample_env_plan(const int n) {
  Plan plan;
  plan_reverse(n, plan);
  return plan;
}
constexpr int SMP_KINDS[4] = {SMP_W, SMP_ROT, SMP_Q, SMP_DRAW};  // the launches of a site, in stream order
// the blocks of a shot chain of R padded rows (p = its state's padded bonds) in the launch `kind` of site k
inline int smp_task_count(const int kind, const int k, const int32_t* p, const int R) {
  switch (kind) {
    case SMP_W: return (int)blocks64(R, 2ll * p[k + 1]);
    case SMP_Q: return (int)blocks64(2ll * R, p[k + 1]);
    default: return R / LOC_CHUNK;  // SMP_ROT, SMP_DRAW
  }
}
struct SmpChains : ChainCore {  // the shot chains of a state batch, state-major in shot order
  std::vector<int32_t> cent, shot0, rows;  // chain -> batch entry, first shot, shots
};
inline SmpChains list_smp_chains(const EnvSizes& z, const int s0, const int nb, const int n_shots, const int tile) {
  const int n = z.n_sites;
  SmpChains c;
  for (int i = 0; i < nb; ++i)
    for (int t = 0; t < smp_tiles(n_shots, tile); ++t) {
      const int rows = std::min(tile, n_shots - t * tile), R = smp_rows_pad(rows);
      long long nt = 0;
      for (int k = 0; k < n; ++k)
        for (const int kind : SMP_KINDS) nt += smp_task_count(kind, k, &z.pad[(size_t)(s0 + i) * (n + 1)], R);
      c.cent.push_back(i), c.shot0.push_back(t * tile), c.rows.push_back(rows);
      c.slot.push_back((long long)smp_size() * z.pmax[s0 + i] * R), c.ntasks.push_back(nt);
      c.weight.push_back(c.slot.back() + nt + 4);
    }
  return c;
}
// Task lists (chain of the batch, block) of the shot chains [c0, c0 + nc): launch 4k + j is SMP_KINDS[j] at site k.  The cut into
// chain batches is chain_cut (QK_SAMPLE_BATCH caps the chains of one).
inline void smp_lists(const EnvSizes& z, const int s0, const SmpChains& c, const size_t c0, const size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) {
  const int n = z.n_sites;
  tasks.clear(), first.clear();
  for (int k = 0; k < n; ++k)
    for (const int kind : SMP_KINDS) {
      first.push_back((long long)tasks.size());
      for (size_t e = 0; e < nc; ++e) {
        const int nbk = smp_task_count(kind, k, &z.pad[(size_t)(s0 + c.cent[c0 + e]) * (n + 1)], smp_rows_pad(c.rows[c0 + e]));
        for (int b = 0; b < nbk; ++b) tasks.push_back(Task2{(int)e, b});
      }
    }
  first.push_back((long long)tasks.size());
}
// the first basis code outside 1..3 = X, Y, Z: its index, or -1
inline long long smp_bad_basis(const uint8_t* bases, const long long count) {
  for (long long e = 0; e < count; ++e)
    if (bases[e] < 1 || bases[e] > 3) return e;
  return -1;
}

// ---- amplitudes of given strings (qk_amplitudes_host) -------------------------------------------------------------------------------
// An amplitude chain is one (state, string tile): `tile` = 16 m consecutive strings of the call, the last tile ragged, rows padded
// to R as a shot chain's.  It needs no right environment and no draw, so its slot is amp_size() P R doubles, every matrix as a re
// plane then an im plane, offsets in units of P R:
//   V  [P][R]   at amp_V() = 0   the row vectors of the strings, K-major: the A operand of AMP_W, ld = R
//   W  [R][2P]  at amp_W() = 2   (W_0 | W_1) of the rows, ld = 2 pad_{k+1}
// The chains of a state batch are an SmpChains (shot0 = the chain's first string), cut by chain_cut (QK_AMP_BATCH caps the chains of
// a batch).
constexpr int AMP_TILE = SMP_TILE;  // strings per tile: one 64-row block of the ring GEMM
QK_HD constexpr int amp_V() { return 0; }
QK_HD constexpr int amp_W() { return 2; }
QK_HD constexpr int amp_size() { return 6; }
static_assert(amp_W() >= amp_V() + 2 && amp_size() >= amp_W() + 4, "V (2 planes of P R) and W (2 planes of 2 P R) do not overlap");
constexpr int AMP_KINDS[2] = {AMP_W, AMP_PICK};  // the launches of a site, in stream order
// the blocks of an amplitude chain of R padded rows (p = its state's padded bonds) in the launch `kind` of site k
inline int amp_task_count(const int kind, const int k, const int32_t* p, const int R) {
  return kind == AMP_W ? (int)blocks64(R, 2ll * p[k + 1]) : R / LOC_CHUNK;
}
// launches of a chain batch: the init kernel, then AMP_KINDS at every site
inline int amp_launches(const int n) { return 2 * n + 1; }
inline SmpChains list_amp_chains(const EnvSizes& z, const int s0, const int nb, const int n_strings, const int tile) {
  const int n = z.n_sites;
  SmpChains c;
  for (int i = 0; i < nb; ++i)
    for (int t = 0; t < smp_tiles(n_strings, tile); ++t) {
      const int rows = std::min(tile, n_strings - t * tile), R = smp_rows_pad(rows);
      long long nt = 0;
      for (int k = 0; k < n; ++k)
        for (const int kind : AMP_KINDS) nt += amp_task_count(kind, k, &z.pad[(size_t)(s0 + i) * (n + 1)], R);
      c.cent.push_back(i), c.shot0.push_back(t * tile), c.rows.push_back(rows);
      c.slot.push_back((long long)amp_size() * z.pmax[s0 + i] * R), c.ntasks.push_back(nt);
      c.weight.push_back(c.slot.back() + nt + 4);
    }
  return c;
}
// Task lists (chain of the batch, block) of the amplitude chains [c0, c0 + nc): launch 2k + j is AMP_KINDS[j] at site k.
inline void amp_lists(const EnvSizes& z, const int s0, const SmpChains& c, const size_t c0, const size_t nc, std::vector<Task2>& tasks, std::vector<long long>& first) {
  const int n = z.n_sites;
  tasks.clear(), first.clear();
  for (int k = 0; k < n; ++k)
    for (const int kind : AMP_KINDS) {
      first.push_back((long long)tasks.size());
      for (size_t e = 0; e < nc; ++e) {
        const int nbk = amp_task_count(kind, k, &z.pad[(size_t)(s0 + c.cent[c0 + e]) * (n + 1)], smp_rows_pad(c.rows[c0 + e]));
        for (int b = 0; b < nbk; ++b) tasks.push_back(Task2{(int)e, b});
      }
    }
  first.push_back((long long)tasks.size());
}
// the first byte of an outcome table that is neither 0 nor 1: its index, or -1
inline long long amp_bad_bit(const uint8_t* bits, const long long count) {
  for (long long e = 0; e < count; ++e)
    if (bits[e] > 1) return e;
  return -1;
}
// log of |v 2^E|^2 / <psi|psi> from the mantissa v = (re, im), the exponent E and log <psi|psi>: -inf for a zero amplitude
inline double amp_logp(const double re, const double im, const int32_t E, const double log_norm) {
  const double a = std::hypot(re, im);
  return a == 0.0 ? -std::numeric_limits<double>::infinity() : 2.0 * (std::log(a) + E * 0.69314718055994530942) - log_norm;
}

// ---- windows of k qubits (qk_window_rdms_host) ------------------------------------------------------------------------------------
// A window chain is one (state, window): the qubits a .. a+w-1 of the state, b = a + w, 1 <= w <= WIN_MAX_WIDTH.  The product of its
// sites grows from the right, the new site's physical index most significant, from two seeds (definitions in qk_local.hip):
// G_j, Gr_j [pad_{b-j}][2^j pad_b].  Its slot is win_size() U doubles, U = 2^w P^2 (P = the state's largest padded bond), every
// matrix as a re plane then an im plane of U, offsets in units of U:
//   G_j  at win_G(j)  = 0 | 2 (j even | odd), ld = 2^j pad_b; G_0 is never stored and G_1 is the site b-1 itself, read from the set
//   Gr_j at win_Gr(j) = 4 | 6, ld = 2^j pad_b; Gr_0 = R_b is read from the kept environments
//   H    at win_H(w)  = the G buffer that G_w does not lie in (G_{w-1} is dead once G_w exists), ld = 2^w pad_b
// A step reads the buffer of one parity and writes the other, so no block of a launch reads what another block of it writes.
constexpr int WIN_MAX_WIDTH = 6;
QK_HD constexpr int win_dim(const int w) { return 1 << w; }
QK_HD constexpr int win_G(const int j) { return 2 * (j & 1); }
QK_HD constexpr int win_Gr(const int j) { return 4 + 2 * (j & 1); }
QK_HD constexpr int win_H(const int w) { return win_G(w + 1); }
QK_HD constexpr int win_size() { return 8; }
QK_HD constexpr long long win_unit(const long long P, const int w) { return (P * P) << w; }
// The closing sums of a chain: (Re, Im) of rho[s][s'] for every s <= s', pairs row-major, win_pairs(w) of them.
QK_HD constexpr int win_pairs(const int w) { return win_dim(w) * (win_dim(w) + 1) / 2; }
QK_HD constexpr int win_vals(const int w) { return 2 * win_pairs(w); }
QK_HD constexpr int win_pair(const int s, const int sp, const int w) { return s * win_dim(w) - s * (s - 1) / 2 + (sp - s); }  // s <= sp
QK_HD inline void win_pair_of(int p, const int w, int& s, int& sp) {
  const int D = win_dim(w);
  for (s = 0; p >= D - s; ++s) p -= D - s;
  sp = s + p;
}
constexpr int WIN_CLOSE_GROUP = 16;  // pairs a workgroup of the closing kernel takes at a time (16 lanes each)
// the width must be in 1 .. min(n, WIN_MAX_WIDTH)
inline bool win_bad_width(const int w, const int n) { return w < 1 || w > n || w > WIN_MAX_WIDTH; }
// starts must be strictly increasing in 0 .. n - w: returns -1, or the index of the first offender
inline int win_bad_start(const int n_starts, const int32_t* starts, const int n, const int w) {
  for (int i = 0; i < n_starts; ++i)
    if (starts[i] < 0 || starts[i] > n - w || (i > 0 && starts[i] <= starts[i - 1])) return i;
  return -1;
}
// The launches of a chain batch in stream order: the steps j = 0 .. w-1 (step 0 grows Gr alone), H, the closing sums.
inline Plan win_plan(const int w) {
  Plan plan;
  for (int j = 0; j < w; ++j) plan.push_back({WIN_G, j});
  plan.push_back({WIN_H, 0}), plan.push_back({WIN_CLOSE, 0});
  return plan;
}
// the 64 x 64 blocks of one product of step j (one seed, one t): M = pad_c, N = 2^j pad_b
inline long long win_step_blocks(const int j, const int32_t* p, const int a, const int w) { return blocks64(p[a + w - 1 - j], (long long)p[a + w] << j); }
// The blocks of a window chain (p = its state's padded bonds) in the launch `kind` of step j.  WIN_G: block number = q per + block
// of the product, q = 2 seed + t, seed 0 = Gr, 1 = G (step 0 has seed 0 only).
inline int win_task_count(const int kind, const int j, const int32_t* p, const int a, const int w) {
  switch (kind) {
    case WIN_G: return (int)((j == 0 ? 2 : 4) * win_step_blocks(j, p, a, w));
    case WIN_H: return (int)blocks64(p[a], (long long)p[a + w] << w);
    default: return p[a] / LOC_CHUNK;  // WIN_CLOSE
  }
}
struct WinChains : ChainCore {  // the window chains of a state batch, state-major in window order
  std::vector<int32_t> cent, cwin;  // chain -> batch entry, window (index into the starts)
};
inline WinChains list_win_chains(const EnvSizes& z, const int s0, const int nb, const int w, const int n_windows, const int32_t* starts) {
  const int n = z.n_sites;
  const Plan plan = win_plan(w);
  WinChains c;
  for (int i = 0; i < nb; ++i)
    for (int m = 0; m < n_windows; ++m) {
      long long nt = 0;
      for (const auto& [kind, j] : plan) nt += win_task_count(kind, j, &z.pad[(size_t)(s0 + i) * (n + 1)], starts[m], w);
      c.cent.push_back(i), c.cwin.push_back(m);
      c.slot.push_back(win_size() * win_unit(z.pmax[s0 + i], w)), c.ntasks.push_back(nt);
      c.weight.push_back(c.slot.back() + (long long)z.max_chunks * win_vals(w) + nt + 2);
    }
  return c;
}
// Task lists (chain of the batch, block) of the window chains [c0, c0 + nc) for every launch of win_plan(w).  The cut into chain
// batches is chain_cut (QK_WINDOW_BATCH caps the chains of one).
inline void win_lists(const EnvSizes& z, const int s0, const WinChains& c, const size_t c0, const size_t nc, const int w, const int32_t* starts,
                      std::vector<Task2>& tasks, std::vector<long long>& first) {
  const int n = z.n_sites;
  tasks.clear(), first.clear();
  for (const auto& [kind, j] : win_plan(w)) {
    first.push_back((long long)tasks.size());
    for (size_t e = 0; e < nc; ++e) {
      const int nbk = win_task_count(kind, j, &z.pad[(size_t)(s0 + c.cent[c0 + e]) * (n + 1)], starts[c.cwin[c0 + e]], w);
      for (int b = 0; b < nbk; ++b) tasks.push_back(Task2{(int)e, b});
    }
  }
  first.push_back((long long)tasks.size());
}

// ---- block overlaps from measurement shots (qk_shot_block_sums_host) -----------------------------------------------------------------
// U settings of M shots, shot u M + a in setting u; a shot's block bits are packed into one 32-bit word, and a pair's sums are
//     D_w(s, s') = popcount((s xor s') & mask(w)),   term_w = (-1)^D_w 2^(w - D_w),   S_u[w] = sum_{a, b < M} term_w(x[u M + a], y[u M + b])
// less M 2^w for a self pair (definitions in include/qkgram.h).  A task is one pair and a chunk of consecutive settings.
constexpr int SBK_MAX_WIDTH = 32;      // qubits of a packed word
constexpr int SBK_STAGE_WORDS = 4096;  // y words a workgroup stages in LDS at a time (16 KiB)
constexpr int SBK_MAX_CHUNK = 64;      // settings of a task: bounds the workgroup's table of per-setting wave sums
constexpr int SBK_GROUP = 8;           // widths of one launch
constexpr int SBK_LAUNCH_TASKS = 2048; // tasks of one launch: eight workgroups per CU, so no launch runs long on a shared device
QK_HD constexpr uint32_t sbk_mask(const int w) { return w >= 32 ? 0xffffffffu : (1u << w) - 1u; }  // (no shift by 32)
QK_HD constexpr long long sbk_term(const int D, const int w) { return (D & 1) ? -(1ll << (w - D)) : (1ll << (w - D)); }
// The kernel counts the agreeing bits A = w - D = popcount(~(s xor s') & mask(w)) and adds doubles built from E = 1023 + A alone:
// the high word (E << 20) | (E << 31) (low word 0) is the double (-1)^E 2^A = -(-1)^A 2^A, and term_w = sbk_agree_sign(w) times it.
QK_HD constexpr uint32_t sbk_agree_hi(const uint32_t E) { return E << 20 | E << 31; }
QK_HD constexpr int sbk_agree_sign(const int w) { return (w & 1) ? 1 : -1; }
QK_HD constexpr int sbk_round4(const int v) { return (v + 3) & ~3; }
// The packed word of a shot: bit k = bits[k] (side 0) or bits[n - 1 - k] (side 1), k < min(n, 32).  bad is set where a byte read
// is neither 0 nor 1.
QK_HD inline uint32_t sbk_pack(const uint8_t* bits, const int n, const int side, bool& bad) {
  uint32_t word = 0;
  const int nb = n < SBK_MAX_WIDTH ? n : SBK_MAX_WIDTH;
  for (int k = 0; k < nb; ++k) {
    const uint32_t b = bits[side ? n - 1 - k : k];
    if (b > 1) bad = true;
    word |= (b & 1u) << k;
  }
  return word;
}
// the overflow rule: U M^2 2^w_max <= 2^62, so that every sum and every partial sum fits an int64
inline bool sbk_fits(const long long U, const long long M, const int w_max) { return (unsigned __int128)U * M * M <= ((unsigned __int128)1 << (62 - w_max)); }
// widths must be strictly increasing in 1 .. min(n, 32): returns -1, or the index of the first offender
inline int sbk_bad_width(const int n_widths, const int32_t* widths, const int n) { return blk_bad_width(n_widths, widths, n < SBK_MAX_WIDTH ? n : SBK_MAX_WIDTH); }
// Settings per task: what the staged y words of a chunk (rows of M rounded up to 4 words; a longer row is staged in pieces, one
// setting at a time) and the table of wave sums allow, and no more than leaves about SBK_LAUNCH_TASKS tasks in the call.
inline int sbk_chunk(const int U, const int M, const long long n_pairs) {
  const long long lds = M >= SBK_STAGE_WORDS ? 1 : SBK_STAGE_WORDS / sbk_round4(M);
  const long long fill = std::max(1ll, (long long)U * n_pairs / SBK_LAUNCH_TASKS);
  return (int)std::max(1ll, std::min({lds, (long long)SBK_MAX_CHUNK, (long long)U, fill}));
}
QK_HD constexpr int sbk_n_chunks(const int U, const int chunk) { return (U + chunk - 1) / chunk; }
// task t of a pair batch: pair t / n_chunks of the batch and the settings [u0, u1)
QK_HD inline void sbk_task(const long long t, const int U, const int chunk, long long& pair, int& u0, int& u1) {
  const int nc = sbk_n_chunks(U, chunk);
  pair = t / nc;
  u0 = (int)(t % nc) * chunk;
  u1 = u0 + chunk < U ? u0 + chunk : U;
}
// The work of a wave inside a setting: the M x words in blocks of 64 (one per lane) times `parts` pieces of the staged y row, so that
// four waves have work when M is small.  Piece p of a row of bn words is [sbk_part_lo(p), sbk_part_lo(p + 1)), bounds in fours.
QK_HD constexpr int sbk_a_blocks(const int M) { return (M + 63) / 64; }
QK_HD constexpr int sbk_parts(const int M) { return sbk_a_blocks(M) == 1 ? 4 : sbk_a_blocks(M) == 2 ? 2 : 1; }
QK_HD constexpr int sbk_part_lo(const int p, const int parts, const int bn) {
  const int per = sbk_round4((bn + parts - 1) / parts);
  return p * per < bn ? p * per : bn;
}
// the widths of a call in launches of 8, 4, 2 or 1: the size of the group that starts at width index `at`
QK_HD constexpr int sbk_group(const int n_widths, const int at) {
  const int left = n_widths - at;
  return left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1;
}
// Pairs per batch: their per-setting sums [n_widths][pairs][U] (int64) and their pair entries within `room` bytes, at least one.
inline long long sbk_batch_pairs(const long long room, const int n_widths, const int U) {
  return std::max(1ll, room / ((long long)n_widths * U * 8 + 8));
}

// ---- the shadow kernel's shot-pair histograms (qk_shadow_hist_host) -------------------------------------------------------------------
// A shot is a record of three 32-bit planes per group of 32 qubits: bit k % 32 of group k / 32 holds the outcome bit (plane 0),
// code & 1 (plane 1) and code >> 1 (plane 2) of qubit k, codes 1, 2, 3 = X, Y, Z; pad bits are 0 in all planes.  Two shots enter the
// kernel through d = (qubits measured in the same basis with the same outcome) - (same basis, other outcome), and a pair of states
// through the histogram of d over all its shot pairs (definitions in include/qkgram.h).  A task is one pair and a range of blocks of
// 64 x shots (a block is what a wave holds in registers, one record per lane).
constexpr int SHK_MAX_QUBITS = 128;
constexpr int SHK_MAX_GROUPS = SHK_MAX_QUBITS / 32;
constexpr int SHK_BLOCK = 64;            // x shots of a block: one per lane of a wave
constexpr int SHK_STAGE_SHOTS = 256;     // y records a workgroup stages in LDS at a time
constexpr int SHK_LAUNCH_TASKS = 2048;   // tasks of one launch: eight workgroups per CU, so no launch runs long on a shared device
constexpr int SHK_LDS_BYTES = 160 * 1024;  // of a CU, and the most one workgroup may take
constexpr long long SHK_COUNTER_MAX = 0xffffffffll;  // a counter in LDS is 32 bits wide
constexpr long long SHK_SHARED_PAIRS = 1ll << 14;     // shot pairs of a pair of states up to which one histogram per wave is used
enum ShkLayout : int {
  SHK_PRIVATE = 0,  // counters [bin][thread]: every lane owns its counters, so an increment never meets another lane's
  SHK_SHARED = 1,   // counters [wave][bin]: one histogram per wave; lanes that meet in a bin are serialised by the LDS
};
QK_HD constexpr int shk_groups(const int n) { return (n + 31) / 32; }
QK_HD constexpr int shk_words(const int n) { return 3 * shk_groups(n); }                    // of a record in memory
QK_HD constexpr int shk_stride(const int groups) { return (3 * groups + 3) & ~3; }          // of a staged record in LDS: 16-byte reads
QK_HD constexpr int shk_bins(const int n) { return 2 * n + 1; }
// The record of a shot: rec[3 g + plane].  bad_bit / bad_code are set where a bit is not 0 or 1 / a code is not in 1 .. 3 (the
// offending entry contributes its low bits; the caller rejects the table).
QK_HD inline void shk_pack(const uint8_t* bits, const uint8_t* bases, const int n, uint32_t* rec, bool& bad_bit, bool& bad_code) {
  const int groups = shk_groups(n);
  for (int g = 0; g < groups; ++g) {
    uint32_t p0 = 0, p1 = 0, p2 = 0;
    const int k1 = n - 32 * g < 32 ? n - 32 * g : 32;
    for (int k = 0; k < k1; ++k) {
      const uint32_t b = bits[32 * g + k], c = bases[32 * g + k];
      if (b > 1) bad_bit = true;
      if (c < 1 || c > 3) bad_code = true;
      p0 |= (b & 1u) << k, p1 |= (c & 1u) << k, p2 |= ((c >> 1) & 1u) << k;
    }
    rec[3 * g] = p0, rec[3 * g + 1] = p1, rec[3 * g + 2] = p2;
  }
}
QK_HD inline int shk_popc(const uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}
// d of two records (strides sx, sy words between groups' planes: 3 in memory, and 3 in a staged record too): the one place it is defined.
//     eq = same basis on a measured qubit,   d = popcount(eq) - 2 popcount(eq & (outcomes differ))
QK_HD inline int shk_d(const uint32_t* x, const uint32_t* y, const int groups) {
  int same = 0, differ = 0;
  for (int g = 0; g < groups; ++g) {
    const uint32_t eq = ~((x[3 * g + 1] ^ y[3 * g + 1]) | (x[3 * g + 2] ^ y[3 * g + 2])) & (x[3 * g + 1] | x[3 * g + 2]);
    same += shk_popc(eq), differ += shk_popc(eq & (x[3 * g] ^ y[3 * g]));
  }
  return same - 2 * differ;
}
QK_HD constexpr int shk_x_blocks(const int shots_x) { return (shots_x - 1) / SHK_BLOCK + 1; }  // shots_x >= 1; no sum that could pass 2^31
// The LDS layout, a pure function of n and the shots.  Private counters cost a task bins x threads words to clear and as many to
// add up, whatever the shots; a histogram per wave costs bins words per wave but serialises the lanes that meet in a bin (d sits
// within a few sqrt(n) of 0, so most of a wave does).  So: shared while a pair of states has at most SHK_SHARED_PAIRS shot pairs --
// about what clearing and adding 256 private copies of a hundred bins costs -- and private beyond.
QK_HD constexpr ShkLayout shk_layout(const int /*n*/, const long long shots_x, const long long shots_y) {
  return shots_x * shots_y <= SHK_SHARED_PAIRS ? SHK_SHARED : SHK_PRIVATE;
}
QK_HD constexpr int shk_stage_bytes(const int n) { return SHK_STAGE_SHOTS * shk_stride(shk_groups(n)) * 4; }
// Waves of a workgroup: four, or as many (at least two at n = 128) as the private counters leave room for next to the staged records.
QK_HD constexpr int shk_waves(const int n, const ShkLayout layout) {
  if (layout == SHK_SHARED) return 4;
  const int fit = (SHK_LDS_BYTES - shk_stage_bytes(n)) / (shk_bins(n) * 64 * 4);
  return fit < 4 ? fit : 4;
}
// dynamic LDS of the histogram kernel: [staged y records | counters]
QK_HD constexpr int shk_lds_bytes(const int n, const ShkLayout layout) {
  return shk_stage_bytes(n) + shk_bins(n) * 4 * shk_waves(n, layout) * (layout == SHK_SHARED ? 1 : 64);
}
// The counter bound: the most x blocks a task may take so that no 32-bit counter passes SHK_COUNTER_MAX before the task adds its
// counters into int64.  A private counter takes at most one increment per (block of its wave, y shot); a wave's shared counter at
// most 64 per (block, y shot).  shots_y < 2^31, so one block always fits a private counter; a shared layout has at most
// SHK_SHARED_PAIRS increments in all.
QK_HD constexpr long long shk_max_blocks(const ShkLayout layout, const long long shots_y) {
  return SHK_COUNTER_MAX / (shots_y * (layout == SHK_SHARED ? SHK_BLOCK : 1));
}
// x blocks per task: all of a pair's when the call has pairs enough to fill launches, fewer when it has not, never more than the
// counter bound allows, at least one.
inline int shk_task_blocks(const ShkLayout layout, const int shots_x, const long long shots_y, const long long n_pairs) {
  const long long nxb = shk_x_blocks(shots_x);
  const long long fill = std::max(1ll, nxb * n_pairs / SHK_LAUNCH_TASKS);
  return (int)std::max(1ll, std::min({nxb, fill, shk_max_blocks(layout, shots_y)}));
}
QK_HD constexpr int shk_pair_tasks(const int shots_x, const int task_blocks) { return (shk_x_blocks(shots_x) + task_blocks - 1) / task_blocks; }
// task t of a pair batch: pair t / pair_tasks of the batch and the x blocks [b0, b1)
QK_HD inline void shk_task(const long long t, const int shots_x, const int task_blocks, long long& pair, int& b0, int& b1) {
  const int nt = shk_pair_tasks(shots_x, task_blocks), nxb = shk_x_blocks(shots_x);
  pair = t / nt;
  b0 = (int)(t % nt) * task_blocks;
  b1 = b0 + task_blocks < nxb ? b0 + task_blocks : nxb;
}
// A wave's units inside a staging pass: (x block of the task, piece of the bn staged records), pieces so that every wave has a unit
// when the task has fewer blocks than waves.
QK_HD constexpr int shk_parts(const int blocks, const int waves) { return blocks >= waves ? 1 : (waves + blocks - 1) / blocks; }
QK_HD constexpr int shk_part_lo(const int p, const int parts, const int bn) {
  const int per = (bn + parts - 1) / parts;
  return p * per < bn ? p * per : bn;
}
// Pairs per batch: per pair its entry (8 bytes), the per-task rows, the total row and the equal-shot row (bins int64 each) within
// `room` bytes, at least one.
inline long long shk_batch_pairs(const long long room, const int n, const int pair_tasks) {
  return std::max(1ll, room / (8 + (long long)(pair_tasks + 2) * shk_bins(n) * 8));
}

// ---- Pauli strings estimated from shots (qk_shot_strings_host) -----------------------------------------------------------------------
// The shots are the records of the shadow kernel (shk_pack).  A Pauli string is a record of two planes per group of 32 qubits:
// rec[2 g] = s1 (code & 1), rec[2 g + 1] = s2 (code >> 1), codes 0 .. 3 = I, X, Y, Z; I and the pad bits are 0 in both, so
// supp = s1 | s2 is the support.  A shot matches a string when its basis equals the string's code on every qubit of the support; its
// sign is the parity of its outcome bits there (definitions in include/qkgram.h).  A task is one state, one block of 64 strings (a
// string per lane of a wave) and a range of chunks of SST_STAGE_SHOTS shots (a chunk is what a workgroup stages in LDS at a time).
constexpr int SST_BLOCK = 64;            // strings of a block: one per lane of a wave
constexpr int SST_STAGE_SHOTS = 256;     // shot records a workgroup stages in LDS at a time: a chunk
constexpr int SST_LAUNCH_TASKS = 2048;   // tasks of one launch, as SHK_LAUNCH_TASKS: no launch runs long on a shared device
constexpr int SST_ROW = 2 * SST_BLOCK;   // int32 of a task's row: the 64 partial sums, then the 64 partial counts
constexpr long long SST_PARTIAL_MAX = 0x7fffffffll;  // a partial sum or count is an int32
QK_HD constexpr int sst_words(const int n) { return 2 * shk_groups(n); }  // of a string record
// The record of a string; bad is set where a code is above 3 (it contributes its low bits; the caller rejects the table).
QK_HD inline void sst_pack_string(const uint8_t* codes, const int n, uint32_t* rec, bool& bad) {
  const int groups = shk_groups(n);
  for (int g = 0; g < groups; ++g) {
    uint32_t s1 = 0, s2 = 0;
    const int k1 = n - 32 * g < 32 ? n - 32 * g : 32;
    for (int k = 0; k < k1; ++k) {
      const uint32_t c = codes[32 * g + k];
      if (c > 3) bad = true;
      s1 |= (c & 1u) << k, s2 |= ((c >> 1) & 1u) << k;
    }
    rec[2 * g] = s1, rec[2 * g + 1] = s2;
  }
}
// One (shot record, string record): the one place match and sign are defined.  miss collects the qubits of the support whose basis
// differs, odd the outcome bits on the support; the parity of a sum of popcounts is the parity of the XOR of the words.
//     match = (supp & ((s1 ^ p1) | (s2 ^ p2))) == 0 in every group,     sign = 1 - 2 (popcount(p0 & supp) summed over the groups & 1)
QK_HD inline void sst_test(const uint32_t* shot, const uint32_t* str, const int groups, bool& match, int& sign) {
  uint32_t miss = 0, odd = 0;
  for (int g = 0; g < groups; ++g) {
    const uint32_t supp = str[2 * g] | str[2 * g + 1];
    miss |= supp & ((str[2 * g] ^ shot[3 * g + 1]) | (str[2 * g + 1] ^ shot[3 * g + 2]));
    odd ^= shot[3 * g] & supp;
  }
  match = miss == 0;
  sign = 1 - 2 * (shk_popc(odd) & 1);
}
QK_HD constexpr int sst_blocks(const int n_strings) { return (n_strings - 1) / SST_BLOCK + 1; }    // n_strings >= 1
QK_HD constexpr int sst_chunks(const int shots) { return (shots - 1) / SST_STAGE_SHOTS + 1; }      // shots >= 1
// The overflow bound: a partial count is at most the shots of its task and a partial sum at most that in magnitude, so a task takes
// at most this many chunks.
QK_HD constexpr long long sst_max_chunks() { return SST_PARTIAL_MAX / SST_STAGE_SHOTS; }
// Chunks per task: all the shots when the call has (state, string block) units enough to fill launches, fewer when it has not, never
// more than the overflow bound allows, at least one.
inline int sst_task_chunks(const int shots, const long long units) {
  const long long nc = sst_chunks(shots);
  const long long fill = units >= SST_LAUNCH_TASKS ? nc : std::max(1ll, nc * units / SST_LAUNCH_TASKS);  // (no product that could pass 2^63)
  return (int)std::max(1ll, std::min({nc, fill, sst_max_chunks()}));
}
QK_HD constexpr int sst_ranges(const int shots, const int task_chunks) { return (sst_chunks(shots) + task_chunks - 1) / task_chunks; }
// task t of a batch of `blocks` string blocks: state t / (blocks ranges), then the block, then the range, its shots [t0, t1)
QK_HD inline void sst_task(const long long t, const int blocks, const int shots, const int task_chunks, long long& state, int& block, int& t0, int& t1) {
  const int ranges = sst_ranges(shots, task_chunks);
  const long long per = (long long)task_chunks * SST_STAGE_SHOTS, lo = (t % ranges) * per;
  state = t / ((long long)blocks * ranges);
  block = (int)((t / ranges) % blocks);
  t0 = (int)lo;
  t1 = (int)(lo + per < shots ? lo + per : shots);
}
// Strings per batch: per string its record, per state the task rows of its block (8 bytes of each row are the string's) and the two
// int64 totals, within `room` bytes; whole blocks when there is room for one, at least one string, at most `cap` when cap > 0.
inline long long sst_batch_strings(const long long room, const int n, const long long n_states, const int ranges, const long long cap) {
  long long fit = room / (4ll * sst_words(n) + n_states * (8ll * ranges + 16));
  if (fit >= SST_BLOCK) fit -= fit % SST_BLOCK;
  fit = std::max(1ll, fit);
  return cap > 0 ? std::min(fit, cap) : fit;
}

// ---- MPO observables (qk_mpo_expectations_host) -------------------------------------------------------------------------------------
// An MPO on n sites is n tensors W_k[u][v][s'][s] (complex, [w_k][w_{k+1}][2][2], w_0 = w_n = 1, 1 <= w_k <= MPO_MAX_BOND), packed
// MPO-major and site-major as (re, im) doubles.  Its support [a, b] is the hull of the sites whose tensor is not exactly the 1 x 1
// identity.  A chain is one (state, MPO) with a support; it starts from E_a = L_a and closes with R_{b+1} as a string chain does.
// Its slot is mpo_size() U doubles, U = w P^2 (w = the MPO's largest bond, P = the state's largest padded bond), every matrix as a
// re plane then an im plane, offsets in units of U:
//   E  [pad_k][w_k pad_k]         at mpo_E()  = 0   the planes E[u] side by side (column u pad_k), ld = w_k pad_k; the im plane lies
//                                                   w_k P^2 behind the re plane, so that of a closed chain (w = 1) lies where the
//                                                   closing kernel of the operator strings reads it
//   T  [w_k pad_k][2 pad_{k+1}]   at mpo_T()  = 2   the planes T[u] stacked (row u pad_k + a), ld = 2 pad_{k+1}; planes of 2 U
//   T' [w_{k+1} pad_k][2 pad_{k+1}] at mpo_Tp() = 6 the planes T'[v] stacked, as T
// Per (MPO, site) the host lists the blocks (u, v) whose four entries are not all exactly zero, sorted by v, then u; vfirst holds,
// per site with a mix launch, w_{k+1} + 1 block indices (the blocks of plane v are [vfirst[v], vfirst[v + 1])).
constexpr int MPO_MAX_BOND = 32;
QK_HD constexpr int mpo_E() { return 0; }
QK_HD constexpr int mpo_T() { return 2; }
QK_HD constexpr int mpo_Tp() { return 6; }
QK_HD constexpr int mpo_size() { return 10; }
QK_HD constexpr long long mpo_unit(const long long P, const int w) { return P * P * w; }
static_assert(mpo_T() >= mpo_E() + 2 && mpo_Tp() >= mpo_T() + 4 && mpo_size() >= mpo_Tp() + 4, "E (2 planes of U), T and T' (2 planes of 2 U each) do not overlap");
constexpr int MPO_KINDS[4] = {MPO_T, MPO_MIX, MPO_X, MPO_CLOSE};  // the launches of a site, in stream order

struct MpoPlan {
  int n_mpos = 0, n_sites = 0;
  std::vector<int32_t> bonds;   // [n_mpos][n_sites + 1]
  std::vector<int64_t> toff;    // [n_mpos][n_sites]: first double of W_k in the packed tensors
  std::vector<int32_t> supp;    // [n_mpos][2]: a, b (-1, -1: every tensor is the 1 x 1 identity)
  std::vector<int32_t> wmax;    // [n_mpos]: the largest bond
  std::vector<int32_t> vat;     // [n_mpos][n_sites]: where the site's w_{k+1} + 1 entries of vfirst start; -1: the exact 1 x 1 identity (no mix launch)
  std::vector<int32_t> vfirst;  // block indices
  std::vector<int32_t> blk_u, blk_v;  // per listed block (blk_v is host-only: the tests read it)
  std::vector<double> blk_w;    // per listed block: (re, im) of W[u][v][s'][s], s' major
};
// bonds must be in 1 .. MPO_MAX_BOND: returns -1, or the index m (n + 1) + k of the first offender
inline long long mpo_bad_bond(const int32_t* bonds, const int n_mpos, const int n) {
  for (long long e = 0; e < (long long)n_mpos * (n + 1); ++e)
    if (bonds[e] < 1 || bonds[e] > MPO_MAX_BOND) return e;
  return -1;
}
// the doubles of the packed tensors of valid bonds
inline long long mpo_doubles(const int32_t* bonds, const int n_mpos, const int n) {
  long long tot = 0;
  for (int m = 0; m < n_mpos; ++m)
    for (int k = 0; k < n; ++k) tot += 8ll * bonds[(size_t)m * (n + 1) + k] * bonds[(size_t)m * (n + 1) + k + 1];
  return tot;
}
inline bool mpo_is_identity(const double* w, const int wl, const int wr) {
  return wl == 1 && wr == 1 && w[0] == 1.0 && w[1] == 0.0 && w[2] == 0.0 && w[3] == 0.0 && w[4] == 0.0 && w[5] == 0.0 && w[6] == 1.0 && w[7] == 0.0;
}
// supports, block lists and bond maxima of MPOs with valid bonds
inline MpoPlan mpo_plan(const int32_t* bonds, const double* tensors, const int n_mpos, const int n) {
  MpoPlan mp;
  mp.n_mpos = n_mpos, mp.n_sites = n;
  mp.bonds.assign(bonds, bonds + (size_t)n_mpos * (n + 1));
  mp.toff.resize((size_t)n_mpos * n), mp.supp.assign((size_t)2 * n_mpos, -1), mp.wmax.assign(n_mpos, 1), mp.vat.assign((size_t)n_mpos * n, -1);
  long long at = 0;
  for (int m = 0; m < n_mpos; ++m)
    for (int k = 0; k < n; ++k) {
      const int wl = bonds[(size_t)m * (n + 1) + k], wr = bonds[(size_t)m * (n + 1) + k + 1];
      const double* w = tensors + at;
      mp.toff[(size_t)m * n + k] = at, at += 8ll * wl * wr;
      mp.wmax[m] = std::max({mp.wmax[m], wl, wr});
      if (mpo_is_identity(w, wl, wr)) continue;
      if (mp.supp[2 * m] < 0) mp.supp[2 * m] = k;
      mp.supp[2 * m + 1] = k;
      mp.vat[(size_t)m * n + k] = (int32_t)mp.vfirst.size();
      for (int v = 0; v < wr; ++v) {
        mp.vfirst.push_back((int32_t)mp.blk_u.size());
        for (int u = 0; u < wl; ++u) {
          const double* b = w + 8 * ((size_t)u * wr + v);
          bool zero = true;
          for (int e = 0; e < 8; ++e) zero = zero && b[e] == 0.0;
          if (zero) continue;
          mp.blk_u.push_back(u), mp.blk_v.push_back(v);
          mp.blk_w.insert(mp.blk_w.end(), b, b + 8);
        }
      }
      mp.vfirst.push_back((int32_t)mp.blk_u.size());
    }
  return mp;
}
// the blocks of a chain (p = its state's padded bonds, m = its MPO) in the launch `kind` of site k
inline int mpo_task_count(const int kind, const int k, const int32_t* p, const MpoPlan& mp, const int m) {
  const int n = mp.n_sites, a = mp.supp[2 * m], b = mp.supp[2 * m + 1];
  if (a < 0 || k < a || k > b) return 0;
  const int wl = mp.bonds[(size_t)m * (n + 1) + k], wr = mp.bonds[(size_t)m * (n + 1) + k + 1];
  switch (kind) {
    case MPO_T: return (int)blocks64((long long)wl * p[k], 2ll * p[k + 1]);
    case MPO_MIX: return mp.vat[(size_t)m * n + k] < 0 ? 0 : wr * (p[k] / LOC_CHUNK);
    case MPO_X: return (int)(wr * blocks64(p[k + 1], p[k + 1]));
    default: return k == b ? p[k + 1] / LOC_CHUNK : 0;  // MPO_CLOSE
  }
}
// the chains of a state batch, state-major in MPO order (cstr = the MPO); a chunk sum is (Re, Im)
inline Chains list_mpo_chains(const EnvSizes& z, const int s0, const int nb, const MpoPlan& mp) {
  const int n = z.n_sites;
  Chains c;
  for (int i = 0; i < nb; ++i)
    for (int m = 0; m < mp.n_mpos; ++m)
      if (mp.supp[2 * m] >= 0) {
        long long nt = 0;
        for (int k = mp.supp[2 * m]; k <= mp.supp[2 * m + 1]; ++k)
          for (const int kind : MPO_KINDS) nt += mpo_task_count(kind, k, &z.pad[(size_t)(s0 + i) * (n + 1)], mp, m);
        c.cent.push_back(i), c.cstr.push_back(m), c.ntasks.push_back(nt);
        c.slot.push_back(mpo_size() * mpo_unit(z.pmax[s0 + i], mp.wmax[m]));
        c.weight.push_back(c.slot.back() + 2ll * z.max_chunks + nt + 2);
      }
  return c;
}
// Task lists (chain of the batch, block) of the chains [c0, c0 + nc): launch 4k + j is MPO_KINDS[j] at site k.  The cut into chain
// batches is chain_cut (QK_MPO_BATCH caps the chains of one).
inline void mpo_lists(const EnvSizes& z, const int s0, const Chains& c, const size_t c0, const size_t nc, const MpoPlan& mp, std::vector<Task2>& tasks, std::vector<long long>& first) {
  const int n = z.n_sites;
  tasks.clear(), first.clear();
  for (int k = 0; k < n; ++k)
    for (const int kind : MPO_KINDS) {
      first.push_back((long long)tasks.size());
      for (size_t e = 0; e < nc; ++e) {
        const int nbk = mpo_task_count(kind, k, &z.pad[(size_t)(s0 + c.cent[c0 + e]) * (n + 1)], mp, c.cstr[c0 + e]);
        for (int b = 0; b < nbk; ++b) tasks.push_back(Task2{(int)e, b});
      }
    }
  first.push_back((long long)tasks.size());
}

// ---- applying an MPO to a set (qk_mps_set_apply_mpo) --------------------------------------------------------------------------------
// The product of one MPO (an MpoPlan of one MPO) with every state of a set: site k of a state with true bonds chi_k becomes
//     B_k[(u, a)][s'][(v, b)] = sum_s W_k[u][v][s'][s] A_k[a][s][b],   row u chi_k + a, column v chi_{k+1} + b
// with true bonds w_k chi_k, each padded to a multiple of 16, in the split-plane layout of a set, states and sites in order without
// gaps (the layout qk_mps_set_create makes).  A product bond above APPLY_MAX_BOND is refused: bad_state / bad_bond name the first
// one and no table is made.  Per site the listed blocks of mpo_plan are listed again by row: the blocks of row u are
// [ufirst[uat[k] + u], ufirst[uat[k] + u + 1]) in ascending v; a site that is the exact 1 x 1 identity is marked in `copy` and
// keeps one block (0, 0) with the identity's entries.  A task is one (state, site, u, 16-row chunk of a): x = state n + site,
// y = u << 8 | chunk.  It writes its rows over the whole padded width -- the columns of a v without a block and the padding columns
// as zeros -- and the task of the last u and the last chunk also writes the padding rows, so the tasks of a call write every
// double of the new image exactly once.  Offsets and the total are 64-bit.
constexpr int APPLY_MAX_BOND = 512;  // SPEC_QMAX of the compress sweep and the limit of the fused Gram sweep: every consumer takes every product
struct ApplyPlan {
  int n_states = 0, n_sites = 0, max_pad = 0;
  int bad_state = -1, bad_bond = -1;  // the first w_k chi_k above APPLY_MAX_BOND
  long long total = 0;                // doubles of the new image
  long long read = 0;                 // doubles of the source the tasks read: every true element of a site once per u
  std::vector<int32_t> tru, pad;      // [n_states][n_sites + 1]: the new true and padded bonds
  std::vector<int64_t> offs;          // [n_states][n_sites]: re-plane offsets (doubles) in the new image
  std::vector<int32_t> copy;          // [n_sites]: 1 = W_k is the exact 1 x 1 identity (the site is copied bit for bit)
  std::vector<int32_t> uat;           // [n_sites]: where the site's w_k + 1 entries of ufirst start
  std::vector<int32_t> ufirst;        // block indices
  std::vector<int32_t> blk_u, blk_v;  // per listed block, by site, then u, then v (blk_u is host-only: the tests read it)
  std::vector<double> blk_w;          // per listed block: (re, im) of W[u][v][s'][s], s' major
  std::vector<Task2> tasks;
};
QK_HD constexpr int apply_task_u(const int y) { return y >> 8; }
QK_HD constexpr int apply_task_chunk(const int y) { return y & 255; }
inline ApplyPlan apply_plan(const int32_t* src_tru, const int ns, const int n, const MpoPlan& mp) {
  ApplyPlan ap;
  ap.n_states = ns, ap.n_sites = n;
  const int n1 = n + 1;
  const int32_t* w = mp.bonds.data();  // MPO 0
  for (int s = 0; s < ns && ap.bad_state < 0; ++s)
    for (int k = 0; k <= n; ++k)
      if ((long long)w[k] * src_tru[(size_t)s * n1 + k] > APPLY_MAX_BOND) {
        ap.bad_state = s, ap.bad_bond = k;
        break;
      }
  if (ap.bad_state >= 0) return ap;
  ap.tru.resize((size_t)ns * n1), ap.pad.resize((size_t)ns * n1), ap.offs.resize((size_t)ns * n);
  for (int s = 0; s < ns; ++s) {
    for (int k = 0; k <= n; ++k) {
      const int x = w[k] * src_tru[(size_t)s * n1 + k];
      ap.tru[(size_t)s * n1 + k] = x, ap.pad[(size_t)s * n1 + k] = qk_pad16(x);
      ap.max_pad = std::max(ap.max_pad, qk_pad16(x));
    }
    for (int k = 0; k < n; ++k) {
      ap.offs[(size_t)s * n + k] = ap.total;
      ap.total += 2ll * ap.pad[(size_t)s * n1 + k] * 2 * ap.pad[(size_t)s * n1 + k + 1];
      ap.read += 4ll * w[k] * src_tru[(size_t)s * n1 + k] * src_tru[(size_t)s * n1 + k + 1];
    }
  }
  ap.copy.assign(n, 0), ap.uat.resize(n);
  for (int k = 0; k < n; ++k) {
    ap.uat[k] = (int32_t)ap.ufirst.size();
    const int at = mp.vat[k];
    if (at < 0) {  // the exact 1 x 1 identity
      ap.copy[k] = 1;
      ap.ufirst.push_back((int32_t)ap.blk_v.size());
      ap.blk_u.push_back(0), ap.blk_v.push_back(0);
      const double eye[8] = {1, 0, 0, 0, 0, 0, 1, 0};
      ap.blk_w.insert(ap.blk_w.end(), eye, eye + 8);
    } else {
      for (int u = 0; u < w[k]; ++u) {
        ap.ufirst.push_back((int32_t)ap.blk_v.size());
        for (int v = 0; v < w[k + 1]; ++v)
          for (int j = mp.vfirst[at + v]; j < mp.vfirst[at + v + 1]; ++j)
            if (mp.blk_u[j] == u) {
              ap.blk_u.push_back(u), ap.blk_v.push_back(v);
              ap.blk_w.insert(ap.blk_w.end(), mp.blk_w.begin() + 8 * (size_t)j, mp.blk_w.begin() + 8 * (size_t)j + 8);
            }
      }
    }
    ap.ufirst.push_back((int32_t)ap.blk_v.size());
  }
  for (int s = 0; s < ns; ++s)
    for (int k = 0; k < n; ++k)
      for (int u = 0; u < w[k]; ++u)
        for (int c = 0; c < (src_tru[(size_t)s * n1 + k] + LOC_CHUNK - 1) / LOC_CHUNK; ++c) ap.tasks.push_back(Task2{s * n + k, u << 8 | c});
  return ap;
}

}  // namespace qkl
