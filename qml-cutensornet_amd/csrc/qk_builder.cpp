// qk_builder.cpp -- native host builder of the ansatz MPS: the same algorithm as
// qml-cutensornet_amd/mps.py:_simulate (one LAPACK gesdd per two-qubit gate, QR centre moves, ITensors-style cutoff),
// without the Python interpreter between the 10^3 ... 10^4 small LAPACK calls of a circuit.  Plain C++ (g++), no HIP:
// built as libqkbuilder.so next to libqkgram.so.  LAPACK/BLAS come from the OpenBLAS that scipy already ships
// (symbols scipy_zgesdd_, scipy_zgeqrf_, scipy_zungqr_, scipy_zgemm_), resolved at run time with dlopen: the Python
// side passes the library's path (qkb_init).  Reference semantics: gpu_backend/kernel_state_ansatz.py:141-144, 221
// (MPSxGate, truncation_fidelity) and KernelPkg.jl:68 (cutoff).
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using cd = std::complex<double>;

namespace {
thread_local std::string g_err;

// Fortran LAPACK / BLAS entry points (LP64 integers)
using zgesdd_t = void (*)(const char*, const int*, const int*, cd*, const int*, double*, cd*, const int*, cd*, const int*, cd*, const int*,
                          double*, int*, int*);
using zgeqrf_t = void (*)(const int*, const int*, cd*, const int*, cd*, cd*, const int*, int*);
using zungqr_t = void (*)(const int*, const int*, const int*, cd*, const int*, const cd*, cd*, const int*, int*);
using zgemm_t = void (*)(const char*, const char*, const int*, const int*, const int*, const cd*, const cd*, const int*, const cd*, const int*,
                         const cd*, cd*, const int*);
zgesdd_t p_zgesdd = nullptr;
zgeqrf_t p_zgeqrf = nullptr;
zungqr_t p_zungqr = nullptr;
zgemm_t p_zgemm = nullptr;

// ansatz.py.  Codes 8 and 9 are the matrix gates: valid only in a program that comes with a matrix table (N_OPS_MAT codes then).
// Code 10 is the one-qubit Kraus channel: valid only in a program that comes with a channel table; code 11 the two-qubit Kraus
// channel on (q0, q0+1): valid only in a program that comes with a two-qubit channel table.
enum { OP_H = 0, OP_RZ = 1, OP_XX = 2, OP_SWAP = 3, OP_RX = 4, OP_RY = 5, OP_YY = 6, OP_ZZ = 7, N_OPS = 8, OP_M1 = 8, OP_M2 = 9, N_OPS_MAT = 10, OP_K1 = 10, OP_K2 = 11 };

inline bool is_two_qubit(int o) { return o == OP_XX || o == OP_SWAP || o == OP_YY || o == OP_ZZ || o == OP_M2 || o == OP_K2; }

// sum_s m[s] t[s] over n terms in the fixed order of the matrix gates: column 0 first, ascending, the real and the imaginary part
// each one chain of fused multiply-adds (the device builder's mat_dot, qk_build_kernels.h, does the same arithmetic)
inline cd mat_dot(const cd* m, const cd* t, int n) {
  double re = m[0].real() * t[0].real(), im = m[0].real() * t[0].imag();
  re = std::fma(-m[0].imag(), t[0].imag(), re);
  im = std::fma(m[0].imag(), t[0].real(), im);
  for (int s = 1; s < n; ++s) {
    re = std::fma(m[s].real(), t[s].real(), re);
    re = std::fma(-m[s].imag(), t[s].imag(), re);
    im = std::fma(m[s].real(), t[s].imag(), im);
    im = std::fma(m[s].imag(), t[s].real(), im);
  }
  return cd(re, im);
}

// The matrix table of a program: every matrix gate's index inside 0..n_mats-1, its 2x2 ([:2][:2] of the slot) or 4x4 finite and
// unitary, max |M^H M - 1| <= 1e-12 (the canonical-form bookkeeping assumes unitary gates).  Empty string, or what is wrong.
std::string check_table(int n_ops, const int8_t* op, int n_mats, const cd* mats, const int32_t* mat) {
  for (int i = 0; i < n_ops; ++i) {
    if (op[i] != OP_M1 && op[i] != OP_M2) continue;
    const int k = mat[i], d = op[i] == OP_M1 ? 2 : 4;
    if (k < 0 || k >= n_mats) return "gate " + std::to_string(i) + ": matrix index " + std::to_string(k) + " outside 0.." + std::to_string(n_mats - 1);
    const cd* m = mats + (size_t)k * 16;
    double dev = 0;
    bool finite = true;
    for (int a = 0; a < d; ++a)
      for (int b = 0; b < d; ++b) {
        finite = finite && std::isfinite(m[a * 4 + b].real()) && std::isfinite(m[a * 4 + b].imag());
        cd g = (a == b) ? cd(-1, 0) : cd(0, 0);
        for (int r = 0; r < d; ++r) g += std::conj(m[r * 4 + a]) * m[r * 4 + b];
        dev = std::max(dev, std::abs(g));
      }
    if (!finite || !(dev <= 1e-12))
      return "gate " + std::to_string(i) + ": the matrix of table entry " + std::to_string(k) + (finite ? " is not unitary (max |M^H M - 1| > 1e-12)" : " has an entry that is not finite");
  }
  return "";
}

// The channel tables of a program and the names of one trajectory (qkb_simulate_channels2); n_channels = 0: no one-qubit table, code 10
// is unknown; n_channels2 = 0: no two-qubit table, code 11 is unknown.
struct Channels {
  int n_channels = 0;
  const cd* kraus = nullptr;        // [n_channels][4][2][2], K[s'][s]
  const int32_t* n_kraus = nullptr; // [n_channels] 1..4
  int n_channels2 = 0;
  const cd* kraus2 = nullptr;        // [n_channels2][16][4][4], K[(p,p')][(s,s')], qubit q0 most significant
  const int32_t* n_kraus2 = nullptr; // [n_channels2] 1..16
  const int32_t* channel = nullptr; // [n_ops], read where op is 10 (index into kraus) or 11 (into kraus2)
  const int32_t* branch = nullptr;  // [n_ops] -1: drawn, k: forced
  uint64_t seed = 0;
  uint32_t state_index = 0, trajectory = 0, first_gate = 0;
  double* logw_out = nullptr;
  int8_t* branches_out = nullptr;   // [channel gates of the program, codes 10 and 11 in program order]
  double* margin_out = nullptr;
  const int32_t* cond_gate = nullptr;  // [n_ops] -1: unconditional; g < i: the channel gate whose branch decides (qkb_simulate_conditions)
  const uint32_t* cond_mask = nullptr; // [n_ops] bit v: branch v of gate cond_gate[i] lets gate i run
  bool any() const { return n_channels > 0 || n_channels2 > 0; }
};

// Philox4x32-10 and the uniform of its first two words, written out as in qk_local_plan.h (smp_philox, smp_uniform) and
// engine.philox4x32: counter (gate, trajectory, state, 2), key = the two halves of the seed.
double channel_uniform(uint64_t seed, uint32_t gate, uint32_t trajectory, uint32_t state) {
  uint32_t c0 = gate, c1 = trajectory, c2 = state, c3 = 2u, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    if (r > 0) k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
  }
  return (double)(((uint64_t)(c0 >> 5) << 26) + (uint64_t)(c1 >> 6)) * (1.0 / 9007199254740992.0);
}

// The channel gates of a program, checked before anything runs: the channel inside its table, 1..4 matrices (1..16 for the two-qubit
// channel of code 11), finite entries, the branch inside -1..m-1, a drawn channel trace preserving to 1e-12, the qubit (pair) inside
// the register.  Empty string, or what is wrong.
std::string check_channels(int n_qubits, int n_ops, const int8_t* op, const int32_t* q0, const Channels& ch) {
  for (int i = 0; i < n_ops; ++i) {
    if (op[i] != OP_K1 && op[i] != OP_K2) continue;
    const bool two = op[i] == OP_K2;
    const int d = two ? 4 : 2, n_table = two ? ch.n_channels2 : ch.n_channels;  // d x d matrices, at most d * d of them
    const std::string at = "gate " + std::to_string(i) + ": ", kind = two ? "two-qubit channel " : "channel ";
    const int c = ch.channel[i], b = ch.branch[i];
    if (c < 0 || c >= n_table) return at + kind + "index " + std::to_string(c) + " outside 0.." + std::to_string(n_table - 1);
    const int m = (two ? ch.n_kraus2 : ch.n_kraus)[c];
    if (m < 1 || m > d * d) return at + kind + std::to_string(c) + " has " + std::to_string(m) + " Kraus matrices (1.." + std::to_string(d * d) + ")";
    const cd* K = (two ? ch.kraus2 : ch.kraus) + (size_t)c * d * d * d * d;
    for (int e = 0; e < d * d * m; ++e)
      if (!std::isfinite(K[e].real()) || !std::isfinite(K[e].imag())) return at + "a Kraus matrix of " + kind + std::to_string(c) + " has an entry that is not finite";
    if (b < -1 || b >= m) return at + "branch " + std::to_string(b) + " outside -1.." + std::to_string(m - 1);
    if (b < 0) {
      double dev = 0;
      for (int a = 0; a < d; ++a)
        for (int e = 0; e < d; ++e) {
          cd g = (a == e) ? cd(-1, 0) : cd(0, 0);
          for (int k = 0; k < m; ++k)
            for (int r = 0; r < d; ++r) g += std::conj(K[(k * d + r) * d + a]) * K[(k * d + r) * d + e];
          dev = std::max(dev, std::abs(g));
        }
      if (!(dev <= 1e-12)) return at + "the drawn " + kind + std::to_string(c) + " is not trace preserving (max |sum K^H K - 1| > 1e-12)";
    }
    if (q0[i] < 0 || q0[i] + (two ? 1 : 0) >= n_qubits) return at + kind + "on a qubit outside the register";
  }
  return "";
}

// The condition rows of a program, checked before anything runs: cond_gate[i] inside -1 .. i-1, the gate it names of code 10 or 11, no
// mask bit at or above the number of Kraus matrices of that gate's channel (check_channels has passed: the channel is valid).
std::string check_conditions(int n_ops, const int8_t* op, const Channels& ch) {
  for (int i = 0; i < n_ops; ++i) {
    const int g = ch.cond_gate[i];
    if (g == -1) continue;
    const std::string at = "gate " + std::to_string(i) + ": ";
    if (g < -1 || g >= i) return at + "condition on gate " + std::to_string(g) + " outside -1.." + std::to_string(i - 1);
    if (op[g] != OP_K1 && op[g] != OP_K2) return at + "condition on gate " + std::to_string(g) + ", which is no channel gate (op code " + std::to_string((int)op[g]) + ")";
    const int m = (op[g] == OP_K2 ? ch.n_kraus2 : ch.n_kraus)[ch.channel[g]];
    if (m < 32 && (ch.cond_mask[i] >> m) != 0u) return at + "condition mask names a branch at or above the " + std::to_string(m) + " of gate " + std::to_string(g);
  }
  return "";
}

// The branch of channel gate i with the probabilities p[m] (tot = p_0 + .. in ascending order): the forced one, or drawn: the first k
// with p_k > 0 and u tot < p_0 + .. + p_k, else the last k with p_k > 0, u the uniform of counter (first_gate + i, trajectory,
// state_index, 2); `margin` takes the smallest |u tot - cum| / tot over the thresholds.  -1 with g_err set when the outcome is
// impossible: tot 0 or not finite in a draw, p_b 0 or not finite.
int channel_branch(const Channels& ch, int i, int forced, int m, const double* p, double* margin) {
  double tot = 0;
  for (int k = 0; k < m; ++k) tot += p[k];
  const auto at = [&] { return "state " + std::to_string(ch.state_index) + ", gate " + std::to_string(ch.first_gate + (uint32_t)i) + ": "; };  // error paths only
  int b = forced;
  if (forced < 0) {
    if (!(tot > 0.0) || !std::isfinite(tot)) {
      g_err = at() + "the branch probabilities of the channel sum to 0 or are not finite";
      return -1;
    }
    const double u = channel_uniform(ch.seed, ch.first_gate + (uint32_t)i, ch.trajectory, ch.state_index);
    double cum = 0;
    int last = -1;
    for (int k = 0; k < m; ++k) {
      cum += p[k];
      if (k < m - 1) *margin = std::min(*margin, std::fabs(u * tot - cum) / tot);
      if (p[k] > 0.0) {
        last = k;
        if (b < 0 && u * tot < cum) b = k;
      }
    }
    if (b < 0) b = last;
  }
  if (!(p[b] > 0.0) || !std::isfinite(p[b])) {
    g_err = at() + "branch " + std::to_string(b) + " of the channel has probability 0 or one that is not finite (an impossible outcome was post-selected?)";
    return -1;
  }
  return b;
}

// row-major C[m x n] = A[m x k] * B[k x n]  (as column-major C^T = B^T A^T)
void gemm_rm(int m, int n, int k, const cd* A, const cd* B, cd* C) {
  const cd one(1.0, 0.0), zero(0.0, 0.0);
  p_zgemm("N", "N", &n, &m, &k, &one, B, &n, A, &k, &zero, C, &n);
}

// The state a run starts from instead of |0...0> (qkb_simulate_initial): already canonical with the centre on `centre`, validated by
// the entry.  It reaches simulate_impl through t_initial, set for the duration of one call on the calling thread: the entries between
// the two keep their signatures.
struct Initial {
  const int32_t* dims = nullptr;  // [n_qubits + 1]
  const cd* tensors = nullptr;    // the sites [l][2][r] row-major, back to back
  int centre = 0;
  double fidelity = 1.0, logw = 0.0;
};
thread_local const Initial* t_initial = nullptr;

struct Tensor {  // [l][2][r], row-major
  int l = 1, r = 1;
  std::vector<cd> v;
  cd& at(int a, int p, int c) { return v[((size_t)a * 2 + p) * r + c]; }
};

// economic QR of a row-major M[m x n]: Q[m x k], R[k x n], k = min(m, n)  (geqrf + ungqr, as scipy.linalg.qr(mode="economic"))
int qr_economic(int m, int n, const cd* M, std::vector<cd>& Q, std::vector<cd>& R, std::vector<cd>& work, std::vector<cd>& cm) {
  const int k = std::min(m, n);
  cm.resize((size_t)m * n);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) cm[(size_t)j * m + i] = M[(size_t)i * n + j];  // to column-major
  std::vector<cd> tau(k);
  int info = 0, lwork = -1;
  cd wq;
  p_zgeqrf(&m, &n, cm.data(), &m, tau.data(), &wq, &lwork, &info);
  lwork = std::max(1, (int)wq.real());
  if ((int)work.size() < lwork) work.resize(lwork);
  p_zgeqrf(&m, &n, cm.data(), &m, tau.data(), work.data(), &lwork, &info);
  if (info != 0) return info;
  R.assign((size_t)k * n, cd(0, 0));
  for (int i = 0; i < k; ++i)
    for (int j = i; j < n; ++j) R[(size_t)i * n + j] = cm[(size_t)j * m + i];
  lwork = -1;
  p_zungqr(&m, &k, &k, cm.data(), &m, tau.data(), &wq, &lwork, &info);
  lwork = std::max(1, (int)wq.real());
  if ((int)work.size() < lwork) work.resize(lwork);
  p_zungqr(&m, &k, &k, cm.data(), &m, tau.data(), work.data(), &lwork, &info);
  if (info != 0) return info;
  Q.resize((size_t)m * k);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < k; ++j) Q[(size_t)i * k + j] = cm[(size_t)j * m + i];
  return 0;
}

// how many leading singular values survive, and the kept fraction of the weight (mps.py:_kept)
int kept(const std::vector<double>& s, double budget, double zero, double* frac) {
  const int n = (int)s.size();
  double total = 0;
  for (double x : s) total += x * x;
  int keep = 0;
  for (double x : s) keep += (x > zero);
  keep = std::max(keep, 1);
  double tail = 0;
  int drop = 0;
  for (int i = keep - 1; i >= 0; --i) {  // cumulative weight from the small end; count entries <= budget * total
    tail += s[i] * s[i];
    if (tail <= budget * total) ++drop;
    else break;
  }
  keep = std::max(keep - drop, 1);
  double w = 0;
  for (int i = 0; i < keep; ++i) w += s[i] * s[i];
  *frac = w / total;
  (void)n;
  return keep;
}
}  // namespace

extern "C" {

const char* qkb_last_error(void) { return g_err.c_str(); }

// Resolve LAPACK / BLAS from the OpenBLAS shipped with scipy.  Returns 0 on success.
int qkb_init(const char* openblas_path) {
  if (p_zgesdd) return 0;
  void* h = dlopen(openblas_path, RTLD_NOW | RTLD_GLOBAL);
  if (!h) {
    g_err = std::string("dlopen failed: ") + dlerror();
    return -1;
  }
  auto sym = [&](const char* a, const char* b) -> void* {
    void* s = dlsym(h, a);
    return s ? s : dlsym(h, b);
  };
  p_zgesdd = (zgesdd_t)sym("scipy_zgesdd_", "zgesdd_");
  p_zgeqrf = (zgeqrf_t)sym("scipy_zgeqrf_", "zgeqrf_");
  p_zungqr = (zungqr_t)sym("scipy_zungqr_", "zungqr_");
  p_zgemm = (zgemm_t)sym("scipy_zgemm_", "zgemm_");
  if (!p_zgesdd || !p_zgeqrf || !p_zungqr || !p_zgemm) {
    p_zgesdd = nullptr;
    g_err = "the library does not export zgesdd_/zgeqrf_/zungqr_/zgemm_";
    return -2;
  }
  return 0;
}

// MPS of circuit |0...0>.  op/q0/alpha: the bound gate program (ansatz.py: BoundCircuit).  On success fills
// dims_out[n_qubits + 1] and *tensors_out: ONE malloc'd block holding the site tensors back to back, complex128
// [l][2][r] row-major (free it with qkb_free), and *fidelity.  Returns 0, or a negative code with qkb_last_error().
// Op codes: 0 H, 1 Rz, 2 XXPhase, 3 SWAP, 4 Rx, 5 Ry, 6 YYPhase, 7 ZZPhase (two-qubit gates on (q0, q0+1)); any other
// code fails the call with -7 before a gate is applied.
int qkb_simulate_gates(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                       int32_t max_bond, int32_t n_mats, const double* mats, const int32_t* mat, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out,
                       double* fidelity_out);
static int simulate_impl(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                         int32_t max_bond, int32_t n_mats, const double* mats_raw, const int32_t* mat, const Channels& ch, int32_t* dims_out, double** tensors_out,
                         int64_t* n_complex_out, double* fidelity_out);
int qkb_simulate(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget,
                 double value_of_zero, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out, double* fidelity_out) {
  return qkb_simulate_gates(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, 0, 0, nullptr, nullptr, dims_out, tensors_out, n_complex_out, fidelity_out);
}
// max_bond > 0: at most that many singular values survive a gate (the chi of pytket-cutensornet's Config, reference
// gpu_backend/kernel_state_ansatz.py:141-144); the lost weight goes into the fidelity like any other truncation.
int qkb_simulate_chi(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget,
                     double value_of_zero, int32_t max_bond, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out, double* fidelity_out) {
  return qkb_simulate_gates(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, 0, nullptr, nullptr, dims_out, tensors_out, n_complex_out, fidelity_out);
}
// qkb_simulate_chi with a matrix table: with n_mats > 0 the program may also hold op codes 8 (a 2x2 on q0) and 9 (a 4x4 on (q0, q0+1),
// index (s_q0, s_q0+1), q0 most significant); the matrix of gate i is mats[mat[i]], complex128 [n_mats][4][4] row-major (re, im), a 2x2 in
// [:2][:2]; alpha[i] is ignored there, mat[i] is read at those codes only.  new[(p,p')] = sum M[(p,p')][(s,s')] old[(s,s')].  A mat[i] outside
// 0..n_mats-1 or a matrix that is not finite and unitary to 1e-12 fails the call with -8 before a gate is applied; with n_mats = 0
// codes 8 and 9 are unknown (-7).
int qkb_simulate_gates(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                       int32_t max_bond, int32_t n_mats, const double* mats_raw, const int32_t* mat, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out,
                       double* fidelity_out) {
  return simulate_impl(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats_raw, mat, Channels{}, dims_out, tensors_out, n_complex_out, fidelity_out);
}
// qkb_simulate_gates with a channel table: with n_channels > 0 the program may also hold op code 10, a one-qubit Kraus channel on q0.
// Channel c is n_kraus[c] (1..4) matrices kraus[c][k][s'][s] (complex128 [n_channels][4][2][2], (re, im)); gate i reads channel
// channel[i] and draws its branch (branch[i] = -1) or takes branch[i]; alpha[i] and mat[i] are ignored there.  The step: the centre
// is brought onto q exactly, N = sum |A_q|^2, p_k = sum |K_k A_q|^2 and tot = p_0 + .. in ascending order of elements and of k; drawn:
// u = uniform of Philox counter (first_gate + i, trajectory, state_index, 2) and key (seed), b the first k with p_k > 0 and
// u tot < p_0 + .. + p_k, else the last k with p_k > 0; A_q <- (K_b / sqrt(p_b)) A_q; logw += log(p_b / N).  *logw_out, branches_out
// [channel gates] and *margin_out (the smallest |u tot - cum| / tot over the thresholds of all draws, inf without one) may be null.
// -8 before a gate is applied for a bad channel gate (check_channels); -9 when p_b is 0 or not finite or tot is 0 in a draw, naming
// the state and the gate.  With n_channels = 0 the call IS qkb_simulate_gates.
int qkb_simulate_channels(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                          int32_t max_bond, int32_t n_mats, const double* mats_raw, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                          const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate, int32_t* dims_out,
                          double** tensors_out, int64_t* n_complex_out, double* fidelity_out, double* logw_out, int8_t* branches_out, double* margin_out) {
  Channels ch;
  if (n_channels < 0 || (n_channels > 0 && (!kraus || !n_kraus || !channel || !branch))) {
    g_err = "a channel table needs n_channels >= 0, kraus, n_kraus, channel and branch";
    return -8;
  }
  if (n_channels > 0) {
    ch.n_channels = n_channels, ch.kraus = reinterpret_cast<const cd*>(kraus), ch.n_kraus = n_kraus, ch.channel = channel, ch.branch = branch;
    ch.seed = seed, ch.state_index = state_index, ch.trajectory = trajectory, ch.first_gate = first_gate;
  }
  ch.logw_out = logw_out, ch.branches_out = branches_out, ch.margin_out = margin_out;
  return simulate_impl(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats_raw, mat, ch, dims_out, tensors_out, n_complex_out, fidelity_out);
}
// qkb_simulate_channels with a two-qubit channel table: with n_channels2 > 0 the program may also hold op code 11, a two-qubit Kraus
// channel on (q0, q0+1).  Channel c is n_kraus2[c] (1..16) matrices kraus2[c][k][(p,p')][(s,s')] (complex128 [n_channels2][16][4][4],
// (re, im); the index convention of the 4x4 matrix gates, q0 most significant); gate i reads channel[i] -- an index into kraus2 where
// op is 11 -- and branch[i].  The step: the centre is brought onto the pair and theta = A_q A_q+1 formed as for any two-qubit gate;
// N = sum |theta|^2, p_k = sum_{a,c} |K_k theta[a,(.,.),c]|^2 in ascending order of (a, c), the branch as for code 10 (same uniform);
// theta <- (K_b / sqrt(p_b)) theta, then the SVD, truncation, fidelity product and centre placement of a two-qubit gate; logw +=
// log(p_b / N).  branches_out counts the gates of codes 10 and 11 together in program order.  Errors as qkb_simulate_channels.  Either
// table may be absent; with n_channels2 = 0 the call IS qkb_simulate_channels.
int qkb_simulate_channels2(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                           int32_t max_bond, int32_t n_mats, const double* mats_raw, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                           const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate,
                           int32_t n_channels2, const double* kraus2, const int32_t* n_kraus2, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out,
                           double* fidelity_out, double* logw_out, int8_t* branches_out, double* margin_out) {
  if (n_channels2 == 0)
    return qkb_simulate_channels(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats_raw, mat, n_channels, kraus, n_kraus, channel, branch, seed,
                                 state_index, trajectory, first_gate, dims_out, tensors_out, n_complex_out, fidelity_out, logw_out, branches_out, margin_out);
  Channels ch;
  if (n_channels < 0 || n_channels2 < 0 || !kraus2 || !n_kraus2 || !channel || !branch || (n_channels > 0 && (!kraus || !n_kraus))) {
    g_err = "a channel table needs n_channels >= 0, kraus, n_kraus, channel and branch; a two-qubit one n_channels2 >= 0, kraus2 and n_kraus2";
    return -8;
  }
  if (n_channels > 0) ch.n_channels = n_channels, ch.kraus = reinterpret_cast<const cd*>(kraus), ch.n_kraus = n_kraus;
  ch.n_channels2 = n_channels2, ch.kraus2 = reinterpret_cast<const cd*>(kraus2), ch.n_kraus2 = n_kraus2, ch.channel = channel, ch.branch = branch;
  ch.seed = seed, ch.state_index = state_index, ch.trajectory = trajectory, ch.first_gate = first_gate;
  ch.logw_out = logw_out, ch.branches_out = branches_out, ch.margin_out = margin_out;
  return simulate_impl(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats_raw, mat, ch, dims_out, tensors_out, n_complex_out, fidelity_out);
}
// qkb_simulate_channels2 with condition rows: gate i with cond_gate[i] = g >= 0 (g < i, a gate of op code 10 or 11 of this program) runs
// when the branch b recorded for gate g is >= 0 and bit b of cond_mask[i] is set; else it is skipped: no centre move, no theta, no SVD,
// no change of a bond, of the fidelity or of logw, no draw, no contribution to the margin; a skipped channel gate records branch -2 (a
// condition on it is false).  The look-ahead that places the centre behind a two-qubit gate counts skipped gates as present.  -8
// before a gate is applied, naming the gate, for rows without a channel table, cond_gate[i] outside -1 .. i-1, a gate named that is
// not of code 10 or 11, a mask bit at or above the number of that gate's Kraus matrices, cond_mask null.  With cond_gate null the
// call IS qkb_simulate_channels2.
int qkb_simulate_conditions(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                            int32_t max_bond, int32_t n_mats, const double* mats_raw, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                            const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate,
                            int32_t n_channels2, const double* kraus2, const int32_t* n_kraus2, const int32_t* cond_gate, const uint32_t* cond_mask, int32_t* dims_out,
                            double** tensors_out, int64_t* n_complex_out, double* fidelity_out, double* logw_out, int8_t* branches_out, double* margin_out) {
  if (!cond_gate)
    return qkb_simulate_channels2(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats_raw, mat, n_channels, kraus, n_kraus, channel, branch, seed,
                                  state_index, trajectory, first_gate, n_channels2, kraus2, n_kraus2, dims_out, tensors_out, n_complex_out, fidelity_out, logw_out, branches_out,
                                  margin_out);
  if (!cond_mask) {
    g_err = "condition rows need cond_gate and cond_mask";
    return -8;
  }
  if (n_channels <= 0 && n_channels2 <= 0) {
    g_err = "gate 0: condition rows need a program with a channel table";
    return -8;
  }
  Channels ch;
  if ((n_channels > 0 && (!kraus || !n_kraus)) || (n_channels2 > 0 && (!kraus2 || !n_kraus2)) || !channel || !branch) {
    g_err = "a channel table needs n_channels >= 0, kraus, n_kraus, channel and branch; a two-qubit one n_channels2 >= 0, kraus2 and n_kraus2";
    return -8;
  }
  if (n_channels > 0) ch.n_channels = n_channels, ch.kraus = reinterpret_cast<const cd*>(kraus), ch.n_kraus = n_kraus;
  if (n_channels2 > 0) ch.n_channels2 = n_channels2, ch.kraus2 = reinterpret_cast<const cd*>(kraus2), ch.n_kraus2 = n_kraus2;
  ch.channel = channel, ch.branch = branch, ch.cond_gate = cond_gate, ch.cond_mask = cond_mask;
  ch.seed = seed, ch.state_index = state_index, ch.trajectory = trajectory, ch.first_gate = first_gate;
  ch.logw_out = logw_out, ch.branches_out = branches_out, ch.margin_out = margin_out;
  return simulate_impl(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats_raw, mat, ch, dims_out, tensors_out, n_complex_out, fidelity_out);
}
// qkb_simulate_conditions from a given state: init_dims [n_qubits + 1] and init_tensors (the sites [l][2][r] complex128 row-major, back to
// back) replace |0...0>; the state is taken as it stands -- canonical with its orthogonality centre on init_centre -- and the run begins
// with init_fidelity and init_logw.  -8 before a gate is applied for a bond table that does not chain (dims[0] != 1, dims[n] != 1, an
// entry that is not positive), a centre outside the register, or an entry (tensor, fidelity, log-weight) that is not finite.  With
// init_dims null the call IS qkb_simulate_conditions.
int qkb_simulate_initial(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                         int32_t max_bond, int32_t n_mats, const double* mats_raw, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                         const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate,
                         int32_t n_channels2, const double* kraus2, const int32_t* n_kraus2, const int32_t* cond_gate, const uint32_t* cond_mask, const int32_t* init_dims,
                         const double* init_tensors, int32_t init_centre, double init_fidelity, double init_logw, int32_t* dims_out, double** tensors_out,
                         int64_t* n_complex_out, double* fidelity_out, double* logw_out, int8_t* branches_out, double* margin_out) {
  Initial init;
  if (init_dims) {
    if (!init_tensors || n_qubits < 1) {
      g_err = "an initial state needs init_dims and init_tensors";
      return -8;
    }
    if (init_dims[0] != 1 || init_dims[n_qubits] != 1) {
      g_err = "the initial state's boundary bonds must be 1";
      return -8;
    }
    size_t total = 0;
    for (int k = 0; k <= n_qubits; ++k) {
      if (init_dims[k] <= 0) {
        g_err = "the initial state's bond " + std::to_string(k) + " is " + std::to_string((int)init_dims[k]) + ": bonds must be positive";
        return -8;
      }
      if (k < n_qubits) total += (size_t)init_dims[k] * 2 * (size_t)std::max(init_dims[k + 1], 0);
    }
    if (init_centre < 0 || init_centre >= n_qubits) {
      g_err = "the initial state's centre " + std::to_string((int)init_centre) + " lies outside the register of " + std::to_string((int)n_qubits);
      return -8;
    }
    for (size_t e = 0; e < 2 * total; ++e)
      if (!std::isfinite(init_tensors[e])) {
        g_err = "the initial state has an entry that is not finite";
        return -8;
      }
    if (!std::isfinite(init_fidelity) || !std::isfinite(init_logw)) {
      g_err = "the initial state's fidelity or log-weight is not finite";
      return -8;
    }
    init.dims = init_dims, init.tensors = reinterpret_cast<const cd*>(init_tensors), init.centre = init_centre, init.fidelity = init_fidelity, init.logw = init_logw;
    t_initial = &init;
  }
  const int rc = qkb_simulate_conditions(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats_raw, mat, n_channels, kraus, n_kraus, channel, branch, seed,
                                         state_index, trajectory, first_gate, n_channels2, kraus2, n_kraus2, cond_gate, cond_mask, dims_out, tensors_out, n_complex_out, fidelity_out,
                                         logw_out, branches_out, margin_out);
  t_initial = nullptr;
  return rc;
}
}  // extern "C"

static int simulate_impl(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                         int32_t max_bond, int32_t n_mats, const double* mats_raw, const int32_t* mat, const Channels& ch, int32_t* dims_out, double** tensors_out,
                         int64_t* n_complex_out, double* fidelity_out) {
  if (!p_zgesdd) {
    g_err = "qkb_init has not been called";
    return -1;
  }
  const int n = n_qubits;
  const cd* mats = reinterpret_cast<const cd*>(mats_raw);
  if (n_mats < 0 || (n_mats > 0 && (!mats || !mat))) {
    g_err = "a matrix table needs n_mats >= 0, mats and mat";
    return -8;
  }
  const int n_codes = n_mats > 0 ? N_OPS_MAT : N_OPS;
  for (int i = 0; i < n_ops; ++i)
    if ((op[i] < 0 || op[i] >= n_codes) && !(ch.n_channels > 0 && op[i] == OP_K1) && !(ch.n_channels2 > 0 && op[i] == OP_K2)) {
      g_err = "unknown gate op code " + std::to_string((int)op[i]) + " (valid: 0.." + std::to_string(n_codes - 1) + (ch.n_channels > 0 ? ", 10" : "") + (ch.n_channels2 > 0 ? ", 11)" : ")");
      return -7;
    }
  if (n_mats > 0) {
    g_err = check_table(n_ops, op, n_mats, mats, mat);
    if (!g_err.empty()) return -8;
  }
  if (ch.any()) {
    g_err = check_channels(n, n_ops, op, q0, ch);
    if (!g_err.empty()) return -8;
    if (ch.cond_gate) {
      g_err = check_conditions(n_ops, op, ch);
      if (!g_err.empty()) return -8;
    }
  }
  double logw = 0.0, margin = INFINITY;
  int n_drawn = 0;  // channel gates done: the index into branches_out
  std::vector<int> taken(ch.cond_gate ? n_ops : 0, -1);  // the branch every channel gate of this state took (-2: skipped), by position
  std::vector<Tensor> A(n);
  for (auto& t : A) t.v = {cd(1, 0), cd(0, 0)};
  const Initial* const init = t_initial;
  std::vector<int> two_q_pos;
  for (int i = 0; i < n_ops; ++i)
    if (is_two_qubit(op[i])) two_q_pos.push_back(q0[i]);
  double fidelity = 1.0;
  int centre = 0;  // sites < centre are left-orthonormal, sites > centre right-orthonormal
  if (init) {  // the run goes on from a given state: its sites, centre, fidelity and log-weight
    const cd* src = init->tensors;
    for (int k = 0; k < n; ++k) {
      A[k].l = init->dims[k], A[k].r = init->dims[k + 1];
      const size_t cnt = (size_t)A[k].l * 2 * A[k].r;
      A[k].v.assign(src, src + cnt);
      src += cnt;
    }
    centre = init->centre, fidelity = init->fidelity, logw = init->logw;
  }
  size_t g2 = 0;
  std::vector<cd> Q, R, work, cm, theta, U, VT, tmp;
  std::vector<double> S, rwork;
  std::vector<int> iwork;
  const double sqrt_half = 0.7071067811865476;

  for (int i = 0; i < n_ops; ++i) {
    const int o = op[i], q = q0[i];
    if (q < 0 || q >= n || (is_two_qubit(o) && q + 1 >= n)) {
      g_err = "gate on a qubit outside the register";
      return -3;
    }
    if (ch.cond_gate && ch.cond_gate[i] >= 0) {  // a gate whose condition is false does nothing at all; it is a done gate all the same
      const int b = taken[ch.cond_gate[i]];
      if (b < 0 || !((ch.cond_mask[i] >> b) & 1u)) {
        if (o == OP_K1 || o == OP_K2) {
          taken[i] = -2;
          if (ch.branches_out) ch.branches_out[n_drawn] = -2;
          ++n_drawn;
        }
        g2 += is_two_qubit(o);  // the look-ahead is a function of the op codes alone
        continue;
      }
    }
    if (o == OP_H) {
      Tensor& t = A[q];
      for (int a = 0; a < t.l; ++a)
        for (int c = 0; c < t.r; ++c) {
          const cd t0 = t.at(a, 0, c), t1 = t.at(a, 1, c);
          t.at(a, 0, c) = (t0 + t1) * sqrt_half;
          t.at(a, 1, c) = (t0 - t1) * sqrt_half;
        }
      continue;
    }
    if (o == OP_RZ) {
      const double th = 0.5 * M_PI * alpha[i];
      const cd ph(std::cos(th), std::sin(th));
      Tensor& t = A[q];
      for (int a = 0; a < t.l; ++a)
        for (int c = 0; c < t.r; ++c) {
          t.at(a, 0, c) *= std::conj(ph);
          t.at(a, 1, c) *= ph;
        }
      continue;
    }
    if (o == OP_M1) {  // a 2x2 from the table
      const cd* M = mats + (size_t)mat[i] * 16;
      Tensor& t = A[q];
      for (int a = 0; a < t.l; ++a)
        for (int c = 0; c < t.r; ++c) {
          const cd v[2] = {t.at(a, 0, c), t.at(a, 1, c)};
          t.at(a, 0, c) = mat_dot(M, v, 2);
          t.at(a, 1, c) = mat_dot(M + 4, v, 2);
        }
      continue;
    }
    if (!is_two_qubit(o) && o != OP_K1) {  // Rx: [[c, -i s], [-i s, c]];  Ry: [[c, -s], [s, c]]
      const double th = 0.5 * M_PI * alpha[i];
      const double cs = std::cos(th), sn = std::sin(th);
      const cd m01 = o == OP_RX ? cd(0.0, -sn) : cd(-sn, 0.0), m10 = o == OP_RX ? cd(0.0, -sn) : cd(sn, 0.0);
      Tensor& t = A[q];
      for (int a = 0; a < t.l; ++a)
        for (int c = 0; c < t.r; ++c) {
          const cd t0 = t.at(a, 0, c), t1 = t.at(a, 1, c);
          t.at(a, 0, c) = cs * t0 + m01 * t1;
          t.at(a, 1, c) = m10 * t0 + cs * t1;
        }
      continue;
    }
    // ---- two-qubit gate on (q, q+1): bring the orthogonality centre onto the pair; a channel on q: onto the site
    const int lo = q, hi = (o == OP_K1) ? q : q + 1;
    while (centre < lo) {
      Tensor& t = A[centre];
      const int m = t.l * 2, nn = t.r;
      if (qr_economic(m, nn, t.v.data(), Q, R, work, cm) != 0) {
        g_err = "zgeqrf/zungqr failed";
        return -4;
      }
      const int k = std::min(m, nn);
      Tensor& u = A[centre + 1];  // u <- R u : [k][2 r2] = R[k x nn] * u[nn x 2 r2]
      tmp.resize((size_t)k * 2 * u.r);
      gemm_rm(k, 2 * u.r, nn, R.data(), u.v.data(), tmp.data());
      u.v = tmp;
      u.l = k;
      t.v = Q;
      t.r = k;
      ++centre;
    }
    while (centre > hi) {
      Tensor& t = A[centre];  // [l][2 r] -> QR of its transpose [2r x l]
      const int l = t.l, w = 2 * t.r;
      cm.resize(0);
      std::vector<cd> Tt((size_t)w * l);
      for (int a = 0; a < l; ++a)
        for (int c = 0; c < w; ++c) Tt[(size_t)c * l + a] = t.v[(size_t)a * w + c];
      if (qr_economic(w, l, Tt.data(), Q, R, work, cm) != 0) {
        g_err = "zgeqrf/zungqr failed";
        return -4;
      }
      const int k = std::min(w, l);
      Tensor& d = A[centre - 1];  // d <- d * R^T : new[i,p,j] = sum_l d[i,p,l] R[j,l]
      std::vector<cd> Rt((size_t)l * k);
      for (int jj = 0; jj < k; ++jj)
        for (int a = 0; a < l; ++a) Rt[(size_t)a * k + jj] = R[(size_t)jj * l + a];
      tmp.resize((size_t)d.l * 2 * k);
      gemm_rm(d.l * 2, k, l, d.v.data(), Rt.data(), tmp.data());
      d.v = tmp;
      d.r = k;
      t.v.resize((size_t)k * w);  // t <- Q^T : [k][2 r]
      for (int jj = 0; jj < k; ++jj)
        for (int c = 0; c < w; ++c) t.v[(size_t)jj * w + c] = Q[(size_t)c * k + jj];
      t.l = k;
      --centre;
    }
    if (o == OP_K1) {  // the channel step: the centre stays on q, the bonds do not change
      const int c = ch.channel[i], forced = ch.branch[i], m = ch.n_kraus[c];
      const cd* K = ch.kraus + (size_t)c * 16;
      Tensor& t = A[q];
      double N = 0, p[4] = {0, 0, 0, 0};
      for (int a = 0; a < t.l; ++a)  // every sum in ascending order of (a, c)
        for (int x = 0; x < t.r; ++x) {
          const cd v[2] = {t.at(a, 0, x), t.at(a, 1, x)};
          N += std::norm(v[0]) + std::norm(v[1]);
          for (int k = 0; k < m; ++k) p[k] += std::norm(mat_dot(K + k * 4, v, 2)) + std::norm(mat_dot(K + k * 4 + 2, v, 2));
        }
      const int b = channel_branch(ch, i, forced, m, p, &margin);
      if (b < 0) return -9;
      const double s = std::sqrt(p[b]);
      const cd Kb[4] = {K[b * 4] / s, K[b * 4 + 1] / s, K[b * 4 + 2] / s, K[b * 4 + 3] / s};
      for (int a = 0; a < t.l; ++a)
        for (int x = 0; x < t.r; ++x) {
          const cd v[2] = {t.at(a, 0, x), t.at(a, 1, x)};
          t.at(a, 0, x) = mat_dot(Kb, v, 2);
          t.at(a, 1, x) = mat_dot(Kb + 2, v, 2);
        }
      logw += std::log(p[b] / N);
      if (ch.branches_out) ch.branches_out[n_drawn] = (int8_t)b;
      if (ch.cond_gate) taken[i] = b;
      ++n_drawn;
      continue;
    }
    Tensor& a0 = A[q];
    Tensor& a1 = A[q + 1];
    const int l = a0.l, mid = a0.r, r = a1.r;
    const int m = 2 * l, nn = 2 * r;
    theta.resize((size_t)m * nn);  // theta[(a,p)][(p',c)]
    gemm_rm(m, nn, mid, a0.v.data(), a1.v.data(), theta.data());
    auto TH = [&](int a, int p, int pp, int c) -> cd& { return theta[((size_t)(a * 2 + p)) * nn + (size_t)pp * r + c]; };
    if (o == OP_SWAP) {
      for (int a = 0; a < l; ++a)
        for (int c = 0; c < r; ++c) std::swap(TH(a, 0, 1, c), TH(a, 1, 0, c));
    } else if (o == OP_YY) {  // YYPhase: cos(th) 1 - i sin(th) Y(x)Y
      const double th = 0.5 * M_PI * alpha[i];
      const double cs = std::cos(th), sn = std::sin(th);
      const cd pis(0.0, sn), mis(0.0, -sn);
      for (int a = 0; a < l; ++a)
        for (int c = 0; c < r; ++c) {
          const cd t00 = TH(a, 0, 0, c), t01 = TH(a, 0, 1, c), t10 = TH(a, 1, 0, c), t11 = TH(a, 1, 1, c);
          TH(a, 0, 0, c) = cs * t00 + pis * t11;
          TH(a, 0, 1, c) = cs * t01 + mis * t10;
          TH(a, 1, 0, c) = cs * t10 + mis * t01;
          TH(a, 1, 1, c) = cs * t11 + pis * t00;
        }
    } else if (o == OP_ZZ) {  // ZZPhase: diag(e^-i th, e^i th, e^i th, e^-i th)
      const double th = 0.5 * M_PI * alpha[i];
      const cd ph(std::cos(th), std::sin(th)), phc = std::conj(ph);
      for (int a = 0; a < l; ++a)
        for (int c = 0; c < r; ++c) {
          TH(a, 0, 0, c) *= phc;
          TH(a, 0, 1, c) *= ph;
          TH(a, 1, 0, c) *= ph;
          TH(a, 1, 1, c) *= phc;
        }
    } else if (o == OP_K2) {  // a two-qubit Kraus channel: code 10's branch logic on theta, then the SVD of any two-qubit gate
      const int c = ch.channel[i], forced = ch.branch[i], nk = ch.n_kraus2[c];
      const cd* K = ch.kraus2 + (size_t)c * 256;
      double N = 0, p[16] = {0};
      for (int a = 0; a < l; ++a)  // every sum in ascending order of (a, c)
        for (int x = 0; x < r; ++x) {
          const cd v[4] = {TH(a, 0, 0, x), TH(a, 0, 1, x), TH(a, 1, 0, x), TH(a, 1, 1, x)};
          N += std::norm(v[0]) + std::norm(v[1]) + std::norm(v[2]) + std::norm(v[3]);
          for (int k = forced < 0 ? 0 : forced; k < (forced < 0 ? nk : forced + 1); ++k) {  // a forced branch needs p_b only
            const cd* Kk = K + k * 16;
            p[k] += std::norm(mat_dot(Kk, v, 4)) + std::norm(mat_dot(Kk + 4, v, 4)) + std::norm(mat_dot(Kk + 8, v, 4)) + std::norm(mat_dot(Kk + 12, v, 4));
          }
        }
      const int b = channel_branch(ch, i, forced, nk, p, &margin);
      if (b < 0) return -9;
      const double s = std::sqrt(p[b]);
      cd Kb[16];
      for (int e = 0; e < 16; ++e) Kb[e] = K[b * 16 + e] / s;
      for (int a = 0; a < l; ++a)
        for (int x = 0; x < r; ++x) {
          const cd v[4] = {TH(a, 0, 0, x), TH(a, 0, 1, x), TH(a, 1, 0, x), TH(a, 1, 1, x)};
          TH(a, 0, 0, x) = mat_dot(Kb, v, 4);
          TH(a, 0, 1, x) = mat_dot(Kb + 4, v, 4);
          TH(a, 1, 0, x) = mat_dot(Kb + 8, v, 4);
          TH(a, 1, 1, x) = mat_dot(Kb + 12, v, 4);
        }
      logw += std::log(p[b] / N);
      if (ch.branches_out) ch.branches_out[n_drawn] = (int8_t)b;
      if (ch.cond_gate) taken[i] = b;
      ++n_drawn;
    } else if (o == OP_M2) {  // a 4x4 from the table on (t00, t01, t10, t11)
      const cd* M = mats + (size_t)mat[i] * 16;
      for (int a = 0; a < l; ++a)
        for (int c = 0; c < r; ++c) {
          const cd v[4] = {TH(a, 0, 0, c), TH(a, 0, 1, c), TH(a, 1, 0, c), TH(a, 1, 1, c)};
          TH(a, 0, 0, c) = mat_dot(M, v, 4);
          TH(a, 0, 1, c) = mat_dot(M + 4, v, 4);
          TH(a, 1, 0, c) = mat_dot(M + 8, v, 4);
          TH(a, 1, 1, c) = mat_dot(M + 12, v, 4);
        }
    } else {  // XXPhase: cos(th) 1 - i sin(th) X(x)X
      const double th = 0.5 * M_PI * alpha[i];
      const double cs = std::cos(th), sn = std::sin(th);
      const cd mis(0.0, -sn);
      for (int a = 0; a < l; ++a)
        for (int c = 0; c < r; ++c) {
          const cd t00 = TH(a, 0, 0, c), t01 = TH(a, 0, 1, c), t10 = TH(a, 1, 0, c), t11 = TH(a, 1, 1, c);
          TH(a, 0, 0, c) = cs * t00 + mis * t11;
          TH(a, 0, 1, c) = cs * t01 + mis * t10;
          TH(a, 1, 0, c) = cs * t10 + mis * t01;
          TH(a, 1, 1, c) = cs * t11 + mis * t00;
        }
    }
    // ---- SVD (gesdd, jobz = 'S') of the row-major theta[m x nn]: hand LAPACK the column-major view theta^T [nn x m];
    // theta^T = U' S V'^H  =>  theta = conj(V') S U'^T, i.e. U = conj(V'), Vh = U'^T.  Column-major U' [nn x k] read as
    // row-major is U'^T = Vh [k x nn]; column-major V'^H [k x m] read as row-major is (V'^H)^T = conj(V') = U ... [m x k].
    const int k = std::min(m, nn);
    S.resize(k);
    U.resize((size_t)nn * k);   // LAPACK "U" of theta^T, column-major [nn x k]  == row-major Vh [k x nn]
    VT.resize((size_t)k * m);   // LAPACK "VT" of theta^T, column-major [k x m]  == row-major [m x k] = U of theta
    int info = 0, lwork = -1;
    cd wq;
    const int mnmin = k, mnmax = std::max(m, nn);
    rwork.resize((size_t)std::max(5 * mnmin * mnmin + 5 * mnmin, 2 * mnmax * mnmin + 2 * mnmin * mnmin + mnmin) + 16);
    iwork.resize((size_t)8 * mnmin);
    p_zgesdd("S", &nn, &m, theta.data(), &nn, S.data(), U.data(), &nn, VT.data(), &k, &wq, &lwork, rwork.data(), iwork.data(), &info);
    lwork = std::max(1, (int)wq.real());
    if ((int)work.size() < lwork) work.resize(lwork);
    p_zgesdd("S", &nn, &m, theta.data(), &nn, S.data(), U.data(), &nn, VT.data(), &k, work.data(), &lwork, rwork.data(), iwork.data(), &info);
    if (info != 0) {
      g_err = "zgesdd failed";
      return -5;
    }
    double frac = 1.0;
    int keep = kept(S, trunc_budget, value_of_zero, &frac);
    if (max_bond > 0 && keep > max_bond) {  // the chi cap
      keep = max_bond;
      double tot = 0, w = 0;
      for (double x : S) tot += x * x;
      for (int j = 0; j < keep; ++j) w += S[j] * S[j];
      frac = w / tot;
    }
    fidelity *= frac;
    double nrm = 0;
    for (int j = 0; j < keep; ++j) nrm += S[j] * S[j];
    nrm = std::sqrt(nrm);
    ++g2;
    const int nxt = g2 < two_q_pos.size() ? two_q_pos[g2] : q;
    const bool centre_right = (nxt >= q + 1) || (nxt == q);
    // U of theta: element [row][j] = VT_colmajor[j + row * k] (VT is [k x m] column-major: (j, row) at j + row * k)
    a0.v.resize((size_t)m * keep);
    for (int row = 0; row < m; ++row)
      for (int j = 0; j < keep; ++j) a0.v[(size_t)row * keep + j] = VT[(size_t)row * k + j] * (centre_right ? 1.0 : S[j] / nrm);
    a0.r = keep;
    // Vh of theta: element [j][col] = U_colmajor[col + j * nn]
    a1.v.resize((size_t)keep * nn);
    for (int j = 0; j < keep; ++j)
      for (int col = 0; col < nn; ++col) a1.v[(size_t)j * nn + col] = U[(size_t)j * nn + col] * (centre_right ? S[j] / nrm : 1.0);
    a1.l = keep;
    centre = centre_right ? q + 1 : q;
  }
  // ---- hand the tensors over as one block
  int64_t total = 0;
  dims_out[0] = 1;
  for (int k2 = 0; k2 < n; ++k2) {
    dims_out[k2 + 1] = A[k2].r;
    total += (int64_t)A[k2].v.size();
  }
  cd* block = (cd*)std::malloc((size_t)total * sizeof(cd));
  if (!block) {
    g_err = "out of memory";
    return -6;
  }
  int64_t pos = 0;
  for (int k2 = 0; k2 < n; ++k2) {
    std::memcpy(block + pos, A[k2].v.data(), A[k2].v.size() * sizeof(cd));
    pos += (int64_t)A[k2].v.size();
  }
  *tensors_out = reinterpret_cast<double*>(block);
  *n_complex_out = total;
  *fidelity_out = fidelity;
  if (ch.logw_out) *ch.logw_out = logw;
  if (ch.margin_out) *ch.margin_out = margin;
  return 0;
}

extern "C" {
void qkb_free(double* p) { std::free(p); }

}  // extern "C"
