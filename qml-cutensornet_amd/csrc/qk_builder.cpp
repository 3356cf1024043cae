// qk_builder.cpp -- native host builder of the ansatz MPS: the same algorithm as
// qml-cutensornet_amd/mps.py:_simulate (one LAPACK gesdd per two-qubit gate, QR centre moves, ITensors-style cutoff),
// without the Python interpreter between the 10^3 ... 10^4 small LAPACK calls of a circuit.  Plain C++ (g++), no HIP:
// built as libqkbuilder.so next to libqkgram.so.  LAPACK/BLAS come from the OpenBLAS that scipy already ships
// (symbols scipy_zgesdd_, scipy_zgeqrf_, scipy_zungqr_, scipy_zgemm_), resolved at run time with dlopen: the Python
// side passes the library's path (qkb_init).  Reference semantics: gpu_backend/kernel_state_ansatz.py:141-144, 221
// (MPSxGate, truncation_fidelity) and KernelPkg.jl:68 (cutoff).
#include "qk_builder.h"
#include "qk_program.h"

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

// The branch of channel gate i with the probabilities p[m] (tot = p_0 + .. in ascending order): the forced one, or drawn: the first k
// with p_k > 0 and u tot < p_0 + .. + p_k, else the last k with p_k > 0, u the uniform of counter (first_gate + i, trajectory,
// state_index, 2); `margin` takes the smallest |u tot - cum| / tot over the thresholds.  -1 with g_err set when the outcome is
// impossible: tot 0 or not finite in a draw, p_b 0 or not finite.
int channel_branch(const qk_program& prog, int i, int forced, int m, const double* p, double* margin) {
  double tot = 0;
  for (int k = 0; k < m; ++k) tot += p[k];
  const uint32_t state = prog.state_index ? prog.state_index[0] : 0u, trajectory = prog.trajectory ? prog.trajectory[0] : 0u;
  const auto at = [&] { return "state " + std::to_string(state) + ", gate " + std::to_string(prog.first_gate + (uint32_t)i) + ": "; };  // error paths only
  int b = forced;
  if (forced < 0) {
    if (!(tot > 0.0) || !std::isfinite(tot)) {
      g_err = at() + "the branch probabilities of the channel sum to 0 or are not finite";
      return -1;
    }
    const double u = channel_uniform(prog.seed, prog.first_gate + (uint32_t)i, trajectory, state);
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

uint32_t qkb_program_size(void) { return (uint32_t)sizeof(qk_program); }
uint32_t qkb_run_size(void) { return (uint32_t)sizeof(qkb_run); }
uint32_t qkb_result_size(void) { return (uint32_t)sizeof(qkb_result); }

static int simulate_impl(const qk_program& prog, const qkb_run& run, qkb_result* res);

// -8 with g_err set, for the checks in front of simulate_impl
static int refuse(const std::string& why) {
  g_err = why;
  return -8;
}

int qkb_simulate_program(const qk_program* program, const qkb_run* run, qkb_result* res) {
  if (!program || !run || !res) return refuse("qkb_simulate_program: null argument");
  if (program->size != sizeof(qk_program) || run->size != sizeof(qkb_run) || res->size != sizeof(qkb_result))
    return refuse("qkb_simulate_program: the sizes of qk_program, qkb_run, qkb_result are " + std::to_string(program->size) + ", " + std::to_string(run->size) + ", " +
                  std::to_string(res->size) + ", this library's are " + std::to_string(sizeof(qk_program)) + ", " + std::to_string(sizeof(qkb_run)) + ", " + std::to_string(sizeof(qkb_result)));
  const qk_program& p = *program;
  if (p.n_states != 1 || p.n_qubits < 1 || p.n_ops < 0 || !res->dims || (p.n_ops > 0 && (!p.op || !p.q0 || !p.alpha)))
    return refuse("qkb_simulate_program: one state of at least one qubit, with op, q0, alpha and dims");
  if (run->init_dims) {
    const int n = p.n_qubits;
    if (!run->init_tensors) return refuse("an initial state needs init_dims and init_tensors");
    if (run->init_dims[0] != 1 || run->init_dims[n] != 1) return refuse("the initial state's boundary bonds must be 1");
    size_t total = 0;
    for (int k = 0; k <= n; ++k) {
      if (run->init_dims[k] <= 0) return refuse("the initial state's bond " + std::to_string(k) + " is " + std::to_string((int)run->init_dims[k]) + ": bonds must be positive");
      if (k < n) total += (size_t)run->init_dims[k] * 2 * (size_t)std::max(run->init_dims[k + 1], 0);
    }
    if (run->init_centre < 0 || run->init_centre >= n)
      return refuse("the initial state's centre " + std::to_string((int)run->init_centre) + " lies outside the register of " + std::to_string(n));
    for (size_t e = 0; e < 2 * total; ++e)
      if (!std::isfinite(run->init_tensors[e])) return refuse("the initial state has an entry that is not finite");
    if (!std::isfinite(run->init_fidelity) || !std::isfinite(run->init_logw)) return refuse("the initial state's fidelity or log-weight is not finite");
  }
  std::string wrong;
  if (!qk_program_check_tables(p, &wrong)) return refuse(wrong);
  return simulate_impl(p, *run, res);
}
}  // extern "C"

// the gates of `prog` (its tables are there: qkb_simulate_program) on |0...0>, or on the initial state of `run`, which is valid
static int simulate_impl(const qk_program& prog, const qkb_run& run, qkb_result* res) {
  if (!p_zgesdd) {
    g_err = "qkb_init has not been called";
    return -1;
  }
  const int n = prog.n_qubits, n_ops = prog.n_ops;
  const int8_t* const op = prog.op;
  const int32_t *const q0 = prog.q0, *const mat = prog.mat;
  const double* const alpha = prog.alpha;
  const cd* const mats = reinterpret_cast<const cd*>(prog.mats);
  if (const int bad = qk_program_check(prog, &g_err)) return bad == QK_PROGRAM_UNKNOWN_OP ? -7 : bad == QK_PROGRAM_MATRIX_GATE_OUTSIDE ? -3 : -8;
  double logw = 0.0, margin = INFINITY;
  int n_drawn = 0;  // channel gates done: the index into res->branches
  std::vector<int> taken(prog.cond_gate ? n_ops : 0, -1);  // the branch every channel gate of this state took (-2: skipped), by position
  std::vector<Tensor> A(n);
  for (auto& t : A) t.v = {cd(1, 0), cd(0, 0)};
  std::vector<int> two_q_pos;
  for (int i = 0; i < n_ops; ++i)
    if (is_two_qubit(op[i])) two_q_pos.push_back(q0[i]);
  double fidelity = 1.0;
  int centre = 0;  // sites < centre are left-orthonormal, sites > centre right-orthonormal
  if (run.init_dims) {  // the run goes on from a given state: its sites, centre, fidelity and log-weight
    const cd* src = reinterpret_cast<const cd*>(run.init_tensors);
    for (int k = 0; k < n; ++k) {
      A[k].l = run.init_dims[k], A[k].r = run.init_dims[k + 1];
      const size_t cnt = (size_t)A[k].l * 2 * A[k].r;
      A[k].v.assign(src, src + cnt);
      src += cnt;
    }
    centre = run.init_centre, fidelity = run.init_fidelity, logw = run.init_logw;
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
    if (prog.cond_gate && prog.cond_gate[i] >= 0) {  // a gate whose condition is false does nothing at all; it is a done gate all the same
      const int b = taken[prog.cond_gate[i]];
      if (b < 0 || !((prog.cond_mask[i] >> b) & 1u)) {
        if (o == OP_K1 || o == OP_K2) {
          taken[i] = -2;
          if (res->branches) res->branches[n_drawn] = -2;
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
      const int c = prog.channel[i], forced = prog.branch[i], m = prog.n_kraus[c];
      const cd* K = reinterpret_cast<const cd*>(prog.kraus) + (size_t)c * 16;
      Tensor& t = A[q];
      double N = 0, p[4] = {0, 0, 0, 0};
      for (int a = 0; a < t.l; ++a)  // every sum in ascending order of (a, c)
        for (int x = 0; x < t.r; ++x) {
          const cd v[2] = {t.at(a, 0, x), t.at(a, 1, x)};
          N += std::norm(v[0]) + std::norm(v[1]);
          for (int k = 0; k < m; ++k) p[k] += std::norm(mat_dot(K + k * 4, v, 2)) + std::norm(mat_dot(K + k * 4 + 2, v, 2));
        }
      const int b = channel_branch(prog, i, forced, m, p, &margin);
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
      if (res->branches) res->branches[n_drawn] = (int8_t)b;
      if (prog.cond_gate) taken[i] = b;
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
      const int c = prog.channel[i], forced = prog.branch[i], nk = prog.n_kraus2[c];
      const cd* K = reinterpret_cast<const cd*>(prog.kraus2) + (size_t)c * 256;
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
      const int b = channel_branch(prog, i, forced, nk, p, &margin);
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
      if (res->branches) res->branches[n_drawn] = (int8_t)b;
      if (prog.cond_gate) taken[i] = b;
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
    int keep = kept(S, run.trunc_budget, run.value_of_zero, &frac);
    if (run.max_bond > 0 && keep > run.max_bond) {  // the chi cap
      keep = run.max_bond;
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
  res->dims[0] = 1;
  for (int k2 = 0; k2 < n; ++k2) {
    res->dims[k2 + 1] = A[k2].r;
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
  res->tensors = reinterpret_cast<double*>(block), res->n_complex = total;
  res->fidelity = fidelity, res->logw = logw, res->margin = margin;
  return 0;
}

extern "C" {
void qkb_free(double* p) { std::free(p); }

}  // extern "C"
