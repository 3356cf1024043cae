// Host-only sanitizer driver for the matrix gates of the native host MPS builder (qk_builder.cpp: qkb_simulate_program, spelt qkb_simulate_gates in tests/host_san/qkb_calls.h), built with
// -fsanitize=address,undefined and run by tests/test_matrix_gates_san.py in the CPU tier.  A 6-qubit program with both matrix codes
// (8: a 2x2, 9: a 4x4), a pair given in reversed order and the named rotations in between is checked against a dense loop in this
// file, then run with a bond cap, and every rejection must come back as its code.  argv[1]: the OpenBLAS scipy ships.
// Test infrastructure: nothing of the product links it.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

using cd = std::complex<double>;

#include "qkb_calls.h"

namespace {
constexpr int N = 6, DIM = 1 << N;
using M2 = std::vector<cd>;  // row-major d x d

M2 u2(double th, double ph, double la) {  // a general 2x2 unitary
  return {cd(std::cos(th), 0), -std::polar(1.0, la) * std::sin(th), std::polar(1.0, ph) * std::sin(th), std::polar(1.0, ph + la) * std::cos(th)};
}
M2 kron(const M2& a, const M2& b) {
  M2 o(16);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k)
        for (int l = 0; l < 2; ++l) o[(size_t)(i * 2 + k) * 4 + (j * 2 + l)] = a[(size_t)i * 2 + j] * b[(size_t)k * 2 + l];
  return o;
}
M2 mul4(const M2& a, const M2& b) {
  M2 o(16, cd(0, 0));
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k) o[(size_t)i * 4 + j] += a[(size_t)i * 4 + k] * b[(size_t)k * 4 + j];
  return o;
}
M2 u4(int seed) {  // (A x B) CX (C x D): not symmetric in its qubits
  const double s = 0.37 * seed;
  const M2 cx = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0};
  return mul4(mul4(kron(u2(0.3 + s, 0.5, -0.2 * s), u2(1.1, s, 0.4)), cx), kron(u2(0.7 * s, -0.9, 0.1), u2(0.2, 0.3 + s, 1.3)));
}
M2 exchange(const M2& m) {  // M'[(t,s)][(t',s')] = M[(s,t)][(s',t')]
  M2 o(16);
  for (int s = 0; s < 2; ++s)
    for (int t = 0; t < 2; ++t)
      for (int s2 = 0; s2 < 2; ++s2)
        for (int t2 = 0; t2 < 2; ++t2) o[(size_t)(t * 2 + s) * 4 + (t2 * 2 + s2)] = m[(size_t)(s * 2 + t) * 4 + (s2 * 2 + t2)];
  return o;
}

// dense loop: qubit 0 is the most significant bit of the index
void dense1(std::vector<cd>& psi, const M2& m, int q) {
  const int b = 1 << (N - 1 - q);
  for (int i = 0; i < DIM; ++i)
    if (!(i & b)) {
      const cd x = psi[(size_t)i], y = psi[(size_t)(i | b)];
      psi[(size_t)i] = m[0] * x + m[1] * y;
      psi[(size_t)(i | b)] = m[2] * x + m[3] * y;
    }
}
void dense2(std::vector<cd>& psi, const M2& m, int qa, int qb) {  // index (s_qa, s_qb), qa most significant
  const int ba = 1 << (N - 1 - qa), bb = 1 << (N - 1 - qb);
  for (int i = 0; i < DIM; ++i)
    if (!(i & ba) && !(i & bb)) {
      const int idx[4] = {i, i | bb, i | ba, i | ba | bb};
      cd v[4], w[4];
      for (int k = 0; k < 4; ++k) v[k] = psi[(size_t)idx[k]];
      for (int r = 0; r < 4; ++r) {
        w[r] = 0;
        for (int k = 0; k < 4; ++k) w[r] += m[(size_t)r * 4 + k] * v[k];
      }
      for (int k = 0; k < 4; ++k) psi[(size_t)idx[k]] = w[k];
    }
}

struct Program {
  std::vector<int8_t> op;
  std::vector<int32_t> q0, mat;
  std::vector<double> alpha;
  std::vector<cd> mats;  // [n_mats][4][4]
  std::vector<cd> want = std::vector<cd>(DIM, cd(0, 0));
  Program() { want[0] = 1; }
  int n_mats() const { return (int)(mats.size() / 16); }
  void named(int code, int q, double a, const M2& dense) {
    op.push_back((int8_t)code), q0.push_back(q), alpha.push_back(a), mat.push_back(-1);
    if (dense.size() == 4) dense1(want, dense, q);
    else dense2(want, dense, q, q + 1);
  }
  void m1(int q, const M2& m) {
    op.push_back(8), q0.push_back(q), alpha.push_back(0), mat.push_back(n_mats());
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) mats.push_back(r < 2 && c < 2 ? m[(size_t)r * 2 + c] : cd(0, 0));
    dense1(want, m, q);
  }
  void m2(int qa, int qb, const M2& m) {  // adjacent qubits in either order: reversed, the table holds the exchanged matrix
    op.push_back(9), q0.push_back(std::min(qa, qb)), alpha.push_back(0), mat.push_back(n_mats());
    const M2 t = qa < qb ? m : exchange(m);
    mats.insert(mats.end(), t.begin(), t.end());
    dense2(want, m, qa, qb);
  }
};

M2 rz(double a) { return {std::polar(1.0, -0.5 * M_PI * a), 0, 0, std::polar(1.0, 0.5 * M_PI * a)}; }
M2 ry(double a) { return {std::cos(0.5 * M_PI * a), -std::sin(0.5 * M_PI * a), std::sin(0.5 * M_PI * a), std::cos(0.5 * M_PI * a)}; }

int run(const Program& p, int cap, std::vector<int32_t>& dims, std::vector<cd>& psi, double* fid, const std::vector<cd>* mats = nullptr, const std::vector<int32_t>* mat = nullptr,
        int n_mats = -1) {
  double* block = nullptr;
  int64_t nc = 0;
  dims.assign(N + 1, 0);
  const std::vector<cd>& mm = mats ? *mats : p.mats;
  const std::vector<int32_t>& mi = mat ? *mat : p.mat;
  const int rc = qkb_simulate_gates(N, (int)p.op.size(), p.op.data(), p.q0.data(), p.alpha.data(), 1e-16, 1e-16, cap, n_mats < 0 ? p.n_mats() : n_mats,
                                    reinterpret_cast<const double*>(mm.data()), mi.data(), dims.data(), &block, &nc, fid);
  if (rc != 0) return rc;
  // contract the chain into the dense vector
  const cd* t = reinterpret_cast<const cd*>(block);
  std::vector<cd> v(1, cd(1, 0));  // [index][bond]
  int rows = 1;
  for (int k = 0; k < N; ++k) {
    const int l = dims[(size_t)k], r = dims[(size_t)k + 1];
    std::vector<cd> w((size_t)rows * 2 * r, cd(0, 0));
    for (int i = 0; i < rows; ++i)
      for (int a = 0; a < l; ++a)
        for (int s = 0; s < 2; ++s)
          for (int c = 0; c < r; ++c) w[((size_t)i * 2 + s) * r + c] += v[(size_t)i * l + a] * t[((size_t)a * 2 + s) * r + c];
    t += (size_t)l * 2 * r;
    v.swap(w);
    rows *= 2;
  }
  psi = v;
  qkb_free(block);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("matrix gates: no OpenBLAS given, nothing to run\n");
    return 0;
  }
  if (qkb_init(argv[1]) != 0) {
    fprintf(stderr, "qkb_init: %s\n", qkb_last_error());
    return 30;
  }
  const M2 h = {M_SQRT1_2, M_SQRT1_2, M_SQRT1_2, -M_SQRT1_2};
  Program p;
  for (int q = 0; q < N; ++q) p.named(0, q, 0, h);
  for (int layer = 0; layer < 3; ++layer) {
    for (int a = layer % 2; a + 1 < N; a += 2) {
      if ((a + layer) % 3 == 1) p.m2(a + 1, a, u4(3 * layer + a));  // a reversed pair
      else p.m2(a, a + 1, u4(3 * layer + a));
    }
    for (int q = 0; q < N; ++q) {
      if (q % 2) p.named(1, q, 0.3 + 0.1 * q, rz(0.3 + 0.1 * q));
      else p.named(5, q, -0.2 + 0.15 * q, ry(-0.2 + 0.15 * q));
    }
    p.m1(layer, u2(0.4 + layer, 0.9, -0.3 * layer));
    p.m1(N - 1, u2(1.0, 0.2 * layer, 0.6));  // a one-qubit matrix on the last qubit is in range
  }
  std::vector<int32_t> dims;
  std::vector<cd> psi;
  double fid = 0;
  int rc = run(p, 0, dims, psi, &fid);
  if (rc != 0) {
    fprintf(stderr, "qkb_simulate_gates: %d %s\n", rc, qkb_last_error());
    return 31;
  }
  double err = 0;
  for (int i = 0; i < DIM; ++i) err = std::max(err, std::abs(psi[(size_t)i] - p.want[(size_t)i]));
  const int chi = *std::max_element(dims.begin(), dims.end());
  printf("matrix gates: %d qubits, %zu gates, %d matrices: max bond %d, fidelity %.17g, max |psi - dense| = %.3e\n", N, p.op.size(), p.n_mats(), chi, fid, err);
  if (!(err <= 1e-12) || chi < 4 || std::abs(fid - 1) > 1e-12) return 32;
  rc = run(p, 2, dims, psi, &fid);  // the bond cap
  if (rc != 0 || *std::max_element(dims.begin(), dims.end()) != 2 || !(fid > 0 && fid < 1 - 1e-3)) return 33;
  double nrm = 0;
  for (const cd& x : psi) nrm += std::norm(x);
  printf("matrix gates: capped at 2: fidelity %.17g, norm %.17g\n", fid, nrm);
  if (std::abs(nrm - 1) > 1e-12) return 34;

  // every rejection returns its code, before a gate is applied
  const int first2 = (int)(std::find(p.op.begin(), p.op.end(), (int8_t)9) - p.op.begin());
  const int first1 = (int)(std::find(p.op.begin(), p.op.end(), (int8_t)8) - p.op.begin());
  if (run(p, 0, dims, psi, &fid, nullptr, nullptr, 0) != -7) return 40;  // codes 8 and 9 without a table: unknown op codes
  {
    std::vector<int32_t> dims2((size_t)N + 1);
    double* block = nullptr;
    int64_t nc = 0;
    if (qkb_simulate_chi(N, (int)p.op.size(), p.op.data(), p.q0.data(), p.alpha.data(), 1e-16, 1e-16, 0, dims2.data(), &block, &nc, &fid) != -7) return 41;  // the old entry
  }
  {
    std::vector<int32_t> bad = p.mat;
    bad[(size_t)first2] = p.n_mats();
    if (run(p, 0, dims, psi, &fid, nullptr, &bad) != -8) return 42;  // index out of range
    bad[(size_t)first2] = -1;
    if (run(p, 0, dims, psi, &fid, nullptr, &bad) != -8) return 43;
  }
  {
    std::vector<cd> bad = p.mats;
    cd* m = bad.data() + (size_t)p.mat[(size_t)first1] * 16;
    m[0] = 1, m[1] = 1, m[4] = 0, m[5] = 1;  // [[1, 1], [0, 1]]
    if (run(p, 0, dims, psi, &fid, &bad) != -8) return 44;  // not unitary
    bad = p.mats;
    bad[(size_t)p.mat[(size_t)first2] * 16 + 6] = cd(std::numeric_limits<double>::quiet_NaN(), 0);
    if (run(p, 0, dims, psi, &fid, &bad) != -8) return 45;  // NaN
    bad = p.mats;
    for (int k = 0; k < 16; ++k) bad[(size_t)p.mat[(size_t)first2] * 16 + k] *= 1.0 + 1e-9;
    if (run(p, 0, dims, psi, &fid, &bad) != -8) return 46;  // off unitary by 2e-9
  }
  {
    Program q = p;
    q.q0[(size_t)first2] = N - 1;
    if (run(q, 0, dims, psi, &fid) != -3) return 47;  // a 4x4 on (n-1, n)
    q = p;
    q.op[(size_t)first2] = 10;
    if (run(q, 0, dims, psi, &fid) != -7) return 48;  // an op code beyond the table's two
  }
  printf("matrix gates: 9 rejections ok (%s)\n", qkb_last_error());
  return 0;
}
