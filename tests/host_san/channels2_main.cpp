// Host-only sanitizer driver for the two-qubit Kraus channels of the native host MPS builder (qk_builder.cpp: qkb_simulate_program, spelt qkb_simulate_channels2 in tests/host_san/qkb_calls.h),
// built with -fsanitize=address,undefined and run by tests/test_channels2_san.py in the CPU tier.  The enumeration case: a 6-qubit
// entangling program with a two-qubit depolarising channel on the interior pair (1, 2) while the orthogonality centre sits on (4, 5)
// and a correlated phase flip on the last pair, its 16 x 2 forced branch sequences summed to the density matrix of a dense Kraus map
// written in this file; then drawn trajectories and their replay, a capped build, and every rejection must come back as its code.
// argv[1]: the OpenBLAS scipy ships.  Test infrastructure: nothing of the product links it.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using cd = std::complex<double>;

#include "qkb_calls.h"

namespace {
constexpr int N = 6, DIM = 1 << N;
using M2 = std::vector<cd>;  // row-major d x d

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
void dense2(std::vector<cd>& psi, const M2& m, int qa) {  // on (qa, qa + 1), qa most significant
  const int ba = 1 << (N - 1 - qa), bb = ba >> 1;
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
M2 kron(const M2& a, const M2& b, cd f) {
  M2 o(16);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k)
        for (int l = 0; l < 2; ++l) o[(size_t)(i * 2 + k) * 4 + (j * 2 + l)] = f * a[(size_t)i * 2 + j] * b[(size_t)k * 2 + l];
  return o;
}
const M2 I2 = {1, 0, 0, 1}, X = {0, 1, 1, 0}, Y = {0, cd(0, -1), cd(0, 1), 0}, Z = {1, 0, 0, -1};
M2 pauli_phase(double a, const M2& p) {  // cos(th) 1 - i sin(th) P (x) P, th = pi a / 2
  const double th = 0.5 * M_PI * a;
  M2 o = kron(p, p, cd(0, -std::sin(th)));
  for (int i = 0; i < 4; ++i) o[(size_t)i * 5] += std::cos(th);
  return o;
}
// the Kraus matrices of the two channels, written out here
std::vector<M2> depolarizing2(double p) {  // sqrt(1 - 15p/16) I(x)I, sqrt(p/16) P(x)Q, P-major over I, X, Y, Z
  const M2* pa[4] = {&I2, &X, &Y, &Z};
  std::vector<M2> k;
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) k.push_back(kron(*pa[a], *pa[b], a + b == 0 ? std::sqrt(1 - 15 * p / 16) : std::sqrt(p / 16)));
  return k;
}
std::vector<M2> correlated_flip(double p) { return {kron(I2, I2, std::sqrt(1 - p)), kron(Z, Z, std::sqrt(p))}; }

struct Gate {
  int code, q;
  double a;
};
// H 0, XX(0,1), Ry 2, XX(1,2), XX(2,3), YY(3,4), XX(4,5), Rx 5, ZZ(4,5) leave the centre on (4, 5); then the depolarising channel on
// (1, 2), more gates, the correlated flip on the last pair, and a gate at the far end
const Gate PROGRAM[] = {{0, 0, 0},   {2, 0, 0.5}, {5, 2, 0.3},  {2, 1, 0.4}, {2, 2, 0.3}, {6, 3, 0.45}, {2, 4, 0.35}, {4, 5, 0.7},
                        {7, 4, 0.6}, {11, 1, 0},  {7, 2, 0.25}, {5, 5, 0.4}, {11, 4, 0},  {6, 0, 0.2}};
constexpr int AT0 = 9, AT1 = 12;

M2 dense_matrix(const Gate& g) {
  const double th = 0.5 * M_PI * g.a, c = std::cos(th), s = std::sin(th), h = std::sqrt(0.5);
  switch (g.code) {
    case 0: return {h, h, h, -h};
    case 4: return {c, cd(0, -s), cd(0, -s), c};
    case 5: return {c, -s, s, c};
    case 2: return pauli_phase(g.a, X);
    case 6: return pauli_phase(g.a, Y);
    default: {  // 7: ZZPhase
      M2 o(16, cd(0, 0));
      o[0] = o[15] = std::polar(1.0, -th), o[5] = o[10] = std::polar(1.0, th);
      return o;
    }
  }
}

struct Tables {
  std::vector<int8_t> op;
  std::vector<int32_t> q0, channel, branch, n_kraus2;
  std::vector<double> alpha;
  std::vector<cd> kraus2;  // [n_channels2][16][4][4]
};

Tables tables() {
  Tables t;
  for (const Gate& x : PROGRAM) {
    t.op.push_back((int8_t)x.code), t.q0.push_back(x.q), t.alpha.push_back(x.a), t.branch.push_back(-1);
    t.channel.push_back(x.code == 11 ? (int32_t)t.n_kraus2.size() : -1);
    if (x.code == 11) {  // a slot per gate
      const std::vector<M2> k = t.n_kraus2.empty() ? depolarizing2(0.3) : correlated_flip(0.2);
      std::vector<cd> slot(256, cd(0, 0));
      for (size_t j = 0; j < k.size(); ++j) std::copy(k[j].begin(), k[j].end(), slot.begin() + 16 * (long)j);
      t.kraus2.insert(t.kraus2.end(), slot.begin(), slot.end());
      t.n_kraus2.push_back((int32_t)k.size());
    }
  }
  return t;
}

struct Result {
  int rc = 0;
  std::vector<cd> psi;
  std::vector<int32_t> dims = std::vector<int32_t>(N + 1, 0);
  std::vector<int8_t> branches = std::vector<int8_t>(4, (int8_t)-9);  // the programs here hold two channel gates
  double fidelity = 0, logw = 0, margin = 0;
};

Result run(const Tables& t, int max_bond, uint64_t seed, uint32_t state, uint32_t traj, uint32_t first, int n_channels2 = -1) {
  Result r;
  double* block = nullptr;
  int64_t count = 0;
  const int nc = n_channels2 < 0 ? (int)t.n_kraus2.size() : n_channels2;
  r.rc = qkb_simulate_channels2(N, (int)t.op.size(), t.op.data(), t.q0.data(), t.alpha.data(), 0.0, 1e-16, max_bond, 0, nullptr, nullptr, 0, nullptr, nullptr, t.channel.data(),
                                t.branch.data(), seed, state, traj, first, nc, reinterpret_cast<const double*>(t.kraus2.data()), t.n_kraus2.data(), r.dims.data(), &block, &count,
                                &r.fidelity, &r.logw, r.branches.data(), &r.margin);
  if (r.rc != 0) return r;
  // contract the chain into the dense vector
  const cd* a = reinterpret_cast<const cd*>(block);
  std::vector<cd> v(1, cd(1, 0));
  size_t rows = 1;
  for (int k = 0; k < N; ++k) {
    const int l = r.dims[(size_t)k], rr = r.dims[(size_t)k + 1];
    std::vector<cd> w(rows * 2 * (size_t)rr, cd(0, 0));
    for (size_t i = 0; i < rows; ++i)
      for (int x = 0; x < l; ++x)
        for (int p = 0; p < 2; ++p)
          for (int c = 0; c < rr; ++c) w[(i * 2 + (size_t)p) * (size_t)rr + (size_t)c] += v[i * (size_t)l + (size_t)x] * a[((size_t)x * 2 + (size_t)p) * (size_t)rr + (size_t)c];
    a += (size_t)l * 2 * (size_t)rr;
    v.swap(w);
    rows *= 2;
  }
  qkb_free(block);
  r.psi = v;
  return r;
}

int fail(const char* what) {
  std::printf("FAILED: %s (%s)\n", what, qkb_last_error());
  return 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || qkb_init(argv[1]) != 0) return fail("qkb_init");
  const Tables t = tables();
  const std::vector<M2> k0 = depolarizing2(0.3), k1 = correlated_flip(0.2);
  // the dense Kraus map: rho = sum over the 32 branch sequences of |phi><phi| with phi the unnormalised branch vector
  std::vector<cd> want((size_t)DIM * DIM, cd(0, 0)), got((size_t)DIM * DIM, cd(0, 0));
  double total = 0;
  for (int b0 = 0; b0 < 16; ++b0)
    for (int b1 = 0; b1 < 2; ++b1) {
      std::vector<cd> phi((size_t)DIM, cd(0, 0));
      phi[0] = 1;
      int j = 0;
      for (const Gate& x : PROGRAM) {
        if (x.code == 11) dense2(phi, j++ == 0 ? k0[(size_t)b0] : k1[(size_t)b1], x.q);
        else if (x.code == 2 || x.code == 6 || x.code == 7) dense2(phi, dense_matrix(x), x.q);
        else dense1(phi, dense_matrix(x), x.q);
      }
      for (int i = 0; i < DIM; ++i)
        for (int k = 0; k < DIM; ++k) want[(size_t)i * DIM + k] += phi[(size_t)i] * std::conj(phi[(size_t)k]);
      Tables f = t;
      f.branch[AT0] = b0, f.branch[AT1] = b1;
      const Result r = run(f, 0, 0, 0, 0, 0);
      if (r.rc != 0) return fail("forced run");
      if (r.branches[0] != b0 || r.branches[1] != b1) return fail("recorded branches");
      const double w = std::exp(r.logw);
      total += w;
      for (int i = 0; i < DIM; ++i)
        for (int k = 0; k < DIM; ++k) got[(size_t)i * DIM + k] += w * r.psi[(size_t)i] * std::conj(r.psi[(size_t)k]);
    }
  double worst = 0;
  for (size_t e = 0; e < want.size(); ++e) worst = std::max(worst, std::abs(want[e] - got[e]));
  std::printf("max |rho - dense| = %.3e, sum of weights - 1 = %.3e\n", worst, total - 1);
  if (!(worst < 1e-12) || !(std::fabs(total - 1) < 1e-12)) return fail("enumeration");
  // drawn trajectories: run to run the same, the replay of the recorded branches bit-identical
  int differ = 0;
  Result first_r;
  for (uint32_t traj = 0; traj < 6; ++traj) {
    const Result a = run(t, 0, 77, 3, traj, 5), b = run(t, 0, 77, 3, traj, 5);
    if (a.rc != 0 || b.rc != 0) return fail("drawn run");
    if (a.logw != b.logw || std::memcmp(a.psi.data(), b.psi.data(), a.psi.size() * sizeof(cd)) != 0) return fail("run to run");
    Tables f = t;
    f.branch[AT0] = a.branches[0], f.branch[AT1] = a.branches[1];
    const Result c = run(f, 0, 1, 9, 9, 0);
    if (c.rc != 0 || c.logw != a.logw || std::memcmp(a.psi.data(), c.psi.data(), a.psi.size() * sizeof(cd)) != 0) return fail("replay");
    if (!(a.margin > 0) || !(c.margin == std::numeric_limits<double>::infinity())) return fail("margin");
    if (traj == 0) first_r = a;
    else differ += (a.branches[0] != first_r.branches[0] || a.branches[1] != first_r.branches[1]);
  }
  std::printf("6 trajectories replayed, %d differ from the first\n", differ);
  // a capped build
  const Result capped = run(t, 2, 77, 3, 0, 0);
  if (capped.rc != 0) return fail("capped run");
  if (*std::max_element(capped.dims.begin(), capped.dims.end()) > 2 || !(capped.fidelity < 1.0)) return fail("cap");
  std::printf("capped at 2: fidelity %.6f\n", capped.fidelity);
  // without a two-qubit table the call is qkb_simulate_channels, and that without a table qkb_simulate_gates: code 11 is unknown (-7)
  int rejected = 0;
  rejected += run(t, 0, 0, 0, 0, 0, 0).rc == -7;
  auto bad = [&](auto edit, int want_rc) {
    Tables f = tables();
    edit(f);
    const Result r = run(f, 0, 0, 0, 0, 0);
    if (r.rc != want_rc) std::printf("expected %d, got %d (%s)\n", want_rc, r.rc, r.rc ? qkb_last_error() : "");
    return r.rc == want_rc ? 1 : 0;
  };
  rejected += bad([](Tables& f) { f.channel[AT0] = 2; }, -8);
  rejected += bad([](Tables& f) { f.channel[AT1] = -1; }, -8);
  rejected += bad([](Tables& f) { f.n_kraus2[0] = 0; }, -8);
  rejected += bad([](Tables& f) { f.n_kraus2[1] = 17; }, -8);
  rejected += bad([](Tables& f) { f.kraus2[256 + 21] = cd(std::nan(""), 0); }, -8);
  rejected += bad([](Tables& f) { f.branch[AT0] = 16; }, -8);
  rejected += bad([](Tables& f) { f.branch[AT1] = -2; }, -8);
  rejected += bad([](Tables& f) { f.kraus2[16 + 1] *= 1 + 2e-9; }, -8);  // drawn and not trace preserving
  rejected += bad([](Tables& f) { f.q0[AT1] = N - 1; }, -8);                // the pair (5, 6) is outside the register
  rejected += bad([](Tables& f) { f.kraus2[16 + 1] *= 1 + 2e-9, f.branch[AT0] = 7; }, 0);  // forced: any finite matrix
  {  // an impossible outcome: the first gate is the flip channel forced to a branch whose matrix is 0 on this state
    Tables f = tables();
    std::fill(f.kraus2.begin() + 256 + 16, f.kraus2.begin() + 256 + 32, cd(0, 0));
    f.kraus2[256 + 16 + 15] = 1;  // |11><11|: |00> has no weight there
    f.op[0] = 11, f.q0[0] = 4, f.channel[0] = 1, f.branch[0] = 1, f.branch[AT1] = 0;  // (both forced: the edited table is no channel)
    const Result r = run(f, 0, 0, 4, 0, 30);
    rejected += r.rc == -9 && std::strstr(qkb_last_error(), "state 4, gate 30") != nullptr;
  }
  std::printf("%d rejections ok\n", rejected);
  return rejected == 12 ? 0 : 1;
}
