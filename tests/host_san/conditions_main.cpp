// Host-only sanitizer driver for classical control in the native host MPS builder (qk_builder.cpp: qkb_simulate_program, spelt qkb_simulate_conditions in tests/host_san/qkb_calls.h), built
// with -fsanitize=address,undefined and run by tests/test_conditions_san.py in the CPU tier.  Teleportation on 3 qubits (the four
// forced outcome patterns and drawn trajectories: qubit 2 carries the Bloch vector of the state prepared on qubit 0); the exact
// enumeration of a 4-qubit program that mixes codes 10 and 11 with conditional gates and conditional channels, every classical
// record (-2 where a channel gate is skipped) summed to the density matrix of a dense branch loop written in this file; and every
// rejection must come back as -8 naming the gate.  argv[1]: the OpenBLAS scipy ships.  Test infrastructure: nothing of the product
// links it.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using cd = std::complex<double>;

#include "qkb_calls.h"

namespace {
using M = std::vector<cd>;  // row-major d x d

// dense loop on n qubits: qubit 0 is the most significant bit of the index
void dense1(std::vector<cd>& psi, int n, const cd* m, int q) {
  const int b = 1 << (n - 1 - q);
  for (int i = 0; i < (1 << n); ++i)
    if (!(i & b)) {
      const cd x = psi[(size_t)i], y = psi[(size_t)(i | b)];
      psi[(size_t)i] = m[0] * x + m[1] * y;
      psi[(size_t)(i | b)] = m[2] * x + m[3] * y;
    }
}
void dense2(std::vector<cd>& psi, int n, const cd* m, int qa) {  // on (qa, qa + 1), qa most significant
  const int ba = 1 << (n - 1 - qa), bb = ba >> 1;
  for (int i = 0; i < (1 << n); ++i)
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
M kron(const M& a, const M& b, cd f) {
  M o(16);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k)
        for (int l = 0; l < 2; ++l) o[(size_t)(i * 2 + k) * 4 + (j * 2 + l)] = f * a[(size_t)i * 2 + j] * b[(size_t)k * 2 + l];
  return o;
}
const M I2 = {1, 0, 0, 1}, X = {0, 1, 1, 0}, Y = {0, cd(0, -1), cd(0, 1), 0}, Z = {1, 0, 0, -1};
const M CX = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0};
M pauli_phase(double a, const M& p) {  // cos(th) 1 - i sin(th) P (x) P, th = pi a / 2
  const double th = 0.5 * M_PI * a;
  M o = kron(p, p, cd(0, -std::sin(th)));
  for (int i = 0; i < 4; ++i) o[(size_t)i * 5] += std::cos(th);
  return o;
}

// one gate of a program: the op code, the qubit (pair), the angle, the matrix (codes 8, 9) or the Kraus matrices (codes 10, 11), the
// condition (-1: none)
struct Gate {
  int code, q;
  double a;
  std::vector<M> ms;
  int cond = -1;
  uint32_t mask = 0;
};

M dense_matrix(const Gate& g) {
  const double th = 0.5 * M_PI * g.a, c = std::cos(th), s = std::sin(th), h = std::sqrt(0.5);
  switch (g.code) {
    case 0: return {h, h, h, -h};
    case 1: return {std::polar(1.0, -th), 0, 0, std::polar(1.0, th)};
    case 4: return {c, cd(0, -s), cd(0, -s), c};
    case 5: return {c, -s, s, c};
    case 2: return pauli_phase(g.a, X);
    case 6: return pauli_phase(g.a, Y);
    case 7: {
      M o(16, cd(0, 0));
      o[0] = o[15] = std::polar(1.0, -th), o[5] = o[10] = std::polar(1.0, th);
      return o;
    }
    default: return g.ms[0];  // 8, 9
  }
}
bool two_qubit(int code) { return code == 2 || code == 6 || code == 7 || code == 9 || code == 11; }

struct Tables {
  int n = 0;
  std::vector<int8_t> op;
  std::vector<int32_t> q0, mat, channel, branch, n_kraus, n_kraus2, cond_gate;
  std::vector<uint32_t> cond_mask;
  std::vector<double> alpha;
  std::vector<cd> mats, kraus, kraus2;  // [n_mats][4][4], [n_channels][4][2][2], [n_channels2][16][4][4]
};

Tables tables(int n, const std::vector<Gate>& prog) {
  Tables t;
  t.n = n;
  for (const Gate& g : prog) {
    t.op.push_back((int8_t)g.code), t.q0.push_back(g.q), t.alpha.push_back(g.a), t.branch.push_back(-1), t.cond_gate.push_back(g.cond), t.cond_mask.push_back(g.mask);
    t.mat.push_back(-1), t.channel.push_back(-1);
    if (g.code == 8 || g.code == 9) {  // a slot per gate; a 2x2 sits in [:2][:2]
      const int d = g.code == 8 ? 2 : 4;
      t.mat.back() = (int32_t)(t.mats.size() / 16);
      std::vector<cd> slot(16, cd(0, 0));
      for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c) slot[(size_t)r * 4 + c] = g.ms[0][(size_t)r * d + c];
      t.mats.insert(t.mats.end(), slot.begin(), slot.end());
    } else if (g.code == 10) {
      t.channel.back() = (int32_t)t.n_kraus.size();
      std::vector<cd> slot(16, cd(0, 0));
      for (size_t j = 0; j < g.ms.size(); ++j) std::copy(g.ms[j].begin(), g.ms[j].end(), slot.begin() + 4 * (long)j);
      t.kraus.insert(t.kraus.end(), slot.begin(), slot.end());
      t.n_kraus.push_back((int32_t)g.ms.size());
    } else if (g.code == 11) {
      t.channel.back() = (int32_t)t.n_kraus2.size();
      std::vector<cd> slot(256, cd(0, 0));
      for (size_t j = 0; j < g.ms.size(); ++j) std::copy(g.ms[j].begin(), g.ms[j].end(), slot.begin() + 16 * (long)j);
      t.kraus2.insert(t.kraus2.end(), slot.begin(), slot.end());
      t.n_kraus2.push_back((int32_t)g.ms.size());
    }
  }
  return t;
}

struct Result {
  int rc = 0;
  std::vector<cd> psi;
  std::vector<int32_t> dims;
  std::vector<int8_t> branches = std::vector<int8_t>(8, (int8_t)-9);  // the programs here hold at most four channel gates
  double fidelity = 0, logw = 0, margin = 0;
};

Result run(const Tables& t, uint64_t seed, uint32_t state, uint32_t traj, bool rows = true, bool mask = true) {
  Result r;
  r.dims.assign((size_t)t.n + 1, 0);
  double* block = nullptr;
  int64_t count = 0;
  r.rc = qkb_simulate_conditions(t.n, (int)t.op.size(), t.op.data(), t.q0.data(), t.alpha.data(), 0.0, 1e-16, 0, (int)(t.mats.size() / 16),
                                 reinterpret_cast<const double*>(t.mats.data()), t.mat.data(), (int)t.n_kraus.size(), reinterpret_cast<const double*>(t.kraus.data()), t.n_kraus.data(),
                                 t.channel.data(), t.branch.data(), seed, state, traj, 0, (int)t.n_kraus2.size(), reinterpret_cast<const double*>(t.kraus2.data()), t.n_kraus2.data(),
                                 rows ? t.cond_gate.data() : nullptr, mask ? t.cond_mask.data() : nullptr, r.dims.data(), &block, &count, &r.fidelity, &r.logw, r.branches.data(),
                                 &r.margin);
  if (r.rc != 0) return r;
  const cd* a = reinterpret_cast<const cd*>(block);  // contract the chain into the dense vector
  std::vector<cd> v(1, cd(1, 0));
  size_t rowsv = 1;
  for (int k = 0; k < t.n; ++k) {
    const int l = r.dims[(size_t)k], rr = r.dims[(size_t)k + 1];
    std::vector<cd> w(rowsv * 2 * (size_t)rr, cd(0, 0));
    for (size_t i = 0; i < rowsv; ++i)
      for (int x = 0; x < l; ++x)
        for (int p = 0; p < 2; ++p)
          for (int c = 0; c < rr; ++c) w[(i * 2 + (size_t)p) * (size_t)rr + (size_t)c] += v[i * (size_t)l + (size_t)x] * a[((size_t)x * 2 + (size_t)p) * (size_t)rr + (size_t)c];
    a += (size_t)l * 2 * (size_t)rr;
    v.swap(w);
    rowsv *= 2;
  }
  qkb_free(block);
  r.psi = v;
  return r;
}

int fail(const char* what) {
  std::printf("FAILED: %s (%s)\n", what, qkb_last_error());
  return 1;
}

// (<X>, <Y>, <Z>) of the last qubit of a normalised vector
void bloch_last(const std::vector<cd>& psi, double* out) {
  cd r01 = 0;
  double z = 0;
  for (size_t i = 0; i < psi.size(); i += 2) {
    r01 += psi[i] * std::conj(psi[i + 1]);
    z += std::norm(psi[i]) - std::norm(psi[i + 1]);
  }
  out[0] = 2 * r01.real(), out[1] = -2 * r01.imag(), out[2] = z;
}

const M P0 = {1, 0, 0, 0}, P1 = {0, 0, 0, 1};

// ---- the enumeration: every classical record of the program by a dense branch loop, and the builder forced to the same record
struct Enum {
  const std::vector<Gate>& prog;
  const Tables& t;
  int n;
  std::vector<cd> want, got;
  double total = 0;
  int records = 0, skipped = 0, failed = 0;
  std::vector<int> taken;  // per gate: the branch (-2: skipped), read by conditions

  void leaf(const std::vector<cd>& phi) {
    const int dim = 1 << n;
    double nrm = 0;
    for (const cd& x : phi) nrm += std::norm(x);
    for (int i = 0; i < dim; ++i)
      for (int k = 0; k < dim; ++k) want[(size_t)i * dim + k] += phi[(size_t)i] * std::conj(phi[(size_t)k]);
    if (nrm < 1e-20) return;  // an impossible record: the builder refuses to force it
    Tables f = t;
    std::vector<int8_t> rec;
    for (size_t i = 0; i < prog.size(); ++i)
      if (prog[i].code == 10 || prog[i].code == 11) {
        rec.push_back((int8_t)taken[i]);
        if (taken[i] >= 0) f.branch[i] = taken[i];  // a skipped gate keeps its own entry
        skipped += taken[i] == -2;
      }
    const Result r = run(f, 1, 2, 3);
    if (r.rc != 0 || !std::equal(rec.begin(), rec.end(), r.branches.begin())) {
      ++failed;
      return;
    }
    ++records;
    const double w = std::exp(r.logw);
    total += w;
    for (int i = 0; i < dim; ++i)
      for (int k = 0; k < dim; ++k) got[(size_t)i * dim + k] += w * r.psi[(size_t)i] * std::conj(r.psi[(size_t)k]);
  }

  void walk(size_t i, std::vector<cd> phi) {
    if (i == prog.size()) return leaf(phi);
    const Gate& g = prog[i];
    const bool is_channel = g.code == 10 || g.code == 11;
    if (g.cond >= 0 && !(taken[(size_t)g.cond] >= 0 && ((g.mask >> taken[(size_t)g.cond]) & 1u))) {
      if (is_channel) taken[i] = -2;
      return walk(i + 1, phi);
    }
    if (!is_channel) {
      const M m = dense_matrix(g);
      if (two_qubit(g.code)) dense2(phi, n, m.data(), g.q);
      else dense1(phi, n, m.data(), g.q);
      return walk(i + 1, phi);
    }
    for (size_t b = 0; b < g.ms.size(); ++b) {
      std::vector<cd> next = phi;
      if (g.code == 11) dense2(next, n, g.ms[b].data(), g.q);
      else dense1(next, n, g.ms[b].data(), g.q);
      taken[i] = (int)b;
      walk(i + 1, next);
    }
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || qkb_init(argv[1]) != 0) return fail("qkb_init");
  // ---- teleportation: Ry(a) Rz(b) on qubit 0, a Bell pair on (1, 2), CX(0, 1), H(0), two measurements, X if m1, Z if m0
  const double a = 0.37, b = 0.81;
  std::vector<Gate> tele = {{5, 0, a, {}}, {1, 0, b, {}}, {0, 1, 0, {}}, {9, 1, 0, {CX}}, {9, 0, 0, {CX}}, {0, 0, 0, {}}, {10, 0, 0, {P0, P1}}, {10, 1, 0, {P0, P1}},
                            {8, 2, 0, {X}, 7, 2u}, {8, 2, 0, {Z}, 6, 2u}};
  const Tables tt = tables(3, tele);
  const double th = 0.5 * M_PI * a, ph = 0.5 * M_PI * b, c = std::cos(th), s = std::sin(th);
  const double want_bloch[3] = {2 * c * s * std::cos(2 * ph), 2 * c * s * std::sin(2 * ph), c * c - s * s};
  double worst_tele = 0;
  int bare_differs = 0;
  for (int m0 = 0; m0 < 2; ++m0)
    for (int m1 = 0; m1 < 2; ++m1) {
      Tables f = tt;
      f.branch[6] = m0, f.branch[7] = m1;
      const Result r = run(f, 0, 0, 0);
      if (r.rc != 0 || r.branches[0] != m0 || r.branches[1] != m1) return fail("forced teleportation");
      double got[3];
      bloch_last(r.psi, got);
      for (int k = 0; k < 3; ++k) worst_tele = std::max(worst_tele, std::fabs(got[k] - want_bloch[k]));
      worst_tele = std::max(worst_tele, std::fabs(r.logw - std::log(0.25)));
      std::fill(f.cond_mask.begin(), f.cond_mask.end(), 0u);  // never: the program without its two corrections
      const Result bare = run(f, 0, 0, 0);
      if (bare.rc != 0) return fail("teleportation without corrections");
      bloch_last(bare.psi, got);
      double off = 0;
      for (int k = 0; k < 3; ++k) off = std::max(off, std::fabs(got[k] - want_bloch[k]));
      bare_differs += off > 0.05;
    }
  int patterns = 0;
  for (uint32_t traj = 0; traj < 12; ++traj) {
    const Result r = run(tt, 2025, 1, traj);
    if (r.rc != 0) return fail("drawn teleportation");
    double got[3];
    bloch_last(r.psi, got);
    for (int k = 0; k < 3; ++k) worst_tele = std::max(worst_tele, std::fabs(got[k] - want_bloch[k]));
    worst_tele = std::max(worst_tele, std::fabs(r.logw - std::log(0.25)));
    patterns |= 1 << (r.branches[0] * 2 + r.branches[1]);
  }
  std::printf("teleportation: max deviation %.3e, %d of 4 patterns differ without the corrections, drawn pattern set %d\n", worst_tele, bare_differs, patterns);
  if (!(worst_tele < 1e-12) || bare_differs != 3) return fail("teleportation");
  // ---- the enumeration on 4 qubits
  const double p = 0.4, q = 0.5, f3 = 0.3;
  const std::vector<M> damping = {{1, 0, 0, std::sqrt(1 - p)}, {0, std::sqrt(p), 0, 0}};
  std::vector<M> depol1 = {{std::sqrt(1 - 0.75 * q), 0, 0, std::sqrt(1 - 0.75 * q)}, X, Y, Z};  // sqrt(1 - 3q/4) 1, sqrt(q/4) X, Y, Z
  for (int k = 1; k < 4; ++k)
    for (cd& x : depol1[(size_t)k]) x *= std::sqrt(q / 4);
  std::vector<M> measure2(4, M(16, cd(0, 0)));
  for (int k = 0; k < 4; ++k) measure2[(size_t)k][(size_t)k * 5] = 1;
  const std::vector<M> flip = {kron(I2, I2, std::sqrt(1 - f3)), kron(Z, Z, std::sqrt(f3))};
  const std::vector<Gate> prog = {{0, 0, 0, {}},        {9, 0, 0, {CX}},          {5, 2, 0.3, {}},         {2, 1, 0.4, {}},         {10, 1, 0, damping},
                                  {2, 2, 0.35, {}},     {11, 2, 0, measure2},     {8, 0, 0, {X}, 4, 2u},   {6, 1, 0.3, {}, 6, 6u},  {10, 2, 0, depol1, 6, 9u},
                                  {1, 3, 0.7, {}, 9, 14u}, {11, 0, 0, flip, 4, 1u}, {7, 2, 0.25, {}, 11, 2u}, {5, 1, 0.2, {}}};
  const Tables t = tables(4, prog);
  Enum e{prog, t, 4, std::vector<cd>(256, cd(0, 0)), std::vector<cd>(256, cd(0, 0))};
  e.taken.assign(prog.size(), -1);
  std::vector<cd> phi(16, cd(0, 0));
  phi[0] = 1;
  e.walk(0, phi);
  double worst = 0, trace = 0;
  for (size_t k = 0; k < e.want.size(); ++k) worst = std::max(worst, std::abs(e.want[k] - e.got[k]));
  for (int i = 0; i < 16; ++i) trace += e.want[(size_t)i * 17].real();
  std::printf("enumeration: %d records (%d skipped channel gates), max |rho - dense| = %.3e, sum of weights - 1 = %.3e, trace - 1 = %.3e\n", e.records, e.skipped, worst,
              e.total - 1, trace - 1);
  if (e.failed || e.skipped == 0 || !(worst < 1e-10) || !(std::fabs(e.total - 1) < 1e-10) || !(std::fabs(trace - 1) < 1e-12)) return fail("enumeration");
  // ---- without rows the call is qkb_simulate_channels2; rows that condition nothing change nothing
  {
    Tables none = t;
    std::fill(none.cond_gate.begin(), none.cond_gate.end(), -1);
    const Result x = run(none, 7, 1, 0), y = run(t, 7, 1, 0, false);
    if (x.rc != 0 || y.rc != 0 || x.logw != y.logw || std::memcmp(x.psi.data(), y.psi.data(), x.psi.size() * sizeof(cd)) != 0) return fail("no conditions");
  }
  // ---- the rejections: -8, the gate named
  int rejected = 0;
  auto bad = [&](auto edit, const char* text, bool rows = true, bool mask = true) {
    Tables f = tables(4, prog);
    edit(f);
    const Result r = run(f, 0, 0, 0, rows, mask);
    const bool ok = r.rc == -8 && std::strstr(qkb_last_error(), text) != nullptr;
    if (!ok) std::printf("expected -8 with '%s', got %d (%s)\n", text, r.rc, r.rc ? qkb_last_error() : "");
    return ok ? 1 : 0;
  };
  rejected += bad([](Tables& f) { f.cond_gate[3] = -2; }, "gate 3: condition on gate -2");
  rejected += bad([](Tables& f) { f.cond_gate[7] = 7; }, "gate 7: condition on gate 7");
  rejected += bad([](Tables& f) { f.cond_gate[5] = 6; }, "gate 5: condition on gate 6");
  rejected += bad([](Tables& f) { f.cond_gate[8] = 5; }, "gate 8: condition on gate 5, which is no channel gate");
  rejected += bad([](Tables& f) { f.cond_mask[7] = 4u; }, "gate 7: condition mask");
  rejected += bad([](Tables& f) { f.cond_mask[8] = 16u; }, "gate 8: condition mask");
  rejected += bad([](Tables&) {}, "cond_mask", true, false);
  {  // rows in a call without a channel table
    Tables f = tables(4, {{0, 0, 0, {}}, {2, 0, 0.3, {}}, {1, 1, 0.2, {}, 1, 1u}});
    const Result r = run(f, 0, 0, 0);
    rejected += r.rc == -8 && std::strstr(qkb_last_error(), "gate 0") != nullptr && std::strstr(qkb_last_error(), "channel table") != nullptr;
  }
  std::printf("%d rejections ok\n", rejected);
  return rejected == 8 ? 0 : 1;
}
