// Host-only sanitizer driver for building from a given state in the native host MPS builder (qk_builder.cpp: qkb_simulate_program, spelt qkb_simulate_initial in tests/host_san/qkb_calls.h),
// built with -fsanitize=address,undefined and run by tests/test_initial_san.py in the CPU tier.  A 5-qubit program with a Unitary-like
// 4x4, a Measure with a conditional X and a two-qubit dephasing channel is (a) run from a product state written out here against a
// dense loop of this file, forced through every classical record, and (b) split behind a two-qubit gate: the second half, started from
// the tensors the first half returned, must give the vector, the record and the log-weight of the uninterrupted run.  A null bond
// table is qkb_simulate_conditions bit for bit, the initial fidelity and log-weight travel, and every rejection comes back as -8.
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
constexpr int N = 5;

void dense1(std::vector<cd>& psi, const cd* m, int q) {
  const int b = 1 << (N - 1 - q);
  for (int i = 0; i < (1 << N); ++i)
    if (!(i & b)) {
      const cd x = psi[(size_t)i], y = psi[(size_t)(i | b)];
      psi[(size_t)i] = m[0] * x + m[1] * y;
      psi[(size_t)(i | b)] = m[2] * x + m[3] * y;
    }
}
void dense2(std::vector<cd>& psi, const cd* m, int qa) {  // on (qa, qa + 1), qa most significant
  const int ba = 1 << (N - 1 - qa), bb = ba >> 1;
  for (int i = 0; i < (1 << N); ++i)
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

// The program: 0 Ry(0) 1 Ry(3) 2 XX(1,2) 3 M9(2,3) | 4 Rz(2) 5 Measure(2) 6 X(4) if gate 5 gave 1 7 ZZdephase(0,1) 8 XX(3,4) 9 Ry(1)
// (the bar: the cut of the split run, behind the 4x4 on (2, 3): the first half, run alone, ends with it and leaves its centre on site 3)
constexpr int CUT = 4, CUT_CENTRE = 3, N_OPS = 10;
const int8_t OP[N_OPS] = {5, 5, 2, 9, 1, 10, 8, 11, 2, 5};
const int32_t Q0[N_OPS] = {0, 3, 1, 2, 2, 2, 4, 0, 3, 1};
const double ALPHA[N_OPS] = {0.3, 0.7, 0.4, 0, 0.6, 0, 0, 0, 0.35, 0.2};
const int32_t MAT[N_OPS] = {-1, -1, -1, 0, -1, -1, 1, -1, -1, -1};
const int32_t CHANNEL[N_OPS] = {-1, -1, -1, -1, -1, 0, -1, 0, -1, -1};
const int32_t COND_GATE[N_OPS] = {-1, -1, -1, -1, -1, -1, 5, -1, -1, -1};
const uint32_t COND_MASK[N_OPS] = {0, 0, 0, 0, 0, 0, 2u, 0, 0, 0};

struct Tables {
  std::vector<cd> mats = std::vector<cd>(32, cd(0, 0)), kraus = std::vector<cd>(16, cd(0, 0)), kraus2 = std::vector<cd>(256, cd(0, 0));
  int32_t n_kraus = 2, n_kraus2 = 2;
  cd u4[16];
  Tables() {
    // a 4x4 unitary: (CX . (Ry(0.5) (x) Rz(0.3))) with a phase
    const double c = std::cos(0.25 * M_PI), s = std::sin(0.25 * M_PI);
    const cd ry[4] = {c, -s, s, c}, rz[4] = {std::polar(1.0, -0.15 * M_PI), 0, 0, std::polar(1.0, 0.15 * M_PI)};
    cd k[16];
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j)
        for (int a = 0; a < 2; ++a)
          for (int b = 0; b < 2; ++b) k[(i * 2 + a) * 4 + (j * 2 + b)] = ry[i * 2 + j] * rz[a * 2 + b];
    const int perm[4] = {0, 1, 3, 2};  // CX rows
    for (int r = 0; r < 4; ++r)
      for (int col = 0; col < 4; ++col) u4[r * 4 + col] = std::polar(1.0, 0.4) * k[perm[r] * 4 + col];
    std::copy(u4, u4 + 16, mats.begin());
    mats[16 + 1] = 1, mats[16 + 4] = 1;  // X in [:2][:2] of slot 1
    kraus[0] = 1, kraus[4 + 3] = 1;      // the projectors of Measure
    const double f = 0.3;
    for (int i = 0; i < 4; ++i) {
      kraus2[(size_t)i * 5] = std::sqrt(1 - f);
      kraus2[16 + (size_t)i * 5] = std::sqrt(f) * ((i == 0 || i == 3) ? 1.0 : -1.0);  // sqrt(f) Z (x) Z
    }
  }
};

struct Result {
  int rc = 0;
  std::vector<int32_t> dims = std::vector<int32_t>(N + 1, 0);
  std::vector<cd> tensors, psi;
  int8_t branches[4] = {-9, -9, -9, -9};
  double fidelity = 0, logw = 0, margin = 0;
};

struct Init {
  const int32_t* dims = nullptr;
  const cd* tensors = nullptr;
  int centre = 0;
  double fidelity = 1, logw = 0;
};

// gates [a, b) of the program from `init` (null bond table: |0...0>), branch rows `branch` of the whole program
Result run(const Tables& t, int a, int b, const int32_t* branch, const Init& in, uint32_t traj, bool through_conditions = false) {
  Result r;
  std::vector<int32_t> cg(COND_GATE + a, COND_GATE + b);
  for (int32_t& g : cg) g = g >= 0 ? g - a : g;
  double* block = nullptr;
  int64_t count = 0;
  const double* mats = reinterpret_cast<const double*>(t.mats.data());
  const double* k1 = reinterpret_cast<const double*>(t.kraus.data());
  const double* k2 = reinterpret_cast<const double*>(t.kraus2.data());
  if (through_conditions)
    r.rc = qkb_simulate_conditions(N, b - a, OP + a, Q0 + a, ALPHA + a, 0.0, 1e-16, 0, 2, mats, MAT + a, 1, k1, &t.n_kraus, CHANNEL + a, branch + a, 11, 0, traj, (uint32_t)a, 1, k2,
                                   &t.n_kraus2, cg.data(), COND_MASK + a, r.dims.data(), &block, &count, &r.fidelity, &r.logw, r.branches, &r.margin);
  else
    r.rc = qkb_simulate_initial(N, b - a, OP + a, Q0 + a, ALPHA + a, 0.0, 1e-16, 0, 2, mats, MAT + a, 1, k1, &t.n_kraus, CHANNEL + a, branch + a, 11, 0, traj, (uint32_t)a, 1, k2,
                                &t.n_kraus2, cg.data(), COND_MASK + a, in.dims, reinterpret_cast<const double*>(in.tensors), in.centre, in.fidelity, in.logw, r.dims.data(), &block,
                                &count, &r.fidelity, &r.logw, r.branches, &r.margin);
  if (r.rc != 0) return r;
  const cd* p = reinterpret_cast<const cd*>(block);
  r.tensors.assign(p, p + count);
  std::vector<cd> v(1, cd(1, 0));
  size_t rows = 1;
  for (int k = 0; k < N; ++k) {
    const int l = r.dims[(size_t)k], rr = r.dims[(size_t)k + 1];
    std::vector<cd> w(rows * 2 * (size_t)rr, cd(0, 0));
    for (size_t i = 0; i < rows; ++i)
      for (int x = 0; x < l; ++x)
        for (int ph = 0; ph < 2; ++ph)
          for (int c = 0; c < rr; ++c) w[(i * 2 + (size_t)ph) * (size_t)rr + (size_t)c] += v[i * (size_t)l + (size_t)x] * p[((size_t)x * 2 + (size_t)ph) * (size_t)rr + (size_t)c];
    p += (size_t)l * 2 * (size_t)rr;
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

// the dense loop over gates [a, b) with the record (m, z): the Measure's outcome and the dephasing channel's branch
void dense_gates(const Tables& t, std::vector<cd>& psi, int a, int b, int m, int z) {
  const double h = 0.5 * M_PI;
  for (int i = a; i < b; ++i) {
    const double th = h * ALPHA[i], c = std::cos(th), s = std::sin(th);
    if (OP[i] == 5) {
      const cd g[4] = {c, -s, s, c};
      dense1(psi, g, Q0[i]);
    } else if (OP[i] == 1) {
      const cd g[4] = {std::polar(1.0, -th), 0, 0, std::polar(1.0, th)};
      dense1(psi, g, Q0[i]);
    } else if (OP[i] == 2) {
      cd g[16] = {};
      for (int k = 0; k < 4; ++k) g[k * 5] = c, g[k * 4 + (3 - k)] = cd(0, -s);
      dense2(psi, g, Q0[i]);
    } else if (OP[i] == 9) {
      dense2(psi, t.u4, Q0[i]);
    } else if (OP[i] == 10) {
      dense1(psi, t.kraus.data() + 4 * m, Q0[i]);
    } else if (OP[i] == 8) {
      const cd x[4] = {0, 1, 1, 0};
      if (m == 1) dense1(psi, x, Q0[i]);
    } else {
      dense2(psi, t.kraus2.data() + 16 * z, Q0[i]);
    }
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || qkb_init(argv[1]) != 0) return fail("qkb_init");
  const Tables t;
  int32_t drawn[N_OPS];
  std::fill(drawn, drawn + N_OPS, -1);
  // ---- (a) a product state, every record forced: |psi0> = (x)_k (cos a_k |0> + e^{i b_k} sin a_k |1>), bonds 1, centre 0
  {
    const int32_t dims[N + 1] = {1, 1, 1, 1, 1, 1};
    std::vector<cd> sites, psi0(1, cd(1, 0));
    for (int k = 0; k < N; ++k) {
      const cd v[2] = {std::cos(0.3 + 0.2 * k), std::polar(std::sin(0.3 + 0.2 * k), 0.5 * k)};
      sites.push_back(v[0]), sites.push_back(v[1]);
      std::vector<cd> w;
      for (const cd& x : psi0) w.push_back(x * v[0]), w.push_back(x * v[1]);
      psi0.swap(w);
    }
    double worst = 0, total = 0;
    for (int m = 0; m < 2; ++m)
      for (int z = 0; z < 2; ++z) {
        int32_t forced[N_OPS];
        std::copy(drawn, drawn + N_OPS, forced);
        forced[5] = m, forced[7] = z;
        const Result r = run(t, 0, N_OPS, forced, Init{dims, sites.data(), 0, 1.0, 0.0}, 0);
        if (r.rc != 0 || r.branches[0] != m || r.branches[1] != z) return fail("forced run from a product state");
        std::vector<cd> phi = psi0;
        dense_gates(t, phi, 0, N_OPS, m, z);
        double p = 0;
        for (const cd& x : phi) p += std::norm(x);
        total += p;
        worst = std::max(worst, std::fabs(r.logw - std::log(p)));
        for (size_t i = 0; i < phi.size(); ++i) worst = std::max(worst, std::abs(r.psi[i] - phi[i] / std::sqrt(p)));
      }
    std::printf("product state: max deviation from the dense loop %.3e, sum of record weights - 1 = %.3e\n", worst, total - 1);
    if (!(worst < 1e-12) || !(std::fabs(total - 1) < 1e-12)) return fail("product state");
  }
  // ---- (b) the split run, drawn: gates [CUT, N_OPS) from what gates [0, CUT) returned (the centre on site 3)
  {
    double worst = 0;
    int patterns = 0;
    for (uint32_t traj = 0; traj < 8; ++traj) {
      const Result whole = run(t, 0, N_OPS, drawn, Init{}, traj);
      const Result first = run(t, 0, CUT, drawn, Init{}, traj);
      if (whole.rc != 0 || first.rc != 0) return fail("uninterrupted run");
      const Result second = run(t, CUT, N_OPS, drawn, Init{first.dims.data(), first.tensors.data(), CUT_CENTRE, first.fidelity, first.logw}, traj);
      if (second.rc != 0 || second.branches[0] != whole.branches[0] || second.branches[1] != whole.branches[1]) return fail("resumed run");
      worst = std::max(worst, std::fabs(second.logw - whole.logw));
      for (size_t i = 0; i < whole.psi.size(); ++i) worst = std::max(worst, std::abs(second.psi[i] - whole.psi[i]));
      patterns |= 1 << (whole.branches[0] * 2 + whole.branches[1]);
    }
    std::printf("split run: max deviation from the uninterrupted run %.3e, drawn pattern set %d\n", worst, patterns);
    if (!(worst < 1e-12)) return fail("split run");
  }
  // ---- a null bond table is qkb_simulate_conditions; fidelity and log-weight travel
  {
    const Result x = run(t, 0, N_OPS, drawn, Init{}, 3), y = run(t, 0, N_OPS, drawn, Init{}, 3, true);
    if (x.rc != 0 || y.rc != 0 || x.logw != y.logw || x.fidelity != y.fidelity || x.tensors.size() != y.tensors.size() ||
        std::memcmp(x.tensors.data(), y.tensors.data(), x.tensors.size() * sizeof(cd)) != 0)
      return fail("null bond table");
    const Result first = run(t, 0, CUT, drawn, Init{}, 3);
    const Result z = run(t, CUT, CUT + 1, drawn, Init{first.dims.data(), first.tensors.data(), CUT_CENTRE, 0.75, -1.5}, 3);
    if (z.rc != 0 || z.fidelity != 0.75 || z.logw != -1.5) return fail("fidelity and log-weight of the initial state");
    std::printf("null bond table and carried weights ok\n");
  }
  // ---- the rejections: -8 before a gate is applied
  int rejected = 0;
  {
    const Result first = run(t, 0, CUT, drawn, Init{}, 0);
    auto bad = [&](std::vector<int32_t> dims, std::vector<cd> tensors, int centre, double fid, const char* text) {
      const Result r = run(t, CUT, N_OPS, drawn, Init{dims.data(), tensors.data(), centre, fid, 0.0}, 0);
      const bool ok = r.rc == -8 && std::strstr(qkb_last_error(), text) != nullptr;
      if (!ok) std::printf("expected -8 with '%s', got %d (%s)\n", text, r.rc, r.rc ? qkb_last_error() : "");
      return ok ? 1 : 0;
    };
    std::vector<int32_t> d = first.dims;
    d[0] = 2;
    rejected += bad(d, first.tensors, CUT_CENTRE, 1.0, "boundary bonds must be 1");
    d = first.dims, d[N] = 3;
    rejected += bad(d, first.tensors, CUT_CENTRE, 1.0, "boundary bonds must be 1");
    d = first.dims, d[2] = 0;
    rejected += bad(d, first.tensors, CUT_CENTRE, 1.0, "bonds must be positive");
    d = first.dims, d[3] = -2;
    rejected += bad(d, first.tensors, CUT_CENTRE, 1.0, "bonds must be positive");
    rejected += bad(first.dims, first.tensors, -1, 1.0, "outside the register");
    rejected += bad(first.dims, first.tensors, N, 1.0, "outside the register");
    std::vector<cd> nan = first.tensors;
    nan.back() = cd(0, std::numeric_limits<double>::quiet_NaN());
    rejected += bad(first.dims, nan, CUT_CENTRE, 1.0, "not finite");
    rejected += bad(first.dims, first.tensors, CUT_CENTRE, std::numeric_limits<double>::infinity(), "not finite");
  }
  std::printf("%d rejections ok\n", rejected);
  return rejected == 8 ? 0 : 1;
}
