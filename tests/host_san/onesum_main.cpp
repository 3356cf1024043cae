// One column block of phase 2 of the site-fused sweep in its one-sum form (csrc/qk_fused.h: qkf_p2_onesum), restated in plain C++.  Built
// with g++ -fsanitize=address,undefined and run by tests/test_onesum_host.py; prints one line per check, exits 1 on a failure.
//
// The block multiplies a T tile (K x 16, K = 4 kmax rows of the bond a, 16 columns of b') with a fragment of A (K x 16 columns of a'):
//     ordinary   X'[m][n] += sum_k T[k][m] conj(A[k][n])      S = Ar + Ai;  k1 = sum ti S;  re = k1 + sum (tr - ti) Ar;  im = k1 + sum (-tr - ti) Ai
//     switch     Y[n][m]  += sum_k conj(T[k][m]) A[k][n]      S = Ar + Ai;  k1 = sum S tr;  re = k1 + sum Ai (ti - tr);  im = k1 + sum Ar (-tr - ti)
// with the matrix instruction D = C + P^T Q on one k-step (4 rows) of its operands, the source operands exchanged in the switch block, the
// chain of k1 started on zero and the chains of re and im started on k1.  The T-side sets (k, a, b) come from the three real products of
// phase 1 (p1 = sum xr br, p2 = sum xi bi, p3 = sum (xr + xi)(br + bi)) directly, and -- the form the kernels use -- from the tile
// (re, im) = (p1 - p2, p3 - p1 - p2) at the head of phase 2.
//   ordinary / switch   kmax = 1 .. 4, the full form (all four k-steps unconditionally) and the ragged one (k-step 0 and those below kmax),
//                       a single tile and a pair of tiles that share the fragment, both derivations of the sets: against the straightforward
//                       complex product to 1e-13 of sum |T| |A|
//   adjoint             the switch result is the conjugate transpose of the ordinary one (same bound)
#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

namespace {

typedef std::complex<double> cd;
constexpr int TILE = 16;

struct Frag {  // one k-step of an operand: 4 rows of 16
  double v[4][TILE];
};
struct Acc {
  double v[TILE][TILE];
};

// v_mfma_f64_16x16x4_f64: D[i][j] = C[i][j] + sum_{k < 4} P[k][i] Q[k][j]
Acc mma(const Frag& p, const Frag& q, const Acc& c) {
  Acc d;
  for (int i = 0; i < TILE; ++i)
    for (int j = 0; j < TILE; ++j) {
      double s = c.v[i][j];
      for (int k = 0; k < 4; ++k) s += p.v[k][i] * q.v[k][j];
      d.v[i][j] = s;
    }
  return d;
}

struct TSet {  // the three register sets of a tile, per k-step
  Frag k[4], a[4], b[4];
};
struct Tile3 {  // what phase 1 leaves: the three real products, per k-step of phase 2 (the C layout of phase 1 is the operand layout of phase 2)
  Frag p1[4], p2[4], p3[4];
};

template <typename F>
Frag map3(const Frag& x, const Frag& y, const Frag& z, F f) {
  Frag r;
  for (int k = 0; k < 4; ++k)
    for (int j = 0; j < TILE; ++j) r.v[k][j] = f(x.v[k][j], y.v[k][j], z.v[k][j]);
  return r;
}

// the sets straight from p1, p2, p3 ...
TSet sets_from_products(const Tile3& t, const bool sw) {
  TSet u;
  for (int i = 0; i < 4; ++i) {
    if (!sw) {
      u.k[i] = map3(t.p1[i], t.p2[i], t.p3[i], [](double p1, double p2, double p3) { return p3 - p1 - p2; });  // ti
      u.a[i] = map3(t.p1[i], t.p2[i], t.p3[i], [](double p1, double, double p3) { return 2 * p1 - p3; });       // tr - ti
    } else {
      u.k[i] = map3(t.p1[i], t.p2[i], t.p3[i], [](double p1, double p2, double) { return p1 - p2; });           // tr
      u.a[i] = map3(t.p1[i], t.p2[i], t.p3[i], [](double p1, double, double p3) { return p3 - 2 * p1; });       // ti - tr
    }
    u.b[i] = map3(t.p1[i], t.p2[i], t.p3[i], [](double, double p2, double p3) { return 2 * p2 - p3; });         // -tr - ti
  }
  return u;
}
// ... and from the tile (re, im) at the head of phase 2
TSet sets_from_tile(const Tile3& t, const bool sw) {
  TSet u;
  for (int i = 0; i < 4; ++i) {
    const Frag re = map3(t.p1[i], t.p2[i], t.p3[i], [](double p1, double p2, double) { return p1 - p2; });
    const Frag im = map3(t.p1[i], t.p2[i], t.p3[i], [](double p1, double p2, double p3) { return p3 - p1 - p2; });
    u.k[i] = sw ? re : im;
    u.a[i] = map3(re, im, im, [sw](double r, double m, double) { return sw ? m - r : r - m; });
    u.b[i] = map3(re, im, im, [](double r, double m, double) { return -r - m; });
  }
  return u;
}

struct AFrag {  // one k-step of the fragment of A
  Frag x, y;
};

// the block, as qkf_p2_onesum issues it (one tile: the second tile of a pair runs the same chains on its own sets)
void block(const TSet& u, const AFrag (&fr)[4], const int kmax, const bool full, const bool sw, Acc* re_out, Acc* im_out) {
  Acc zero{};
  Acc k1 = zero, re = zero, im = zero;
  for (int i = 0; i < 4; ++i) {
    if (!(full || i == 0 || i < kmax)) continue;
    Frag s;
    for (int k = 0; k < 4; ++k)
      for (int j = 0; j < TILE; ++j) s.v[k][j] = fr[i].x.v[k][j] + fr[i].y.v[k][j];
    k1 = sw ? mma(s, u.k[i], i == 0 ? zero : k1) : mma(u.k[i], s, i == 0 ? zero : k1);
  }
  for (int i = 0; i < 4; ++i) {
    if (!(full || i == 0 || i < kmax)) continue;
    if (sw) {
      re = mma(fr[i].y, u.a[i], i == 0 ? k1 : re);
      im = mma(fr[i].x, u.b[i], i == 0 ? k1 : im);
    } else {
      re = mma(u.a[i], fr[i].x, i == 0 ? k1 : re);
      im = mma(u.b[i], fr[i].y, i == 0 ? k1 : im);
    }
  }
  *re_out = re, *im_out = im;
}

}  // namespace

int main() {
  std::mt19937 gen(20261020);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  long long n_blk[2] = {0, 0}, bad_blk[2] = {0, 0}, n_adj = 0, bad_adj = 0;
  double worst[2] = {0, 0}, worst_adj = 0;
  for (int rep = 0; rep < 24; ++rep)
    for (int kmax = 1; kmax <= 4; ++kmax)
      for (int full = 0; full < 2; ++full) {
        if (full && kmax < 4) continue;  // the full form runs where all four k-steps lie below the bond
        for (int tiles = 1; tiles <= 2; ++tiles) {
          // phase 1 of each tile: T = X^T B over 8 values of b, three real products; rows at or above the bond (k-steps >= kmax) are zero
          // in T (X has zero columns there) -- the full form multiplies them, the ragged form skips them
          std::vector<Tile3> t(tiles);
          std::vector<std::vector<cd>> T(tiles, std::vector<cd>(4 * 4 * TILE));  // [k-step][row][m]
          for (int w = 0; w < tiles; ++w)
            for (int i = 0; i < 4; ++i)
              for (int k = 0; k < 4; ++k)
                for (int m = 0; m < TILE; ++m) {
                  double p1 = 0, p2 = 0, p3 = 0;
                  if (i < kmax)
                    for (int l = 0; l < 8; ++l) {
                      const double xr = u(gen), xi = u(gen), br = u(gen), bi = u(gen);
                      p1 += xr * br, p2 += xi * bi, p3 += (xr + xi) * (br + bi);
                    }
                  t[w].p1[i].v[k][m] = p1, t[w].p2[i].v[k][m] = p2, t[w].p3[i].v[k][m] = p3;
                  T[w][(i * 4 + k) * TILE + m] = cd(p1 - p2, p3 - p1 - p2);
                }
          AFrag fr[4];  // (the fragment is loaded whole: k-steps at or above kmax hold whatever the clamped address gave)
          for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k)
              for (int n = 0; n < TILE; ++n) fr[i].x.v[k][n] = u(gen), fr[i].y.v[k][n] = u(gen);
          for (int w = 0; w < tiles; ++w) {
            // the straightforward products and their scale
            std::vector<cd> ord(TILE * TILE), swt(TILE * TILE);
            std::vector<double> scale(TILE * TILE);
            for (int m = 0; m < TILE; ++m)
              for (int n = 0; n < TILE; ++n) {
                cd o = 0, s = 0;
                double sc = 0;
                for (int i = 0; i < kmax; ++i)
                  for (int k = 0; k < 4; ++k) {
                    const cd tt = T[w][(i * 4 + k) * TILE + m], a(fr[i].x.v[k][n], fr[i].y.v[k][n]);
                    o += tt * std::conj(a), s += std::conj(tt) * a, sc += std::abs(tt) * std::abs(a);
                  }
                ord[m * TILE + n] = o, swt[n * TILE + m] = s, scale[m * TILE + n] = sc;
              }
            for (int from_tile = 0; from_tile < 2; ++from_tile) {
              Acc re[2], im[2];
              for (int sw = 0; sw < 2; ++sw) {
                const TSet s = from_tile ? sets_from_tile(t[w], sw != 0) : sets_from_products(t[w], sw != 0);
                block(s, fr, kmax, full != 0, sw != 0, &re[sw], &im[sw]);
                for (int m = 0; m < TILE; ++m)
                  for (int n = 0; n < TILE; ++n) {
                    // ordinary: the accumulators hold X'[m][n]; switch: Y[n][m]
                    const cd got = sw ? cd(re[1].v[n][m], im[1].v[n][m]) : cd(re[0].v[m][n], im[0].v[m][n]);
                    const cd want = sw ? swt[n * TILE + m] : ord[m * TILE + n];
                    const double rel = std::abs(got - want) / scale[m * TILE + n];
                    ++n_blk[sw];
                    if (rel > worst[sw]) worst[sw] = rel;
                    if (!(rel < 1e-13)) {
                      if (++bad_blk[sw] <= 5) std::printf("FAIL %s: kmax %d full %d tile %d of %d sets from %s: [%d][%d] off by %.3e of the scale\n", sw ? "switch" : "ordinary", kmax, full, w, tiles, from_tile ? "the tile" : "p1 p2 p3", m, n, rel);
                    }
                  }
              }
              for (int m = 0; m < TILE; ++m)
                for (int n = 0; n < TILE; ++n) {
                  const cd o(re[0].v[m][n], im[0].v[m][n]), s(re[1].v[n][m], im[1].v[n][m]);
                  const double rel = std::abs(s - std::conj(o)) / scale[m * TILE + n];
                  ++n_adj;
                  if (rel > worst_adj) worst_adj = rel;
                  if (!(rel < 1e-13)) ++bad_adj;
                }
            }
          }
        }
      }
  int bad_total = 0;
  for (int sw = 0; sw < 2; ++sw) {
    std::printf("%s %s: %lld checked, %lld bad (worst %.2e of the scale)\n", bad_blk[sw] ? "FAIL" : "ok  ", sw ? "switch" : "ordinary", n_blk[sw], bad_blk[sw], worst[sw]);
    bad_total += (int)bad_blk[sw];
  }
  std::printf("%s adjoint: %lld checked, %lld bad (worst %.2e of the scale)\n", bad_adj ? "FAIL" : "ok  ", n_adj, bad_adj, worst_adj);
  bad_total += (int)bad_adj;
  return bad_total ? 1 : 0;
}
