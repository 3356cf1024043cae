// The units of an edge product in the site-fused sweep (qk_edge_units / qk_edge_unit, csrc/qk_plan.h), on the CPU.  For every mt, nt in 1..16
// and NW in {8, 12}, walking the indices the way the waves do (u = wave, wave + NW, ... below qk_edge_units):
//   * cover: every tile (ta, tb) of the mt x nt product is taken exactly once, and no unit leaves the product;
//   * pairing: a unit with has1 takes (ta, tb0) and (ta, tb0 + 1) -- the same block of the x operand, neighbouring blocks of the y operand --
//     with tb0 even, and a wave never takes two units in one round;
//   * halves: with `left` pairs in the last round, 2 left <= NW  <=>  that round is dealt as single tiles (no unit of it has has1), its
//     first tiles on the indices r0 .. r0 + left - 1 and its second tiles `left` further up; in every other round each pair that has a
//     second tile takes it (has1), so only the last column block of an odd nt is single there;
//   * the reciprocal: qk_recip20(mt) divides every pair index the decode can meet.
// Built with g++ and run by tests/test_edge_units.py; prints one line per check, exits 1 on a failure.
#include "../../qml-cutensornet_amd/csrc/qk_plan.h"

#include <vector>

namespace {

int report(const char* what, const long checked, const long bad) {
  std::printf("%s  %s: %ld checked, %ld bad\n", bad ? "FAIL" : "ok  ", what, checked, bad);
  return bad ? 1 : 0;
}

}  // namespace

int main() {
  long n = 0, bad_cover = 0, bad_pair = 0, bad_half = 0, bad_recip = 0, n_halves = 0;
  for (const int NW : {8, 12})
    for (int mt = 1; mt <= 16; ++mt)
      for (int nt = 1; nt <= 16; ++nt) {
        ++n;
        const int inv = qk_recip20(mt), units = qk_edge_units(mt, nt, NW);
        const int pairs = mt * ((nt + 1) / 2), r0 = (pairs - 1) / NW * NW, left = pairs - r0;
        const bool halves = 2 * left <= NW;
        n_halves += halves;
        std::vector<int> seen(mt * nt, 0);
        bool cover = true, pairing = true, half = true, recip = true;
        // the count of indices: whole rounds of pairs, then the last round as pairs or as 2 left single tiles -- never more than a round of them
        half = half && units == (halves ? r0 + 2 * left : pairs) && units - r0 <= NW && units - r0 > 0;
        for (int v = 0; v < pairs + NW; ++v) recip = recip && ((v * inv) >> 20) == v / mt;
        for (int wave = 0; wave < NW; ++wave) {
          int last_round = -1;
          for (int u = wave; u < units; u += NW) {
            const QkEdgeUnit un = qk_edge_unit(u, mt, nt, NW, inv);
            pairing = pairing && u / NW != last_round;
            last_round = u / NW;
            const bool tail = u >= r0;
            if (!un.mine) {  // an index without a tile: only the missing second tile of an odd last column block, in a round of singles
              half = half && halves && tail && u >= r0 + left && un.tb0 == nt;
              continue;
            }
            cover = cover && un.ta >= 0 && un.ta < mt && un.tb0 >= 0 && un.tb0 + (un.has1 ? 1 : 0) < nt;
            if (!cover) break;
            ++seen[un.tb0 * mt + un.ta];
            if (un.has1) {
              ++seen[(un.tb0 + 1) * mt + un.ta];  // the same ta, the next column block
              pairing = pairing && un.tb0 % 2 == 0;
            }
            if (halves && tail) {  // a round of singles: first tiles, then second tiles, of the pairs r0 + w
              const int w = (u - r0) % left, v = r0 + w;
              half = half && !un.has1 && un.ta == v % mt && un.tb0 == 2 * (v / mt) + (u - r0) / left;
            } else {  // a pair takes its second tile whenever it has one
              half = half && un.ta == u % mt && un.tb0 == 2 * (u / mt) && un.has1 == (un.tb0 + 1 < nt);
            }
          }
        }
        for (int e = 0; cover && e < mt * nt; ++e) cover = seen[e] == 1;
        bad_cover += !cover, bad_pair += !pairing, bad_half += !half, bad_recip += !recip;
        if (!(cover && pairing && half && recip)) std::printf("      NW %d mt %d nt %d: cover %d pairing %d halves %d recip %d\n", NW, mt, nt, (int)cover, (int)pairing, (int)half, (int)recip);
      }
  int failed = 0;
  failed += report("every tile exactly once", n, bad_cover);
  failed += report("pairs: one row block, neighbouring column blocks, one unit per wave and round", n, bad_pair);
  failed += report("halves rule", n, bad_half);
  failed += report("reciprocal == division", n, bad_recip);
  std::printf("      (%ld of the shapes end in a round of single tiles)\n", n_halves);
  return failed ? 1 : 0;
}
