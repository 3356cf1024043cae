// The integer side of the shot-based block overlaps (csrc/qk_local_plan.h: sbk_*): the mask and the term at the widths where a shift
// could go wrong (1, 31, 32), the double the kernel adds against the integer term, the packed word at n = 1, 32 and 33 on both sides,
// the cut of the work into tasks (every (pair, setting) exactly once, for any chunk size), the chunk the driver picks against what the
// workgroup can stage, the pieces of a staged row, the groups of widths, and the overflow rule at its boundary.  Every expected value
// is restated here from the definitions, not taken from the header.  Built with g++ -fsanitize=address,undefined and run by
// tests/test_shot_block_plan.py; prints one line per section, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace qkl;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

int popcount(uint32_t v) {
  int c = 0;
  for (; v; v &= v - 1) ++c;
  return c;
}

void test_mask_and_term() {
  CHECK(sbk_mask(1) == 0x1u && sbk_mask(2) == 0x3u && sbk_mask(31) == 0x7fffffffu && sbk_mask(32) == 0xffffffffu);
  // term_w = (-1)^D 2^(w - D), an integer in [-2^(w-1), 2^w]
  CHECK(sbk_term(0, 1) == 2 && sbk_term(1, 1) == -1);
  CHECK(sbk_term(0, 31) == (1ll << 31) && sbk_term(1, 31) == -(1ll << 30) && sbk_term(31, 31) == -1 && sbk_term(30, 31) == 2);
  CHECK(sbk_term(0, 32) == (1ll << 32) && sbk_term(1, 32) == -(1ll << 31) && sbk_term(32, 32) == 1 && sbk_term(31, 32) == -2);
  for (const int w : {1, 2, 5, 31, 32})
    for (int D = 0; D <= w; ++D) {
      long long want = 1;
      for (int k = 0; k < w - D; ++k) want *= 2;
      CHECK(sbk_term(D, w) == ((D % 2) ? -want : want));
      // the double of the kernel: high word from E = 1023 + (agreeing bits), low word 0, times the sign of the width
      const uint64_t bits = (uint64_t)sbk_agree_hi(1023u + (uint32_t)(w - D)) << 32;
      double dv;
      std::memcpy(&dv, &bits, sizeof(dv));
      CHECK((long long)dv * sbk_agree_sign(w) == sbk_term(D, w));
    }
  // two words through the mask: D counts the differing bits below w only
  const uint32_t s = 0xdeadbeefu, t = 0x12345678u;
  for (const int w : {1, 31, 32}) {
    int D = 0;
    for (int k = 0; k < w; ++k) D += ((s >> k) & 1u) != ((t >> k) & 1u);
    CHECK(popcount((s ^ t) & sbk_mask(w)) == D && popcount(~(s ^ t) & sbk_mask(w)) == w - D);
  }
  std::printf("ok  mask and term\n");
}

void test_pack() {
  for (const int n : {1, 5, 32, 33, 40}) {
    // each row on the heap with no slack: a read outside [0, n) is an ASan report
    std::vector<uint8_t> bits(n);
    for (int k = 0; k < n; ++k) bits[k] = (uint8_t)((k * 7 + 3) % 5 < 2);
    for (const int side : {0, 1}) {
      bool bad = false;
      const uint32_t word = sbk_pack(bits.data(), n, side, bad);
      CHECK(!bad);
      for (int k = 0; k < 32; ++k) {
        const uint32_t want = k < (n < 32 ? n : 32) ? bits[side ? n - 1 - k : k] : 0u;
        CHECK(((word >> k) & 1u) == want);
      }
    }
  }
  // a byte that is neither 0 nor 1 is reported where the block holds it, and only there
  std::vector<uint8_t> bits(33, 0);
  bits[32] = 2;
  bool bad = false;
  sbk_pack(bits.data(), 33, 0, bad);
  CHECK(!bad);  // qubit 32 is outside the left block
  sbk_pack(bits.data(), 33, 1, bad);
  CHECK(bad);  // and is bit 0 of the right block
  bits[32] = 0, bits[0] = 255, bad = false;
  sbk_pack(bits.data(), 33, 0, bad);
  CHECK(bad);
  std::printf("ok  pack\n");
}

void test_tasks() {
  for (const int U : {1, 3, 7, 64, 65})
    for (const int chunk : {1, 2, 3, 64, 100}) {
      const long long n_pairs = 5;
      const int nc = sbk_n_chunks(U, chunk);
      CHECK(nc == (U + chunk - 1) / chunk);
      std::vector<int> seen((size_t)n_pairs * U, 0);
      for (long long t = 0; t < n_pairs * nc; ++t) {
        long long pair;
        int u0, u1;
        sbk_task(t, U, chunk, pair, u0, u1);
        CHECK(pair >= 0 && pair < n_pairs && u0 >= 0 && u0 < u1 && u1 <= U && u1 - u0 <= chunk);
        for (int u = u0; u < u1; ++u) ++seen[(size_t)pair * U + u];
      }
      for (const int v : seen) CHECK(v == 1);
    }
  std::printf("ok  tasks\n");
}

void test_chunk() {
  const int Ms[] = {1, 2, 63, 64, 65, 257, 1000, 4095, 4096, 4097, 100000};
  for (const int M : Ms)
    for (const int U : {1, 3, 64, 1000})
      for (const long long n_pairs : {1ll, 10ll, 3000ll, 125250ll}) {
        const int chunk = sbk_chunk(U, M, n_pairs);
        CHECK(chunk >= 1 && chunk <= U && chunk <= SBK_MAX_CHUNK);
        // what a workgroup stages: whole rows of M rounded up to 4 words, or pieces of one row
        if (M <= SBK_STAGE_WORDS) CHECK((long long)chunk * ((M + 3) / 4 * 4) <= SBK_STAGE_WORDS);
        else CHECK(chunk == 1);
        // no larger than leaves the call about SBK_LAUNCH_TASKS tasks, where it has the work for them
        if (chunk > 1) CHECK(n_pairs * sbk_n_chunks(U, chunk) >= SBK_LAUNCH_TASKS / 2);
      }
  CHECK(sbk_chunk(64, 64, 125250) == 64 && sbk_chunk(64, 64, 1) == 1 && sbk_chunk(1000, 2, 6144) == 64 && sbk_chunk(1000, 2, 41) == 20 && sbk_chunk(64, 257, 125250) == 15);
  std::printf("ok  chunk\n");
}

void test_parts() {
  for (const int M : {1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 5000}) {
    const int blocks = sbk_a_blocks(M), parts = sbk_parts(M);
    CHECK(blocks == (M + 63) / 64 && parts == (blocks == 1 ? 4 : blocks == 2 ? 2 : 1));
    const int rows[] = {M < SBK_STAGE_WORDS ? M : SBK_STAGE_WORDS, 1, 3, 4, 5, 904};
    for (const int bn : rows) {
      std::vector<int> seen(bn, 0);
      CHECK(sbk_part_lo(0, parts, bn) == 0 && sbk_part_lo(parts, parts, bn) == bn);
      for (int p = 0; p < parts; ++p) {
        const int lo = sbk_part_lo(p, parts, bn), hi = sbk_part_lo(p + 1, parts, bn);
        CHECK(lo <= hi && hi <= bn && (lo == hi || lo % 4 == 0));  // a piece that holds words starts where a 16-byte read may start
        for (int b = lo; b < hi; ++b) ++seen[b];
      }
      for (const int v : seen) CHECK(v == 1);
    }
  }
  std::printf("ok  parts\n");
}

void test_widths_and_groups() {
  for (int nw = 1; nw <= 32; ++nw) {
    int at = 0, launches = 0;
    while (at < nw) {
      const int g = sbk_group(nw, at);
      CHECK((g == 1 || g == 2 || g == 4 || g == 8) && g <= SBK_GROUP && at + g <= nw);
      at += g, ++launches;
    }
    CHECK(at == nw && launches <= nw / 8 + 3);
  }
  const int32_t good[] = {1, 31, 32}, high[] = {1, 33}, flat[] = {2, 2}, zero[] = {0, 1}, five[] = {1, 5, 6};
  CHECK(sbk_bad_width(3, good, 32) == -1 && sbk_bad_width(3, good, 40) == -1 && sbk_bad_width(3, good, 31) == 2);
  CHECK(sbk_bad_width(2, high, 40) == 1 && sbk_bad_width(2, flat, 8) == 1 && sbk_bad_width(2, zero, 8) == 0 && sbk_bad_width(3, five, 5) == 2);
  CHECK(sbk_batch_pairs(0, 4, 64) == 1 && sbk_batch_pairs(1 << 20, 4, 64) == (1 << 20) / (4 * 64 * 8 + 8));
  std::printf("ok  widths and groups\n");
}

void test_overflow() {
  // U M^2 2^w <= 2^62
  CHECK(sbk_fits(1, 1, 32) && sbk_fits(3, 130, 32));
  CHECK(sbk_fits(1, 1 << 15, 32) && !sbk_fits(1, (1 << 15) + 1, 32) && !sbk_fits(2, 1 << 15, 32));  // 2^30 2^32 = 2^62
  CHECK(sbk_fits(1ll << 30, 1, 32) && !sbk_fits((1ll << 30) + 1, 1, 32));
  CHECK(sbk_fits(2, 1ll << 30, 1) && !sbk_fits(3, 1ll << 30, 1));  // 2 2^60 2 = 2^62
  CHECK(sbk_fits(0x7fffffffll, 1, 31) && !sbk_fits(0x7fffffffll, 2, 31) && !sbk_fits(0x7fffffffll, 0x7fffffffll, 1));  // the product passes 2^64
  std::printf("ok  overflow\n");
}

}  // namespace

int main() {
  test_mask_and_term();
  test_pack();
  test_tasks();
  test_chunk();
  test_parts();
  test_widths_and_groups();
  test_overflow();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
