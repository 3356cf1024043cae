// The integer side of the shadow kernel's shot-pair histograms (csrc/qk_local_plan.h: shk_*): the record packer at the qubit counts
// where a group begins or ends (1, 32, 33, 64, 65, 128) with its two bad flags, d of two records against a loop over the qubits at
// those counts (all-pad high bits included), the cut of the work into tasks (every (pair, x block) exactly once, for any cut and
// ragged ends), the bound that keeps a 32-bit counter from overflowing at its boundary and the cut the driver picks against it, the
// LDS layout for every n up to 128 against the 160 KiB of a CU, the pieces of a staged pass, and the pairs of a batch.  Every
// expected value is restated here from the definitions, not taken from the header.  Built with g++ -fsanitize=address,undefined and
// run by tests/test_shadow_plan.py; prints one line per section, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <cstdio>
#include <vector>

using namespace qkl;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

const int QUBITS[] = {1, 5, 31, 32, 33, 64, 65, 96, 97, 128};

uint32_t next(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// one shot on the heap with no slack: a read outside [0, n) is an ASan report
struct Shot {
  std::vector<uint8_t> bits, bases;
  Shot(const int n, uint32_t& seed) : bits(n), bases(n) {
    for (int k = 0; k < n; ++k) bits[k] = (uint8_t)((next(seed) >> 16) & 1u), bases[k] = (uint8_t)(1 + (next(seed) >> 16) % 3);
  }
};

void test_pack() {
  uint32_t seed = 1;
  for (const int n : QUBITS) {
    const Shot s(n, seed);
    const int groups = shk_groups(n);
    CHECK(groups == (n + 31) / 32 && shk_words(n) == 3 * groups && shk_bins(n) == 2 * n + 1);
    std::vector<uint32_t> rec(3 * groups, 0xffffffffu);
    bool bad_bit = false, bad_code = false;
    shk_pack(s.bits.data(), s.bases.data(), n, rec.data(), bad_bit, bad_code);
    CHECK(!bad_bit && !bad_code);
    for (int k = 0; k < 32 * groups; ++k) {
      const uint32_t p0 = (rec[3 * (k / 32)] >> (k % 32)) & 1u, p1 = (rec[3 * (k / 32) + 1] >> (k % 32)) & 1u, p2 = (rec[3 * (k / 32) + 2] >> (k % 32)) & 1u;
      if (k < n) CHECK(p0 == s.bits[k] && p1 == (s.bases[k] & 1u) && p2 == (uint32_t)(s.bases[k] >> 1));
      else CHECK(p0 == 0 && p1 == 0 && p2 == 0);  // pad bits are 0 in all planes
    }
    // a bad bit and a bad code are flagged apart, wherever they sit
    for (const int at : {0, n - 1, n / 2}) {
      for (const int what : {0, 1, 2}) {
        Shot t = s;
        if (what == 0) t.bits[at] = 2;
        if (what == 1) t.bases[at] = 0;
        if (what == 2) t.bases[at] = 4;
        bad_bit = bad_code = false;
        shk_pack(t.bits.data(), t.bases.data(), n, rec.data(), bad_bit, bad_code);
        CHECK(bad_bit == (what == 0) && bad_code == (what != 0));
      }
    }
  }
  std::printf("ok  pack\n");
}

void test_d() {
  uint32_t seed = 7;
  for (const int n : QUBITS) {
    const int groups = shk_groups(n);
    for (int rep = 0; rep < 40; ++rep) {
      Shot a(n, seed), b(n, seed);
      if (rep == 0) b = a;                                                    // d = n
      if (rep == 1) { b = a; for (auto& v : b.bits) v ^= 1; }                 // d = -n
      if (rep == 2) { for (int k = 0; k < n; ++k) b.bases[k] = (uint8_t)(1 + a.bases[k] % 3); }  // d = 0: no basis shared
      int want = 0;
      for (int k = 0; k < n; ++k)
        if (a.bases[k] == b.bases[k]) want += a.bits[k] == b.bits[k] ? 1 : -1;
      std::vector<uint32_t> ra(3 * groups), rb(3 * groups);
      bool f = false, h = false;
      shk_pack(a.bits.data(), a.bases.data(), n, ra.data(), f, h);
      shk_pack(b.bits.data(), b.bases.data(), n, rb.data(), f, h);
      CHECK(shk_d(ra.data(), rb.data(), groups) == want && shk_d(rb.data(), ra.data(), groups) == want);
      if (rep == 0) CHECK(want == n);
      if (rep == 1) CHECK(want == -n);
      if (rep == 2) CHECK(want == 0);
      // a staged record: the same words in a row of shk_stride words
      std::vector<uint32_t> staged(shk_stride(groups), 0xdeadbeefu);
      CHECK(shk_stride(groups) % 4 == 0 && shk_stride(groups) >= 3 * groups && shk_stride(groups) < 3 * groups + 4);
      for (int k = 0; k < 3 * groups; ++k) staged[k] = rb[k];
      CHECK(shk_d(ra.data(), staged.data(), groups) == want);
    }
  }
  std::printf("ok  d\n");
}

void test_tasks() {
  for (const int shots : {1, 63, 64, 65, 257, 1000, 4100})
    for (const int tb : {1, 2, 3, 16, 100}) {
      const long long n_pairs = 5;
      const int nxb = shk_x_blocks(shots), nt = shk_pair_tasks(shots, tb);
      CHECK(nxb == (shots + 63) / 64 && nt == (nxb + tb - 1) / tb);
      std::vector<int> seen((size_t)n_pairs * nxb, 0);
      for (long long t = 0; t < n_pairs * nt; ++t) {
        long long pair;
        int b0, b1;
        shk_task(t, shots, tb, pair, b0, b1);
        CHECK(pair >= 0 && pair < n_pairs && b0 >= 0 && b0 < b1 && b1 <= nxb && b1 - b0 <= tb);
        for (int b = b0; b < b1; ++b) ++seen[(size_t)pair * nxb + b];
      }
      for (const int v : seen) CHECK(v == 1);
    }
  std::printf("ok  tasks\n");
}

void test_counter_bound() {
  // private: one increment per (block, y shot) at most; shared: 64
  CHECK(shk_max_blocks(SHK_PRIVATE, 1) == 0xffffffffll && shk_max_blocks(SHK_PRIVATE, 0xffffffffll) == 1 && shk_max_blocks(SHK_PRIVATE, 0x7fffffffll) == 2);
  CHECK(shk_max_blocks(SHK_PRIVATE, 65536) == 65535 && shk_max_blocks(SHK_PRIVATE, 65537) == 65535 && shk_max_blocks(SHK_PRIVATE, 65535) == 65537);
  CHECK(shk_max_blocks(SHK_SHARED, 1) == 0xffffffffll / 64 && shk_max_blocks(SHK_SHARED, 1 << 14) == 4095);
  for (const long long ty : {1ll, 2ll, 1000ll, 65536ll, 1ll << 20, 0x7fffffffll})
    for (const ShkLayout lay : {SHK_PRIVATE, SHK_SHARED}) {
      const long long per = ty * (lay == SHK_SHARED ? 64 : 1), mb = shk_max_blocks(lay, ty);
      CHECK(mb * per <= SHK_COUNTER_MAX && (mb + 1) * per > SHK_COUNTER_MAX);
    }
  // the cut the driver picks respects the bound, and the layout it is used with
  const int xs[] = {1, 2, 64, 65, 128, 129, 1000, 4100, 1 << 20, 0x7fffffff};
  for (const int tx : xs)
    for (const int ty : xs)
      for (const long long n_pairs : {1ll, 10ll, 3000ll, 125250ll}) {
        const ShkLayout lay = shk_layout(60, tx, ty);
        CHECK((lay == SHK_SHARED) == ((long long)tx * ty <= SHK_SHARED_PAIRS));
        const int tb = shk_task_blocks(lay, tx, ty, n_pairs);
        CHECK(tb >= 1 && tb <= shk_x_blocks(tx));
        // the most increments one counter can take in a task
        const unsigned __int128 most = lay == SHK_SHARED ? (unsigned __int128)tx * ty : (unsigned __int128)tb * ty;
        CHECK(most <= (unsigned __int128)SHK_COUNTER_MAX);
        // no larger than leaves the call about SHK_LAUNCH_TASKS tasks, where it has the work for them
        if (tb > 1) CHECK(n_pairs * shk_pair_tasks(tx, tb) >= SHK_LAUNCH_TASKS / 2);
      }
  CHECK(shk_task_blocks(SHK_PRIVATE, 1000, 1000, 125250) == 16 && shk_task_blocks(SHK_PRIVATE, 1000, 1000, 1) == 1 && shk_task_blocks(SHK_PRIVATE, 4100, 4100, 512) == 16);
  CHECK(shk_task_blocks(SHK_PRIVATE, 0x7fffffff, 0x7fffffff, 1 << 20) == 2);  // the bound, not the fill, decides
  std::printf("ok  counter bound\n");
}

void test_layout() {
  for (int n = 1; n <= SHK_MAX_QUBITS; ++n) {
    CHECK(shk_stage_bytes(n) == SHK_STAGE_SHOTS * shk_stride(shk_groups(n)) * 4);
    for (const ShkLayout lay : {SHK_PRIVATE, SHK_SHARED}) {
      const int waves = shk_waves(n, lay), lds = shk_lds_bytes(n, lay);
      CHECK(waves >= 2 && waves <= 4 && lds <= 160 * 1024 && lds <= SHK_LDS_BYTES);
      const int counters = lay == SHK_PRIVATE ? (2 * n + 1) * 64 * waves : (2 * n + 1) * waves;
      CHECK(lds == shk_stage_bytes(n) + 4 * counters);
      if (lay == SHK_SHARED) CHECK(waves == 4);
      // private: a further wave would not fit
      if (lay == SHK_PRIVATE && waves < 4) CHECK(shk_stage_bytes(n) + 4 * (2 * n + 1) * 64 * (waves + 1) > 160 * 1024);
    }
  }
  CHECK(shk_waves(60, SHK_PRIVATE) == 4 && shk_lds_bytes(60, SHK_PRIVATE) == 8192 + 121 * 1024 && shk_waves(100, SHK_PRIVATE) == 2 && shk_waves(128, SHK_PRIVATE) == 2);
  CHECK(shk_lds_bytes(128, SHK_PRIVATE) == 12288 + 257 * 512 && shk_lds_bytes(128, SHK_SHARED) == 12288 + 257 * 16);
  CHECK(shk_layout(60, 128, 128) == SHK_SHARED && shk_layout(60, 128, 129) == SHK_PRIVATE && shk_layout(1, 257, 257) == SHK_PRIVATE && shk_layout(128, 65, 65) == SHK_SHARED);
  std::printf("ok  layout\n");
}

void test_parts_and_batches() {
  for (int blocks = 1; blocks <= 9; ++blocks)
    for (int waves = 2; waves <= 4; ++waves) {
      const int parts = shk_parts(blocks, waves);
      CHECK(parts >= 1 && blocks * parts >= waves && (blocks >= waves ? parts == 1 : (blocks * (parts - 1) < waves)));
      for (const int bn : {1, 2, 3, 4, 255, 256}) {
        std::vector<int> seen(bn, 0);
        CHECK(shk_part_lo(0, parts, bn) == 0 && shk_part_lo(parts, parts, bn) == bn);
        for (int p = 0; p < parts; ++p) {
          const int lo = shk_part_lo(p, parts, bn), hi = shk_part_lo(p + 1, parts, bn);
          CHECK(lo <= hi && hi <= bn);
          for (int b = lo; b < hi; ++b) ++seen[b];
        }
        for (const int v : seen) CHECK(v == 1);
      }
    }
  CHECK(shk_batch_pairs(0, 60, 1) == 1 && shk_batch_pairs(1 << 20, 60, 1) == (1 << 20) / (8 + 3 * 121 * 8) && shk_batch_pairs(1 << 20, 128, 16) == (1 << 20) / (8 + 18 * 257 * 8));
  std::printf("ok  parts and batches\n");
}

}  // namespace

int main() {
  test_pack();
  test_d();
  test_tasks();
  test_counter_bound();
  test_layout();
  test_parts_and_batches();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
