// The integer side of the Pauli-string estimator (csrc/qk_local_plan.h: sst_*): the string packer at the qubit counts where a group
// begins or ends (1, 31, 32, 33, 64, 65, 128) with its bad flag, match and sign of a (shot record, string record) against a loop
// over the qubits on random records (the identity, a full-weight string and a staged record included), the cut of the work into
// tasks (every (state, string block, shot) exactly once, for several sizes and cuts), the bound that keeps an int32 partial from
// overflowing at its boundary and the cut the driver picks against it, and the strings of a batch.  Every expected value is
// restated here from the definitions, not taken from the header.  Built with g++ -fsanitize=address,undefined and run by
// tests/test_shot_strings_plan.py; prints one line per section, exits 1 on a mismatch.
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

const int QUBITS[] = {1, 31, 32, 33, 64, 65, 128};

uint32_t next(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// tables on the heap with no slack: a read outside [0, n) is an ASan report
std::vector<uint8_t> random_string(const int n, uint32_t& seed, const int kind) {
  std::vector<uint8_t> c(n);
  for (int k = 0; k < n; ++k) {
    const uint32_t r = next(seed) >> 16;
    c[k] = kind == 0 ? 0 : kind == 1 ? (uint8_t)(1 + r % 3) : (r % 4 == 0 ? (uint8_t)(1 + (r >> 2) % 3) : 0);  // identity, full weight, sparse
  }
  return c;
}

void test_pack() {
  uint32_t seed = 1;
  for (const int n : QUBITS)
    for (const int kind : {0, 1, 2}) {
      const std::vector<uint8_t> c = random_string(n, seed, kind);
      const int groups = (n + 31) / 32;
      CHECK(sst_words(n) == 2 * groups);
      std::vector<uint32_t> rec(2 * groups, 0xffffffffu);
      bool bad = false;
      sst_pack_string(c.data(), n, rec.data(), bad);
      CHECK(!bad);
      for (int k = 0; k < 32 * groups; ++k) {
        const uint32_t s1 = (rec[2 * (k / 32)] >> (k % 32)) & 1u, s2 = (rec[2 * (k / 32) + 1] >> (k % 32)) & 1u;
        if (k < n) CHECK(s1 == (c[k] & 1u) && s2 == (uint32_t)(c[k] >> 1));
        else CHECK(s1 == 0 && s2 == 0);  // pad bits are 0 in both planes
      }
      if (kind == 0)
        for (const uint32_t v : rec) CHECK(v == 0);  // the identity is the zero record
      for (const int at : {0, n - 1, n / 2})
        for (const int code : {4, 7, 255}) {
          std::vector<uint8_t> t = c;
          t[at] = (uint8_t)code;
          bad = false;
          sst_pack_string(t.data(), n, rec.data(), bad);
          CHECK(bad);
        }
    }
  std::printf("ok  pack\n");
}

void test_match_and_sign() {
  uint32_t seed = 7;
  for (const int n : QUBITS) {
    const int groups = (n + 31) / 32;
    for (int rep = 0; rep < 200; ++rep) {
      std::vector<uint8_t> bits(n), bases(n);
      for (int k = 0; k < n; ++k) bits[k] = (uint8_t)((next(seed) >> 16) & 1u), bases[k] = (uint8_t)(1 + (next(seed) >> 16) % 3);
      std::vector<uint8_t> c = random_string(n, seed, rep % 3);
      if (rep % 2 == 0)  // make it a match: the string agrees with the bases on its support
        for (int k = 0; k < n; ++k)
          if (c[k]) c[k] = bases[k];
      if (rep % 8 == 2 && rep % 3 != 0) c[n - 1] = (uint8_t)(1 + bases[n - 1] % 3);  // one mismatch, on the last qubit
      bool want_match = true;
      int want_sign = 1;
      for (int k = 0; k < n; ++k)
        if (c[k]) want_match = want_match && c[k] == bases[k], want_sign *= 1 - 2 * bits[k];
      std::vector<uint32_t> shot(3 * groups), str(2 * groups);
      bool f = false, h = false, bad = false;
      shk_pack(bits.data(), bases.data(), n, shot.data(), f, h);
      sst_pack_string(c.data(), n, str.data(), bad);
      CHECK(!f && !h && !bad);
      bool match = !want_match;
      int sign = 0;
      sst_test(shot.data(), str.data(), groups, match, sign);
      CHECK(match == want_match && sign == want_sign);
      if (rep % 3 == 0) CHECK(match && sign == 1);  // the identity matches every shot with sign +1
      // a staged record: the same words in a row of shk_stride words
      std::vector<uint32_t> staged(shk_stride(groups), 0xdeadbeefu);
      for (int k = 0; k < 3 * groups; ++k) staged[k] = shot[k];
      sst_test(staged.data(), str.data(), groups, match, sign);
      CHECK(match == want_match && sign == want_sign);
    }
  }
  std::printf("ok  match and sign\n");
}

void test_tasks() {
  for (const int shots : {1, 255, 256, 257, 1000, 4100})
    for (const int tc : {1, 2, 3, 16, 100})
      for (const int blocks : {1, 3}) {
        const long long n_states = 3;
        const int nc = (shots + 255) / 256, ranges = (nc + tc - 1) / tc;
        CHECK(sst_chunks(shots) == nc && sst_ranges(shots, tc) == ranges);
        std::vector<int> seen((size_t)n_states * blocks * shots, 0);
        for (long long t = 0; t < n_states * blocks * ranges; ++t) {
          long long state;
          int block, t0, t1;
          sst_task(t, blocks, shots, tc, state, block, t0, t1);
          CHECK(state >= 0 && state < n_states && block >= 0 && block < blocks && t0 >= 0 && t0 < t1 && t1 <= shots && t1 - t0 <= tc * 256 && t0 % 256 == 0);
          if (state < 0 || state >= n_states || block < 0 || block >= blocks || t0 < 0 || t1 > shots) continue;
          for (int s = t0; s < t1; ++s) ++seen[((size_t)state * blocks + block) * shots + s];
        }
        for (const int v : seen) CHECK(v == 1);
      }
  CHECK(sst_blocks(1) == 1 && sst_blocks(64) == 1 && sst_blocks(65) == 2 && sst_blocks(3712) == 58 && sst_blocks(0x7fffffff) == 1 << 25);
  CHECK(SST_BLOCK == 64 && SST_STAGE_SHOTS == 256 && SST_ROW == 128);
  std::printf("ok  tasks\n");
}

void test_overflow_bound() {
  // a partial count is at most the shots of the task, a partial sum at most that in magnitude: both must fit an int32
  const long long mc = sst_max_chunks();
  CHECK(mc * 256 <= 0x7fffffffll && (mc + 1) * 256 > 0x7fffffffll && mc == 8388607);
  const int xs[] = {1, 2, 256, 257, 1000, 4100, 1 << 20, 0x7fffffff};
  for (const int shots : xs)
    for (const long long units : {1ll, 10ll, 3000ll, 29000ll, 1ll << 40}) {
      const int tc = sst_task_chunks(shots, units);
      CHECK(tc >= 1 && tc <= sst_chunks(shots) && (long long)tc * 256 <= 0x7fffffffll);
      // the longest range of the cut, from the task function itself
      long long state;
      int block, t0, t1;
      sst_task(0, 1, shots, tc, state, block, t0, t1);
      CHECK((long long)t1 - t0 <= 0x7fffffffll && t1 - t0 >= 1);
      // no larger than leaves the call about SST_LAUNCH_TASKS tasks, where it has the work for them
      if (tc > 1) CHECK(units * sst_ranges(shots, tc) >= SST_LAUNCH_TASKS / 2);
    }
  CHECK(sst_task_chunks(1000, 29000) == 4 && sst_task_chunks(1000, 1) == 1 && sst_task_chunks(1 << 20, 1024) == 2048 && sst_task_chunks(1 << 20, 1) == 2);
  // the bound, not the fill or the shots, decides: 2^23 chunks of which a task may take 2^23 - 1, so two ranges, the second of 255 shots
  CHECK(sst_chunks(0x7fffffff) == 1 << 23 && sst_task_chunks(0x7fffffff, 1ll << 40) == 8388607 && sst_ranges(0x7fffffff, 8388607) == 2);
  long long state;
  int block, t0, t1;
  sst_task(1, 1, 0x7fffffff, 8388607, state, block, t0, t1);
  CHECK(state == 0 && block == 0 && t0 == 2147483392 && t1 == 0x7fffffff);
  sst_task(2, 1, 0x7fffffff, 8388607, state, block, t0, t1);
  CHECK(state == 1 && t0 == 0 && t1 == 2147483392);
  std::printf("ok  overflow bound\n");
}

void test_batches() {
  // per string: its record (8 bytes per group) and per state 8 bytes of each task row of its block and two int64 totals
  CHECK(sst_batch_strings(0, 20, 500, 1, 0) == 1 && sst_batch_strings(63 * (8 + 500 * 24), 20, 500, 1, 0) == 63);
  CHECK(sst_batch_strings(1ll << 30, 20, 500, 1, 0) == ((1ll << 30) / (8 + 500 * 24)) / 64 * 64);
  CHECK(sst_batch_strings(1ll << 30, 128, 3, 4, 0) == ((1ll << 30) / (32 + 3 * 48)) / 64 * 64);
  CHECK(sst_batch_strings(1ll << 30, 20, 500, 1, 7) == 7 && sst_batch_strings(1ll << 30, 20, 500, 1, 1) == 1 && sst_batch_strings(0, 20, 500, 1, 7) == 1);
  for (const long long room : {0ll, 1000ll, 1ll << 20, 1ll << 34})
    for (const long long cap : {0ll, 1ll, 7ll, 100000ll}) {
      const long long b = sst_batch_strings(room, 65, 9, 3, cap);
      CHECK(b >= 1 && (cap == 0 || b <= cap));
      if (b > 1 && cap == 0) CHECK(b * (24 + 9 * (24 + 16)) <= room);  // what the batch takes fits the room
      if (b >= 64 && cap == 0) CHECK(b % 64 == 0);
    }
  std::printf("ok  batches\n");
}

}  // namespace

int main() {
  test_pack();
  test_match_and_sign();
  test_tasks();
  test_overflow_bound();
  test_batches();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
