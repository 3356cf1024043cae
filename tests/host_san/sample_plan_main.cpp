// The host-side plan of the measurement shots (csrc/qk_local_plan.h: the SMP_* kinds) on a hand-made set over 6 sites: Philox4x32-10
// against Random123's known answers and the uniform built from it, the shot tiles of a state (every shot once, ragged tails), the
// regions of a chain's slot against what the launches index, the task counts, the per-site launch lists of a chain batch that does
// not start at chain 0, the same work whatever the cut into chain batches, the environment pass that keeps the right environments
// only, and the check of the basis codes.  Every expected value is restated here from the definitions, not taken from the header.
// Built with g++ -fsanitize=address,undefined and run by tests/test_sample_plan.py; prints one line per section, exits 1 on a
// mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <cstdio>
#include <map>
#include <vector>

using namespace qkl;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr int N = 6, N1 = N + 1, NS = 3;
const int32_t TRU[NS * N1] = {
    1, 2, 4,  8,  4,  2, 1,
    1, 2, 17, 70, 33, 2, 1,
    1, 2, 4,  50, 64, 4, 1,
};
const int PAD[NS * N1] = {
    16, 16, 16, 16, 16, 16, 16,
    16, 16, 32, 80, 48, 16, 16,
    16, 16, 16, 64, 64, 16, 16,
};
const int PMAX[NS] = {16, 80, 64};
constexpr int MAXPAD = 80;

long long b64(const long long m, const long long n) { return ((m + 63) / 64) * ((n + 63) / 64); }

EnvSizes sizes() {
  EnvSizes z;
  env_sizes(TRU, NS, N, MAXPAD, LOC_RMUL, false, z);
  return z;
}

void test_philox() {
  const Philox4 a = smp_philox(0, 0, 0, 0, 0, 0);
  CHECK(a.x[0] == 0x6627e8d5u && a.x[1] == 0xe169c58du && a.x[2] == 0xbc57ac4cu && a.x[3] == 0x9b00dbd8u);
  const uint32_t f = 0xffffffffu;
  const Philox4 b = smp_philox(f, f, f, f, f, f);
  CHECK(b.x[0] == 0x408f276du && b.x[1] == 0x41c83b0eu && b.x[2] == 0xa20bc7c6u && b.x[3] == 0x6d5451fdu);
  // the uniform: counter (site, shot, state, 0), key = the halves of the seed, 53 bits of the first two words
  const uint64_t seed = 0x8000000000000011ull;
  const Philox4 c = smp_philox(4, 3, 2, 0, 0x11u, 0x80000000u);
  const double want = (double)(((uint64_t)(c.x[0] >> 5) << 26) + (c.x[1] >> 6)) / 9007199254740992.0;
  CHECK(smp_uniform(seed, 2, 3, 4) == want);
  double lo = 1.0, hi = 0.0, sum = 0.0;
  for (uint32_t shot = 0; shot < 4000; ++shot) {
    const double u = smp_uniform(seed, 7, shot, shot % 13);
    lo = std::min(lo, u), hi = std::max(hi, u), sum += u;
  }
  CHECK(lo >= 0.0 && hi < 1.0 && sum > 0.45 * 4000 && sum < 0.55 * 4000);
  std::printf("ok  philox\n");
}

void test_tiles() {
  const EnvSizes z = sizes();
  const int cases[][2] = {{70, 64}, {1, 64}, {64, 64}, {65, 64}, {100, 32}, {17, 16}, {128, 64}};
  for (const auto& cs : cases) {
    const int shots = cs[0], tile = cs[1];
    const SmpChains c = list_smp_chains(z, 1, 2, shots, tile);  // states 1 and 2
    const int tiles = (shots + tile - 1) / tile;
    CHECK(smp_tiles(shots, tile) == tiles);
    CHECK((int)c.cent.size() == 2 * tiles);
    for (int i = 0; i < 2; ++i) {
      std::vector<int> seen(shots, 0);
      for (int t = 0; t < tiles; ++t) {
        const size_t e = (size_t)i * tiles + t;
        CHECK(c.cent[e] == i && c.shot0[e] == t * tile);
        CHECK(c.rows[e] >= 1 && c.rows[e] <= tile && (t + 1 < tiles ? c.rows[e] == tile : c.rows[e] == shots - t * tile));
        for (int r = 0; r < c.rows[e]; ++r) ++seen[c.shot0[e] + r];
        const int R = smp_rows_pad(c.rows[e]);
        CHECK(R % 16 == 0 && R >= c.rows[e] && R < c.rows[e] + 16);
        CHECK(c.slot[e] == 14ll * PMAX[1 + i] * R);
      }
      for (int s = 0; s < shots; ++s) CHECK(seen[s] == 1);
    }
  }
  std::printf("ok  tiles\n");
}

// the regions of a slot, in doubles, for P and R: V [P][R], W [R][2P], W' [P][2R], Q [2R][P], each twice (re, im)
void test_slot() {
  const long long sizes_[4] = {2, 4, 4, 4};  // planes x extent in units of P R
  const int at[5] = {smp_V(), smp_W(), smp_Ws(), smp_Q(), smp_size()};
  for (int r = 0; r < 4; ++r) CHECK(at[r + 1] - at[r] == sizes_[r]);
  CHECK(at[0] == 0);
  // the largest element every launch touches, for state 1 (P = 80) and a ragged tile of 6 shots (R = 16), lies inside its region
  const int P = PMAX[1], R = smp_rows_pad(6);
  const long long PR = (long long)P * R;
  for (int k = 0; k < N; ++k) {
    const long long l = PAD[N1 + k], r = PAD[N1 + k + 1];
    CHECK((l - 1) * R + (R - 1) < PR);                    // V[b][row], ld R, plane P R
    CHECK((R - 1) * 2 * r + 2 * r - 1 < 2 * PR);          // W[row][(t, b')], ld 2 r, plane 2 P R
    CHECK((r - 1) * 2 * R + 2 * R - 1 < 2 * PR);          // W'[b'][(o, row)], ld 2 R, plane 2 P R
    CHECK((2ll * R - 1) * r + r - 1 < 2 * PR);            // Q[(o, row)][a'], ld r, plane 2 P R
  }
  std::printf("ok  slot\n");
}

long long expected_tasks(const int kind, const int k, const int* p, const int R) {
  if (kind == SMP_W) return b64(R, 2 * p[k + 1]);      // W [R][2 pad_{k+1}]
  if (kind == SMP_Q) return b64(2 * R, p[k + 1]);      // Q [2 R][pad_{k+1}]
  return R / 16;                                       // 16-row chunks of the shots
}

void test_counts() {
  const EnvSizes z = sizes();
  const int kinds[4] = {SMP_W, SMP_ROT, SMP_Q, SMP_DRAW};
  for (int j = 0; j < 4; ++j) CHECK(SMP_KINDS[j] == kinds[j]);
  CHECK(SMP_W >= 0 && SMP_Q >= 0 && SMP_ROT < 0 && SMP_DRAW < 0 && !conj_b(SMP_W) && !conj_b(SMP_Q));
  for (int s = 0; s < NS; ++s)
    for (const int R : {16, 48, 64, 128})
      for (int k = 0; k < N; ++k)
        for (const int kind : kinds) CHECK(smp_task_count(kind, k, &z.pad[(size_t)s * N1], R) == expected_tasks(kind, k, PAD + s * N1, R));
  // a chain's tasks and weight: 70 shots of state 1 are tiles of 64 and 6 rows
  const SmpChains c = list_smp_chains(z, 1, 1, 70, 64);
  CHECK(c.cent.size() == 2);
  for (size_t e = 0; e < c.cent.size(); ++e) {
    const int R = e == 0 ? 64 : 16;
    long long nt = 0;
    for (int k = 0; k < N; ++k)
      for (const int kind : kinds) nt += expected_tasks(kind, k, PAD + N1, R);
    CHECK(c.ntasks[e] == nt && c.weight[e] >= c.slot[e] + nt);
  }
  std::printf("ok  counts\n");
}

void test_lists() {
  const EnvSizes z = sizes();
  const SmpChains c = list_smp_chains(z, 0, NS, 70, 64);  // 6 chains: (state, tile) = (0,0) (0,1) (1,0) (1,1) (2,0) (2,1)
  CHECK(c.cent.size() == 6);
  std::vector<Task2> tasks;
  std::vector<long long> first;
  const size_t c0 = 1, nc = 4;  // a batch that starts inside state 0 and ends inside state 2
  smp_lists(z, 0, c, c0, nc, tasks, first);
  CHECK(first.size() == 4 * N + 1 && first[0] == 0 && first.back() == (long long)tasks.size());
  const int kinds[4] = {SMP_W, SMP_ROT, SMP_Q, SMP_DRAW};
  long long total = 0;
  for (int k = 0; k < N; ++k)
    for (int j = 0; j < 4; ++j) {
      const size_t li = 4 * k + j;
      long long at = first[li];
      for (size_t e = 0; e < nc; ++e) {  // chain-major, blocks ascending
        const int s = c.cent[c0 + e], R = smp_rows_pad(c.rows[c0 + e]);
        const long long want = expected_tasks(kinds[j], k, PAD + s * N1, R);
        for (long long b = 0; b < want; ++b, ++at) CHECK(at < first[li + 1] && tasks[at].x == (int)e && tasks[at].y == (int)b);
      }
      CHECK(at == first[li + 1]);
      total += first[li + 1] - first[li];
    }
  long long nt = 0;
  for (size_t e = 0; e < nc; ++e) nt += c.ntasks[c0 + e];
  CHECK(total == nt);
  std::printf("ok  lists\n");
}

// the work of a call is the same whatever the cut: per launch, the (global chain, block) pairs of all batches together
void test_cuts() {
  const EnvSizes z = sizes();
  const SmpChains c = list_smp_chains(z, 0, NS, 150, 64);  // 9 chains
  const size_t nch = c.cent.size();
  CHECK(nch == 9);
  std::map<std::pair<int, long long>, int> ref;
  bool have_ref = false;
  long long all = 0;
  for (size_t e = 0; e < nch; ++e) all += c.weight[e];
  const long long rooms[] = {all, all / 2, c.weight[2] + c.weight[3], 1};
  for (const long long cap : {0ll, 1ll, 3ll, 100ll})
    for (const long long room : rooms) {
      const std::vector<size_t> cstart = chain_cut(c.weight, room, cap);
      CHECK(cstart.front() == 0 && cstart.back() == nch);
      std::map<std::pair<int, long long>, int> got;  // (launch, chain * 2^20 + block) -> times
      for (size_t cb = 0; cb + 1 < cstart.size(); ++cb) {
        const size_t c0 = cstart[cb], nc = cstart[cb + 1] - c0;
        CHECK(nc >= 1 && (cap == 0 || (long long)nc <= cap));
        long long w = 0;
        for (size_t e = c0; e < c0 + nc; ++e) w += c.weight[e];
        CHECK(nc == 1 || w <= room);
        std::vector<Task2> tasks;
        std::vector<long long> first;
        smp_lists(z, 0, c, c0, nc, tasks, first);
        for (size_t li = 0; li + 1 < first.size(); ++li)
          for (long long t = first[li]; t < first[li + 1]; ++t) ++got[{(int)li, ((long long)(c0 + tasks[t].x) << 20) + tasks[t].y}];
      }
      for (const auto& kv : got) CHECK(kv.second == 1);
      if (!have_ref) ref = got, have_ref = true;
      CHECK(got == ref);
    }
  std::printf("ok  cuts\n");
}

void test_env() {
  const EnvSizes z = sizes();
  CHECK(!z.keep_l && z.rmul == LOC_RMUL);
  for (int s = 0; s < NS; ++s) {
    long long need = 14ll * PMAX[s] * PMAX[s];
    for (int k = 1; k <= N; ++k) need += 2ll * PAD[s * N1 + k] * PAD[s * N1 + k];  // R_1 .. R_n only
    CHECK(z.need[s] == need && z.pmax[s] == PMAX[s]);
  }
  for (const int n : {1, 2, N}) {
    const Plan plan = sample_env_plan(n);
    CHECK((int)plan.size() == 2 * (n - 1));
    for (int j = 0; j < n - 1; ++j) CHECK(plan[2 * j] == std::make_pair((int)LOC_REV_T, j) && plan[2 * j + 1] == std::make_pair((int)LOC_REV_X, j));
  }
  // the tables of the reversed chain alone, for a batch other than the first: no L offsets
  EnvTables eb;
  env_tables(z, sample_env_plan(N), 1, 2, 0, eb);
  CHECK(eb.h_loff.empty() && eb.h_states[0] == 1 && eb.h_states[1] == 2 && eb.tot == z.need[1] + z.need[2]);
  CHECK(eb.first.size() == 2 * (N - 1) + 1);
  // a one-site chain has an empty plan and no tasks
  const int32_t one[2] = {1, 1};
  EnvSizes z1;
  env_sizes(one, 1, 1, 16, LOC_RMUL, false, z1);
  EnvTables e1;
  env_tables(z1, sample_env_plan(1), 0, 1, 0, e1);
  CHECK(e1.tasks.empty() && e1.first.size() == 1 && e1.h_roff[1] == 0);
  const SmpChains c1 = list_smp_chains(z1, 0, 1, 5, 64);
  CHECK(c1.cent.size() == 1 && c1.rows[0] == 5 && c1.ntasks[0] == 1 + 1 + 1 + 1);
  std::printf("ok  env\n");
}

void test_bases() {
  std::vector<uint8_t> b(70 * N, 3);
  CHECK(smp_bad_basis(b.data(), (long long)b.size()) == -1);
  b[5] = 1, b[6] = 2;
  CHECK(smp_bad_basis(b.data(), (long long)b.size()) == -1);
  b[200] = 0;
  CHECK(smp_bad_basis(b.data(), (long long)b.size()) == 200);
  b[100] = 4;
  CHECK(smp_bad_basis(b.data(), (long long)b.size()) == 100);
  CHECK(smp_bad_basis(b.data(), 100) == -1);
  std::printf("ok  bases\n");
}

}  // namespace

int main() {
  test_philox();
  test_tiles();
  test_slot();
  test_counts();
  test_lists();
  test_cuts();
  test_env();
  test_bases();
  if (failures) std::printf("FAIL: %d check(s)\n", failures);
  return failures ? 1 : 0;
}
