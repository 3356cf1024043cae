// The host-side plan of the local sweeps (csrc/qk_local_plan.h) on three hand-made states over 7 sites: the scratch layout against
// need[s], the pair index and its inverse, the cut into state batches, the tables and task lists of a batch that does not start at
// state 0, and the chain batches of the Pauli strings.  Every expected value is restated here from the definitions, not taken from
// the header.  Built with g++ -fsanitize=address,undefined and run by tests/test_local_plan.py; prints one line per section,
// exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <climits>
#include <cstdio>
#include <map>
#include <numeric>
#include <vector>

using namespace qkl;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr int NS = 3, N = 7, N1 = N + 1;
const int32_t TRU[NS * N1] = {
    1, 2, 4,  8,  4,   2,  1, 1,   // pads to 16 everywhere
    1, 2, 17, 80, 150, 33, 2, 1,   // pads to 16, 16, 32, 80, 160, 48, 16, 16: 1 to 3 row blocks of 64, 1 to 10 chunks
    1, 2, 4,  65, 64,  4,  2, 1,   // pads to 16, 16, 16, 80, 64, 16, 16, 16
};
const int PAD[NS * N1] = {
    16, 16, 16, 16, 16,  16, 16, 16,
    16, 16, 32, 80, 160, 48, 16, 16,
    16, 16, 16, 80, 64,  16, 16, 16,
};
const int PMAX[NS] = {16, 160, 80};
constexpr int MAX_PAD = 160;

long long b64(const long long m, const long long n) { return ((m + 63) / 64) * ((n + 63) / 64); }
long long sq2(const int s, const int k) { return 2ll * PAD[s * N1 + k] * PAD[s * N1 + k]; }  // both planes of a pad_k x pad_k matrix

EnvSizes sizes(const bool pair, const int D, const bool keep_l) {
  EnvSizes z;
  env_sizes(TRU, NS, N, MAX_PAD, rmul(pair, D), keep_l, z);
  z.max_dist = D, z.n_pairs = pair ? n_pairs(D, N) : 0;
  return z;
}

struct Region {
  long long at, len;
};
// every region inside [0, need), no two overlapping; returns the doubles they cover
long long check_regions(std::vector<Region> r, const long long need) {
  std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.at < b.at; });
  long long sum = 0;
  for (size_t i = 0; i < r.size(); ++i) {
    CHECK(r[i].len > 0 && r[i].at >= 0 && r[i].at + r[i].len <= need);
    if (i) CHECK(r[i - 1].at + r[i - 1].len <= r[i].at);
    sum += r[i].len;
  }
  return sum;
}

void test_layout() {
  for (int pair = 0; pair < 2; ++pair)
    for (int D = 1; D <= 4; ++D)
      for (int keep_l = 0; keep_l < 2; ++keep_l) {
        const EnvSizes z = sizes(pair, D, keep_l);
        EnvTables eb;
        env_tables(z, Plan{}, 0, NS, 0, eb);
        const int rm = pair ? 26 + 24 * (D - 1) : 14;
        CHECK(z.rmul == rm && z.max_chunks == MAX_PAD / 16);
        long long base = 0;
        for (int s = 0; s < NS; ++s) {
          const long long P2 = (long long)PMAX[s] * PMAX[s];
          long long need = rm * P2;
          for (int k = 1; k <= N; ++k) need += sq2(s, k);
          for (int k = 0; keep_l && k < N; ++k) need += sq2(s, k);
          CHECK(z.pmax[s] == PMAX[s] && z.need[s] == need && eb.h_sbase[s] == base);
          for (int k = 0; k <= N; ++k) CHECK(z.pad[s * N1 + k] == PAD[s * N1 + k]);
          base += need;
          std::vector<Region> r{{at_L() * P2, 2 * P2}, {at_T() * P2, 4 * P2}, {at_W(0) * P2, 4 * P2}, {at_W(1) * P2, 4 * P2}};
          if (pair) {
            r.push_back({at_Tp() * P2, 4 * P2}), r.push_back({at_V(0) * P2, 4 * P2}), r.push_back({at_V(1) * P2, 4 * P2});
            for (int o = 0; o + 1 < D; ++o) {
              r.push_back({window_slot(o, D) * P2, 8 * P2});
              CHECK(window_slot(o + D - 1, D) == window_slot(o, D));  // origin o lives in slot o mod (D - 1)
            }
            for (int w = 0; w < 4 * (D - 1); ++w) r.push_back({window_tmp(w, D) * P2, 4 * P2});
          }
          for (int k = 1; k <= N; ++k) r.push_back({rm * P2 + eb.h_roff[s * N1 + k], sq2(s, k)});
          for (int k = 0; keep_l && k < N; ++k) r.push_back({rm * P2 + eb.h_loff[s * N1 + k], sq2(s, k)});
          CHECK(check_regions(r, need) == need);  // the regions tile need[s]: nothing is counted that no kernel addresses
          const std::vector<Region> slot{{chain_E() * P2, 2 * P2}, {chain_T() * P2, 4 * P2}};
          CHECK(check_regions(slot, chain_size() * P2) == 6 * P2);
        }
        CHECK(eb.tot == base);
        CHECK(eb.h_loff.size() == (keep_l ? (size_t)NS * N1 : 0));
      }
  std::printf("ok  layout\n");
}

void test_pair_index() {
  for (int n = 2; n <= 9; ++n)
    for (int D = 1; D <= n - 1; ++D) {
      int next = 0;
      for (int d = 1; d <= D; ++d)
        for (int k = 0; k + d <= n - 1; ++k, ++next) {
          CHECK(pair_index(d, k, n) == next);
          CHECK(pair_second(next, n) == k + d);
        }
      CHECK(n_pairs(D, n) == next && next == D * n - D * (D + 1) / 2);
    }
  std::printf("ok  pair index\n");
}

void check_cut(const std::vector<long long>& w, const long long each, const long long budget, const std::vector<int>& b) {
  const int ns = (int)w.size();
  CHECK(b.size() >= 2 && b.front() == 0 && b.back() == ns);
  for (size_t i = 0; i + 1 < b.size(); ++i) {
    CHECK(b[i] < b[i + 1]);  // consecutive, each state exactly once, at least one per batch
    long long sum = 0;
    for (int s = b[i]; s < b[i + 1]; ++s) sum += w[s] + each;
    if (sum > budget) CHECK(b[i + 1] - b[i] == 1);
    if (b[i + 1] < ns) CHECK(sum + w[b[i + 1]] + each > budget);  // the batch ended because the next state did not fit
  }
}

void test_batch_cut() {
  const EnvSizes z = sizes(true, 3, false);
  const std::vector<long long>& w = z.need;
  const long long each = 1000;
  const long long total = std::accumulate(w.begin(), w.end(), 0ll) + NS * each;
  const long long smallest = *std::min_element(w.begin(), w.end()) + each, largest = *std::max_element(w.begin(), w.end()) + each;
  CHECK((batch_cut(w, each, LLONG_MAX / 4) == std::vector<int>{0, NS}));  // unlimited: the single batch
  CHECK((batch_cut(w, each, total) == std::vector<int>{0, NS}));          // everything just fits
  CHECK((batch_cut(w, each, smallest - 1) == std::vector<int>{0, 1, 2, 3}));
  CHECK((batch_cut(w, each, 0) == std::vector<int>{0, 1, 2, 3}));
  CHECK((batch_cut(w, each, w[0] + w[1] + 2 * each) == std::vector<int>{0, 2, 3}));
  CHECK((batch_cut(w, each, total - 1) == std::vector<int>{0, 2, 3}));
  CHECK((batch_cut(w, each, largest) == std::vector<int>{0, 1, 2, 3}));  // state 0 does not fit beside state 1, nor 2 beside 1
  const long long budgets[] = {LLONG_MAX / 4, total, total - 1, w[1] + w[2] + 2 * each, w[0] + w[1] + 2 * each, largest, largest - 1, w[2] + each, smallest, smallest - 1, 1, 0};
  size_t batches = 1;
  for (const long long budget : budgets) {  // descending: a smaller budget never gives fewer batches
    const std::vector<int> b = batch_cut(w, each, budget);
    check_cut(w, each, budget, b);
    CHECK(b.size() - 1 >= batches);
    batches = b.size() - 1;
  }
  CHECK(batches == NS);
  CHECK((batch_cut({}, 0, 10) == std::vector<int>{0, 0}));
  std::printf("ok  batch cut\n");
}

long long expected_tasks(const int kind, const int step, const int* p, const int D) {
  const int o = N - 1 - step, k = step, live = std::min(k, D - 1);
  switch (kind) {
    case LOC_REV_T: return b64(p[o + 1], 2 * p[o]);
    case LOC_REV_X: return b64(p[o], p[o]);
    case LOC_FWD_T: return b64(p[k], 2 * p[k + 1]);
    case LOC_FWD_W: return 2 * b64(p[k + 1], 2 * p[k + 1]);
    case LOC_PAIR_T: return b64(p[k + 2], 2 * p[k + 1]);
    case LOC_PAIR_V: return 2 * b64(p[k + 1], 2 * p[k + 1]);
    case LOC_DIST_T: return 4 * live * b64(p[k], 2 * p[k + 1]);
    case LOC_DIST_X: return 4 * live * b64(p[k + 1], p[k + 1]);
    case LOC_DIST_RHO: return live * (p[k + 1] / 16);
    case LOC_BOND_M: return b64(p[k], p[k]);
    case LOC_BOND_TR: return p[k] / 16;
    case LOC_RHO: case LOC_PAIR_RHO: case LOC_ADMIT: case STR_LNEXT: return p[k + 1] / 16;
  }
  CHECK(!"a kind no plan of a state batch holds");
  return -1;
}

// every (entry, block) of tasks [t0, t1) exactly once, entry e having want[e] blocks
void check_launch(const std::vector<Task2>& tasks, const long long t0, const long long t1, const std::vector<long long>& want) {
  std::map<std::pair<int, int>, int> seen;
  for (long long t = t0; t < t1; ++t) {
    const Task2 q = tasks[t];
    CHECK(q.x >= 0 && q.x < (int)want.size() && q.y >= 0 && q.y < want[q.x]);
    CHECK((++seen[{q.x, q.y}] == 1));
  }
  CHECK(t1 - t0 == std::accumulate(want.begin(), want.end(), 0ll));
}

void test_tables(const char* name, const EnvSizes& z, const Plan& plan, const size_t launches) {
  const int s0 = 1, nb = 2;
  const long long part_per_state = 77;
  CHECK(plan.size() == launches);
  EnvTables eb;
  env_tables(z, plan, 0, NS, 0, eb);  // a first batch, so that the second call has tables to reuse
  env_tables(z, plan, s0, nb, part_per_state, eb);
  CHECK(eb.s0 == s0 && eb.nb == nb && eb.h_states == (std::vector<int32_t>{1, 2}) && eb.h_pmax == (std::vector<int32_t>{PMAX[1], PMAX[2]}));
  CHECK(eb.h_sbase == (std::vector<int64_t>{0, z.need[1]}) && eb.tot == z.need[1] + z.need[2]);
  CHECK(eb.h_roff.size() == (size_t)nb * N1 && eb.h_loff.size() == (z.keep_l ? (size_t)nb * N1 : 0));
  for (int i = 0; i < nb; ++i) {
    long long ro = 0;
    for (int k = 0; k <= N; ++k) {  // the running sums of this batch alone, from 0
      CHECK(eb.h_roff[i * N1 + k] == ro);
      if (k >= 1) ro += sq2(s0 + i, k);
    }
    for (int k = 0; z.keep_l && k <= N; ++k) {  // the L_k behind the R_k
      CHECK(eb.h_loff[i * N1 + k] == ro);
      ro += sq2(s0 + i, k);
    }
  }
  CHECK(eb.first.size() == plan.size() + 1 && eb.first.front() == 0 && eb.first.back() == (long long)eb.tasks.size());
  for (size_t li = 0; li < plan.size(); ++li) {
    CHECK(eb.first[li] <= eb.first[li + 1]);
    std::vector<long long> want(nb);
    for (int i = 0; i < nb; ++i) {
      want[i] = expected_tasks(plan[li].first, plan[li].second, &PAD[(s0 + i) * N1], z.max_dist);
      CHECK(task_count(plan[li].first, plan[li].second, &z.pad[(s0 + i) * N1], N, z.max_dist) == want[i]);
    }
    check_launch(eb.tasks, eb.first[li], eb.first[li + 1], want);
  }
  const size_t table_bytes[] = {eb.b_states, eb.b_pmax, eb.b_sbase, eb.b_roff, eb.b_tasks, eb.b_part, eb.b_tab, eb.b_env};
  for (const size_t b : table_bytes) CHECK(b % 256 == 0);
  CHECK(eb.b_states >= nb * 4 && eb.b_pmax >= nb * 4 && eb.b_sbase >= nb * 8 && eb.b_roff >= (size_t)nb * N1 * 8 && eb.b_tasks >= eb.tasks.size() * 8);
  CHECK(eb.b_tab == eb.b_states + eb.b_pmax + eb.b_sbase + (z.keep_l ? 2 : 1) * eb.b_roff + eb.b_tasks);
  CHECK(eb.b_part >= (size_t)nb * part_per_state * 8 && eb.b_env >= (size_t)eb.tot * 8 && eb.used() == eb.b_tab + eb.b_part + eb.b_env);
  std::printf("ok  tables and tasks: %s (%zu launches, %zu tasks)\n", name, plan.size(), eb.tasks.size());
}

// ---- chains ---------------------------------------------------------------------------------------------------------------------
constexpr int NSTR = 6;
const char* const STRINGS[NSTR] = {"IIIIIII", "XIIIIII", "IIIIIIZ", "IXYZIII", "ZIIIIIX", "IIIXZII"};
const int SUPP[NSTR][2] = {{-1, -1}, {0, 0}, {6, 6}, {1, 3}, {0, 6}, {3, 4}};

long long expected_chain_tasks(const int kind, const int k, const int* p, const uint8_t* codes, const int a, const int b) {
  const bool live = a <= k && k <= b;
  switch (kind) {
    case STR_T: return live ? b64(p[k], 2 * p[k + 1]) : 0;
    case STR_PAULI: return live && codes[k] ? p[k] / 16 : 0;
    case STR_X: return live ? b64(p[k + 1], p[k + 1]) : 0;
    case STR_CLOSE: return k == b ? p[k + 1] / 16 : 0;
  }
  return -1;
}

void test_chains() {
  std::vector<uint8_t> codes(NSTR * N);
  for (int m = 0; m < NSTR; ++m)
    for (int k = 0; k < N; ++k) codes[m * N + k] = (uint8_t)(STRINGS[m][k] == 'X' ? 1 : STRINGS[m][k] == 'Y' ? 2 : STRINGS[m][k] == 'Z' ? 3 : 0);
  std::vector<int32_t> supp;
  CHECK(string_supports(codes.data(), NSTR, N, supp) == -1 && supp.size() == 2 * NSTR);
  for (int m = 0; m < NSTR; ++m) CHECK(supp[2 * m] == SUPP[m][0] && supp[2 * m + 1] == SUPP[m][1]);
  {
    std::vector<uint8_t> bad = codes;
    std::vector<int32_t> s2;
    bad[4 * N + 5] = 4, bad[5 * N + 1] = 9;
    CHECK(string_supports(bad.data(), NSTR, N, s2) == 4 * N + 5);  // the first code that is no Pauli
  }
  const EnvSizes z = sizes(false, 1, true);
  const int s0 = 1, nb = 2;
  const Chains ch = list_chains(z, s0, nb, NSTR, codes.data(), supp);
  const size_t nch = (size_t)nb * (NSTR - 1);  // state-major, string order, the all-identity string has no chain
  CHECK(ch.cent.size() == nch && ch.cstr.size() == nch && ch.ntasks.size() == nch && ch.weight.size() == nch);
  for (size_t e = 0; e < nch; ++e) {
    const int i = (int)(e / (NSTR - 1)), m = 1 + (int)(e % (NSTR - 1));
    CHECK(ch.cent[e] == i && ch.cstr[e] == m);
    long long nt = 0;
    for (int k = 0; k < N; ++k)
      for (const int kind : {STR_T, STR_PAULI, STR_X, STR_CLOSE}) nt += expected_chain_tasks(kind, k, &PAD[(s0 + i) * N1], &codes[m * N], SUPP[m][0], SUPP[m][1]);
    CHECK(ch.ntasks[e] == nt);
    CHECK(ch.slot.size() == nch && ch.slot[e] == 6ll * PMAX[s0 + i] * PMAX[s0 + i]);
    CHECK(ch.weight[e] == 6ll * PMAX[s0 + i] * PMAX[s0 + i] + MAX_PAD / 16 + nt + 2);
  }
  const long long all = std::accumulate(ch.weight.begin(), ch.weight.end(), 0ll);
  const long long heaviest = *std::max_element(ch.weight.begin(), ch.weight.end());
  struct Cut {
    long long room, cap;
    size_t batches;  // 0: not stated
  };
  const Cut cuts[] = {{all, 1, nch}, {all, 2, (nch + 1) / 2}, {all, 0, 1}, {heaviest, 0, 0}, {heaviest, 2, 0}, {0, 0, nch}, {0, 3, nch}};
  std::vector<Task2> tasks;
  std::vector<long long> first;
  for (const Cut& cut : cuts) {
    const std::vector<size_t> cs = chain_cut(ch.weight, cut.room, cut.cap);
    CHECK(cs.size() >= 2 && cs.front() == 0 && cs.back() == nch);
    if (cut.batches) CHECK(cs.size() - 1 == cut.batches);
    for (size_t cb = 0; cb + 1 < cs.size(); ++cb) {
      const size_t c0 = cs[cb], nc = cs[cb + 1] - c0;
      CHECK(cs[cb] < cs[cb + 1]);  // every chain in exactly one batch
      if (cut.cap) CHECK((long long)nc <= cut.cap);
      const long long sum = std::accumulate(ch.weight.begin() + c0, ch.weight.begin() + c0 + nc, 0ll);
      if (sum > cut.room) CHECK(nc == 1);
      if (cs[cb + 1] < nch) CHECK(sum + ch.weight[cs[cb + 1]] > cut.room || (cut.cap && (long long)nc == cut.cap));
      chain_lists(z, s0, ch, c0, nc, codes.data(), supp, tasks, first);
      CHECK(first.size() == 4 * N + 1 && first.front() == 0 && first.back() == (long long)tasks.size());
      std::vector<long long> per_chain(nc, 0);
      for (int li = 0; li < 4 * N; ++li) {
        const int k = li / 4, kind = CHAIN_KINDS[li % 4];
        std::vector<long long> want(nc);
        for (size_t e = 0; e < nc; ++e) {
          const int m = ch.cstr[c0 + e];
          want[e] = expected_chain_tasks(kind, k, &PAD[(s0 + ch.cent[c0 + e]) * N1], &codes[m * N], SUPP[m][0], SUPP[m][1]);
          per_chain[e] += want[e];
        }
        CHECK(first[li] <= first[li + 1]);
        check_launch(tasks, first[li], first[li + 1], want);
      }
      for (size_t e = 0; e < nc; ++e) CHECK(per_chain[e] == ch.ntasks[c0 + e]);
    }
  }
  CHECK(CHAIN_KINDS[0] == STR_T && CHAIN_KINDS[1] == STR_PAULI && CHAIN_KINDS[2] == STR_X && CHAIN_KINDS[3] == STR_CLOSE);
  {  // only all-identity strings: no chain, one empty chain batch
    const std::vector<uint8_t> none(2 * N, 0);
    std::vector<int32_t> s2;
    CHECK(string_supports(none.data(), 2, N, s2) == -1);
    const Chains empty = list_chains(z, 0, NS, 2, none.data(), s2);
    CHECK(empty.cent.empty() && (chain_cut(empty.weight, all, 1) == std::vector<size_t>{0, 0}));
  }
  std::printf("ok  chains\n");
}

void test_kinds() {  // one integer space: no two kinds share a value, GEMM kinds are the ones >= 0
  const int gemm[] = {LOC_REV_T, LOC_REV_X, LOC_FWD_T, LOC_FWD_W, LOC_PAIR_T, LOC_PAIR_V, LOC_DIST_T, LOC_DIST_X, LOC_BOND_M, STR_T, STR_X};
  const int other[] = {LOC_RHO, LOC_PAIR_RHO, LOC_DIST_RHO, LOC_ADMIT, LOC_BOND_TR, STR_LNEXT, STR_PAULI, STR_CLOSE};
  std::map<int, int> seen;
  for (const int k : gemm) CHECK(k >= 0 && ++seen[k] == 1);
  for (const int k : other) CHECK(k < 0 && ++seen[k] == 1);
  for (const int k : gemm) CHECK(conj_b(k) == (k == LOC_REV_X || k == LOC_FWD_W || k == LOC_PAIR_V || k == LOC_DIST_X || k == STR_X));
  std::printf("ok  kinds\n");
}

}  // namespace

int main() {
  test_kinds();
  test_layout();
  test_pair_index();
  test_batch_cut();
  // reverse 2 (n - 1) = 12 launches; forward per site T, W, rho = 21; pair: T', V, pair rho at k = 0 .. 5 = 18;
  // D = 3: T'', X'', distant rho at k = 1 .. 5 = 15 and the admit at k = 0 .. 4 = 5
  test_tables("one-qubit sweep", sizes(false, 1, false), local_plan(N, false, 1), 33);
  test_tables("pair sweep, D = 1", sizes(true, 1, false), local_plan(N, true, 1), 51);
  test_tables("pair sweep, D = 3", sizes(true, 3, false), local_plan(N, true, 3), 71);
  test_tables("environment pass", sizes(false, 1, true), env_plan(N), 33);
  Plan purities = env_plan(N);
  const Plan tail = bond_tail(N);
  purities.insert(purities.end(), tail.begin(), tail.end());
  test_tables("environment pass and bond tail", sizes(false, 1, true), purities, 33 + 12);
  test_chains();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
