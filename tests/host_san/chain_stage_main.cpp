// The device buffer of a chain batch (csrc/qk_local_plan.h: chain_offsets, chain_stage, chain_stage_max) for the five chain
// families -- Pauli strings (and operator strings, whose partial sums are twice as wide), block pair chains, shot chains, amplitude
// chains, window chains -- on the three hand-made 7-site states of local_plan_main.cpp, and the batch cap of the environment
// (batch_cap).  Every expected offset is restated here from the layout
//     [the family's columns | slot bases (int64) | tasks (8 bytes each) | partial sums | slots], all but the slots rounded up to 256,
// not taken from the header.  Built with g++ -fsanitize=address,undefined and run by tests/test_chain_stage_plan.py; prints one line
// per section, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_local_plan.h"

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

using namespace qkl;

namespace {
std::string last_error;
}
int qk_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error = buf;
  return code;
}

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) ++failures, std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr int NS = 3, N = 7;
const int32_t TRU[NS * (N + 1)] = {
    1, 2, 4,  8,  4,   2,  1, 1,   // pads to 16 everywhere
    1, 2, 17, 80, 150, 33, 2, 1,   // pads to 16, 16, 32, 80, 160, 48, 16, 16
    1, 2, 4,  65, 64,  4,  2, 1,   // pads to 16, 16, 16, 80, 64, 16, 16, 16
};
const long long PMAX[NS] = {16, 160, 80};
constexpr int MAX_PAD = 160, MAX_CHUNKS = MAX_PAD / 16;

size_t a256(const size_t b) { return (b + 255) / 256 * 256; }

struct Region {
  size_t at, len;
};
// every region inside [0, total), no two overlapping
void check_regions(std::vector<Region> r, const size_t total) {
  std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.at < b.at; });
  for (size_t i = 0; i < r.size(); ++i) {
    CHECK(r[i].len > 0 && r[i].at + r[i].len <= total);
    if (i) CHECK(r[i - 1].at + r[i - 1].len <= r[i].at);
  }
}

struct Family {
  const char* name;
  std::vector<ChainCol> cols;
  std::vector<size_t> bytes;  // restated: bytes per chain of every column of the family
  const ChainCore* core;
  std::vector<long long> slot;  // restated: doubles of every chain's slot
  long long width;              // doubles of a chain's partial sums
  std::function<void(size_t, size_t, std::vector<Task2>&, std::vector<long long>&)> lists;
};

// the restated total of the chains [c0, c1)
size_t expected_total(const Family& f, const size_t c0, const size_t c1) {
  const size_t nc = c1 - c0;
  size_t at = 0;
  for (const size_t b : f.bytes) at += a256(nc * b);
  long long nt = 0, sl = 0;
  for (size_t e = c0; e < c1; ++e) nt += f.core->ntasks[e], sl += f.slot[e];
  return at + a256(nc * 8) + a256((size_t)nt * 8) + a256(nc * (size_t)f.width * 8) + (size_t)sl * 8;
}

void check_range(const Family& f, const size_t c0, const size_t c1, ChainStage& st) {
  const ChainCore& c = *f.core;
  const size_t nc = c1 - c0, ncols = f.cols.size();
  std::vector<Task2> tasks;
  std::vector<long long> first;
  f.lists(c0, nc, tasks, first);
  long long nt = 0, sl = 0, wsum = 0;
  for (size_t e = c0; e < c1; ++e) nt += c.ntasks[e], sl += f.slot[e], wsum += c.weight[e];
  CHECK((long long)tasks.size() == nt && first.back() == nt);
  chain_stage(f.cols, c, c0, c1, f.width, tasks, st);
  // offsets against the restated sums
  CHECK(st.col.size() == ncols + 1);
  size_t at = 0;
  std::vector<Region> regions;
  std::vector<char> covered(st.image.size(), 0);
  for (size_t k = 0; k < ncols; ++k) {
    CHECK(st.col[k] == at);
    const size_t len = nc * f.bytes[k];
    CHECK(f.cols[k].elem * f.cols[k].per == f.bytes[k]);
    regions.push_back({at, len});
    for (size_t b = 0; b < len && at + b < st.image.size(); ++b) {
      covered[at + b] = 1;
      const char want = f.cols[k].src ? static_cast<const char*>(f.cols[k].src)[c0 * f.bytes[k] + b] : 0;  // a column without a source is zeros
      if (st.image[at + b] != want) {
        CHECK(!"a column's bytes in the image differ from the source's");
        break;
      }
    }
    at += a256(len);
  }
  CHECK(st.col[ncols] == at);
  regions.push_back({at, nc * 8});
  CHECK(st.cbase.size() == nc);
  long long run = 0;
  for (size_t e = 0; e < nc; ++e) {  // slot bases: the running sum of the slots of this range alone
    CHECK(st.cbase[e] == run);
    int64_t in_image = -1;
    std::memcpy(&in_image, st.image.data() + at + 8 * e, 8);
    CHECK(in_image == run);
    run += f.slot[c0 + e];
    for (size_t b = 0; b < 8; ++b) covered[at + 8 * e + b] = 1;
  }
  at += a256(nc * 8);
  CHECK(st.tasks == at);
  regions.push_back({at, (size_t)nt * 8});
  CHECK(std::memcmp(st.image.data() + at, tasks.data(), (size_t)nt * 8) == 0);
  for (size_t b = 0; b < (size_t)nt * 8; ++b) covered[at + b] = 1;
  at += a256((size_t)nt * 8);
  CHECK(st.part == at && st.image.size() == at);  // the table part is what is uploaded
  if (f.width) regions.push_back({at, nc * (size_t)f.width * 8});
  at += a256(nc * (size_t)f.width * 8);
  CHECK(st.slots == at);
  regions.push_back({at, (size_t)sl * 8});
  CHECK(st.total == at + (size_t)sl * 8 && st.total == expected_total(f, c0, c1));
  CHECK((size_t)(st.cbase[nc - 1] + f.slot[c1 - 1]) * 8 == st.total - st.slots);  // the last slot ends where the region does
  for (size_t b = 0; b < st.image.size(); ++b)
    if (!covered[b] && st.image[b] != 0) {
      CHECK(!"a pad byte of the image is not zero");
      break;
    }
  check_regions(regions, st.total);
  // the budget: a batch chain_cut admitted outgrows 8 bytes per unit of weight by the rounding alone
  CHECK(st.total <= 8 * (size_t)wsum + 256 * (ncols + 1 + 2));
  // the offsets alone give the same
  ChainStage only;
  CHECK(chain_offsets(f.cols, c, c0, c1, f.width, only) == st.total && only.col == st.col && only.tasks == st.tasks && only.part == st.part && only.slots == st.slots);
}

void check_family(const Family& f) {
  const ChainCore& c = *f.core;
  const size_t n = c.weight.size();
  CHECK(n >= 6 && c.slot.size() == n && c.ntasks.size() == n && f.slot.size() == n);
  for (size_t e = 0; e < n; ++e) CHECK(c.slot[e] == f.slot[e]);
  ChainStage st;  // one stage for every range, as the drivers keep it: nothing of a larger batch may survive in a smaller one
  check_range(f, 0, n, st);
  check_range(f, 2, n - 1, st);
  check_range(f, n - 1, n, st);
  const long long all = std::accumulate(c.weight.begin(), c.weight.end(), 0ll);
  const long long rooms[] = {LLONG_MAX / 4, all / 2};
  for (const long long room : rooms)
    for (const long long cap : {1ll, 3ll, 0ll}) {
      const std::vector<size_t> cs = chain_cut(c.weight, room, cap);
      size_t most = 0;
      for (size_t cb = 0; cb + 1 < cs.size(); ++cb) most = std::max(most, expected_total(f, cs[cb], cs[cb + 1]));
      CHECK(chain_stage_max(f.cols, c, cs, f.width) == most);
      if (cap == 1) CHECK(cs.size() == n + 1);
      if (cap == 0 && room > all) CHECK(cs.size() == 2 && most == expected_total(f, 0, n));
    }
  CHECK(chain_stage_max(f.cols, c, {0, 0}, f.width) == 0);  // no chain: one empty batch, nothing behind the state batch
  std::printf("ok  %s (%zu chains)\n", f.name, n);
}

void test_batch_cap() {
  const char* var = "QK_CHAIN_STAGE_TEST_BATCH";
  long long cap = -1;
  unsetenv(var);
  CHECK(batch_cap("f", var, cap) == QK_OK && cap == 0);  // unset: the memory rule alone
  setenv(var, "5", 1);
  CHECK(batch_cap("f", var, cap) == QK_OK && cap == 5);
  setenv(var, "1", 1);
  CHECK(batch_cap("f", var, cap) == QK_OK && cap == 1);
  for (const char* bad : {"0", "-3", "x"}) {
    setenv(var, bad, 1);
    last_error.clear();
    CHECK(batch_cap("qk_some_host", var, cap) == QK_EINVAL);
    CHECK(last_error == std::string("qk_some_host: QK_CHAIN_STAGE_TEST_BATCH must be >= 1 (got \"") + bad + "\")");
  }
  unsetenv(var);
  std::printf("ok  batch cap\n");
}

}  // namespace

int main() {
  EnvSizes z;
  env_sizes(TRU, NS, N, MAX_PAD, LOC_RMUL, true, z);
  CHECK(z.max_chunks == MAX_CHUNKS);

  // Pauli strings, and operator strings on the same chains: a chunk sum is (Re, Im), the weight grows by max_chunks
  const char* const STRINGS[6] = {"IIIIIII", "XIIIIII", "IIIIIIZ", "IXYZIII", "ZIIIIIX", "IIIXZII"};
  std::vector<uint8_t> codes(6 * N);
  for (int m = 0; m < 6; ++m)
    for (int k = 0; k < N; ++k) codes[m * N + k] = (uint8_t)(STRINGS[m][k] == 'X' ? 1 : STRINGS[m][k] == 'Y' ? 2 : STRINGS[m][k] == 'Z' ? 3 : 0);
  std::vector<int32_t> supp;
  CHECK(string_supports(codes.data(), 6, N, supp) == -1);
  Chains str = list_chains(z, 0, NS, 6, codes.data(), supp);  // 15 chains: the all-identity string has none
  std::vector<long long> str_slot;
  for (size_t e = 0; e < str.cent.size(); ++e) str_slot.push_back(6 * PMAX[str.cent[e]] * PMAX[str.cent[e]]);
  auto str_lists = [&](size_t c0, size_t nc, std::vector<Task2>& t, std::vector<long long>& f) { chain_lists(z, 0, str, c0, nc, codes.data(), supp, t, f); };
  check_family({"strings", {{str.cent.data(), 4, 1}, {str.cstr.data(), 4, 1}}, {4, 4}, &str, str_slot, MAX_CHUNKS, str_lists});
  for (long long& w : str.weight) w += MAX_CHUNKS;
  check_family({"operator strings", {{str.cent.data(), 4, 1}, {str.cstr.data(), 4, 1}}, {4, 4}, &str, str_slot, 2 * MAX_CHUNKS, str_lists});

  // block: every pair of the three states, widths 2 and 5 from the left
  const int32_t widths[2] = {2, 5};
  std::vector<int32_t> pairs, cpm;
  std::vector<long long> blk_slot;
  for (int i = 0; i < NS; ++i)
    for (int j = 0; j < NS; ++j) {
      pairs.push_back(i), pairs.push_back(j);
      cpm.push_back((int32_t)std::max(PMAX[i], PMAX[j]));
      blk_slot.push_back(6ll * cpm.back() * cpm.back());
    }
  const std::vector<BlkLaunch> bplan = blk_plan(2, widths);
  const BlkChains blk = list_blk_chains(z, z, NS * NS, pairs.data(), 0, bplan, 2);
  check_family({"block", {{pairs.data(), 4, 2}, {cpm.data(), 4, 1}}, {8, 4}, &blk, blk_slot, 2 * MAX_CHUNKS,
                [&](size_t c0, size_t nc, std::vector<Task2>& t, std::vector<long long>& f) { blk_lists(z, z, pairs.data(), c0, nc, 0, bplan, t, f); }});

  // sample and amplitude: 150 rows per state in tiles of 64 (64, 64, 22 -> 32 padded rows)
  const SmpChains smp = list_smp_chains(z, 0, NS, 150, 64), amp = list_amp_chains(z, 0, NS, 150, 64);
  std::vector<long long> smp_slot, amp_slot;
  for (size_t e = 0; e < smp.cent.size(); ++e) {
    const long long R = (smp.rows[e] + 15) / 16 * 16;
    smp_slot.push_back(14 * PMAX[smp.cent[e]] * R), amp_slot.push_back(6 * PMAX[amp.cent[e]] * R);
  }
  check_family({"sample", {{smp.cent.data(), 4, 1}, {smp.shot0.data(), 4, 1}, {smp.rows.data(), 4, 1}, {nullptr, 4, 1}}, {4, 4, 4, 4}, &smp, smp_slot, 0,
                [&](size_t c0, size_t nc, std::vector<Task2>& t, std::vector<long long>& f) { smp_lists(z, 0, smp, c0, nc, t, f); }});
  check_family({"amplitude", {{amp.cent.data(), 4, 1}, {amp.shot0.data(), 4, 1}, {amp.rows.data(), 4, 1}}, {4, 4, 4}, &amp, amp_slot, 0,
                [&](size_t c0, size_t nc, std::vector<Task2>& t, std::vector<long long>& f) { amp_lists(z, 0, amp, c0, nc, t, f); }});

  // window: width 3, every start; the closing sums of a chain are 2 * 36 doubles per chunk
  const int32_t starts[5] = {0, 1, 2, 3, 4};
  const WinChains win = list_win_chains(z, 0, NS, 3, 5, starts);
  std::vector<long long> win_slot;
  for (size_t e = 0; e < win.cent.size(); ++e) win_slot.push_back(8 * PMAX[win.cent[e]] * PMAX[win.cent[e]] * 8);
  check_family({"window", {{win.cent.data(), 4, 1}, {win.cwin.data(), 4, 1}}, {4, 4}, &win, win_slot, MAX_CHUNKS * 72,
                [&](size_t c0, size_t nc, std::vector<Task2>& t, std::vector<long long>& f) { win_lists(z, 0, win, c0, nc, 3, starts, t, f); }});

  test_batch_cap();
  if (failures) std::printf("FAIL %d checks\n", failures);
  return failures ? 1 : 0;
}
