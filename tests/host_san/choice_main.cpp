// The sweep's choice of launches (qk_choose_sweep, csrc/qk_plan.h) on hand-made plans, 256 CUs: per case the kernel, grid, dynamic LDS
// and pairs of each launch, the grid qk_stats reports and the scratch bytes.  The expected values are what qk_gram_values launched before
// the choice was a function of its own.  Built with g++ and run by tests/test_sweep_choice.py; prints one line per case, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_plan.h"

#include <cstring>
#include <vector>

namespace {

struct In {  // one call: the context's switches, the plan, the two sets (one shape for both)
  QkSweepPolicy pol;
  qk_plan plan;
  QkSetShape set{128, 64, 60};
  In(long long np = 125250) {
    plan.pairs.assign(2 * np, 0);
    plan.n_first = np, plan.nq = 16;
  }
  template <typename T>
  In& sw(T QkSweepPolicy::*field, T v) { return pol.*field = v, *this; }
  In& pad(int p) { return set.max_pad = p, *this; }
  In& fp32() { return set.precision = 32, *this; }
  In& sites(int n) { return set.n_sites = n, *this; }
  In& fit(double two, double narrow) { return plan.fit_two = two, plan.fit_narrow = narrow, *this; }
  In& first(long long n, bool wave2 = false) { return plan.n_first = n, plan.second_wave2 = wave2, *this; }
  In& quad() { return plan.quad = true, *this; }
};

struct Run {
  int kernel;
  long long grid;
  size_t lds;
  long long first, count;
};

struct Case {
  const char* name;
  In in;
  std::vector<Run> runs;  // empty: the call fails with `err`
  long long launched_grid;
  size_t scratch;
  const char* err;
};

#define P(f) &QkSweepPolicy::f  // a switch: P(wave2_path) false = QK_WAVE2=0, P(wave2_ring) false = QK_WAVE2=2, P(fused_dual) false = QK_FUSED_DUAL=0

const Case cases[] = {
  // clang-format off
  {"bonds <= 16",                     In().pad(16),                                      {{QK_KERNEL_WAVE, 4096, 0, 0, 125250}},           4096, 6291456, nullptr},
  {"bonds <= 32",                     In().pad(32),                                      {{QK_KERNEL_WAVE2, 2048, 0, 0, 125250}},          2048, 25165824, nullptr},
  {"bonds <= 32, QK_WAVE2=0",         In().pad(32).sw(P(wave2_path), false),             {{QK_KERNEL_SMALL, 512, 75688, 0, 125250}},       512, 25165824, nullptr},
  {"bonds <= 32, QK_WAVE2=2",         In().pad(32).sw(P(wave2_ring), false),             {{QK_KERNEL_WAVE2_PLAIN, 2048, 0, 0, 125250}},    2048, 25165824, nullptr},
  {"bonds <= 32, QK_FUSED=2",         In().pad(32).sw(P(fused_path), 2),                 {{QK_KERNEL_FUSED2, 512, 77840, 0, 125250}},      512, 25165824, nullptr},
  {"fp32, bonds <= 32",               In().pad(32).fp32(),                               {{QK_KERNEL_WAVE2, 2048, 0, 0, 125250}},          2048, 25165824, nullptr},
  {"fp32, bonds 128",                 In().fp32(),                                       {{QK_KERNEL_RING, 512, 51112, 0, 125250}},        512, 402653184, nullptr},
  {"12-wave dual shape",              In().fit(0.5, 1),                                  {{QK_KERNEL_FUSED_DUAL, 256, 135184, 0, 125250}}, 256, 201326592, nullptr},
  {"... QK_FUSED_DUAL=0",             In().fit(0.5, 1).sw(P(fused_dual), false),         {{QK_KERNEL_FUSED1, 256, 135184, 0, 125250}},     256, 201326592, nullptr},
  {"... QK_FUSED_WGS=2",              In().fit(0.5, 1).sw(P(fused_wgs), 2),              {{QK_KERNEL_FUSED2, 512, 77840, 0, 125250}},      512, 402653184, nullptr},
  {"two-wg plan, QK_FUSED_WGS=1",     In().sw(P(fused_wgs), 1),                          {{QK_KERNEL_FUSED_DUAL, 256, 135184, 0, 125250}}, 256, 201326592, nullptr},
  {"two-wg shape by fit_two/narrow",  In().fit(0.8, 0.6),                                {{QK_KERNEL_FUSED2, 512, 77840, 0, 125250}},      512, 402653184, nullptr},
  {"dual shape: fit_narrow < 0.5",    In().fit(0.8, 0.4),                                {{QK_KERNEL_FUSED_DUAL, 256, 135184, 0, 125250}}, 256, 201326592, nullptr},
  {"split, >= 100 pairs per CU",      In().pad(256).fit(0.5, 1).first(60000),
                                      {{QK_KERNEL_FUSED_DUAL, 256, 135184, 0, 60000}, {QK_KERNEL_FUSED2, 512, 77840, 60000, 65250}},    256, 1610612736, nullptr},
  {"split, < 100 pairs per CU",       In(20000).pad(256).fit(0.5, 1).first(9000),       {{QK_KERNEL_FUSED_DUAL, 256, 135184, 0, 20000}},  256, 805306368, nullptr},
  {"... QK_FUSED_SPLIT=2",            In(20000).pad(256).fit(0.5, 1).first(9000).sw(P(fused_split), 2),
                                      {{QK_KERNEL_FUSED_DUAL, 256, 135184, 0, 9000}, {QK_KERNEL_FUSED2, 512, 77840, 9000, 11000}},      256, 1610612736, nullptr},
  {"mixed",                           In().fit(0.5, 1).first(100000, true),
                                      {{QK_KERNEL_FUSED_DUAL, 256, 135184, 0, 100000}, {QK_KERNEL_WAVE2, 2048, 0, 100000, 25250}},      256, 201326592, nullptr},
  {"DET, dual shape",                 In().fit(0.5, 1).sw(P(deterministic), true),       {{QK_KERNEL_FUSED_DUAL_DET, 256, 135704, 0, 125250}}, 256, 201326592, nullptr},
  {"DET, single tiles",               In().fit(0.5, 1).sw(P(deterministic), true).sw(P(fused_dual), false),
                                      {{QK_KERNEL_FUSED1_DET, 256, 135704, 0, 125250}},                                                 256, 201326592, nullptr},
  {"DET, two-wg shape",               In().sw(P(deterministic), true),                   {{QK_KERNEL_FUSED2_DET, 512, 78360, 0, 125250}},  512, 402653184, nullptr},
  {"DET, split",                      In().pad(256).fit(0.5, 1).first(60000).sw(P(deterministic), true),
                                      {{QK_KERNEL_FUSED_DUAL_DET, 256, 137240, 0, 60000}, {QK_KERNEL_FUSED2_DET, 512, 79896, 60000, 65250}}, 256, 1610612736, nullptr},
  {"QK_FUSED=0",                      In().sw(P(fused_path), 0),                         {{QK_KERNEL_RING, 512, 51112, 0, 125250}},        512, 402653184, nullptr},
  {"quad plan (product build)",       In(4000).quad(), {}, 0, 0,
                                      "qk_gram_values: QK_PLAN_QUADS plans are swept by an experimental kernel that only libqklab.so contains"},
  {"chain too long for the ring",     In().sites(1100), {}, 0, 0,
                                      "qk_gram_values: 1100 sites need 84392 bytes of LDS per workgroup (limit 80 KiB for 2 workgroups per CU)"},
  // clang-format on
};

}  // namespace

int main() {
  int bad = 0;
  for (const Case& c : cases) {
    const QkSweepChoice ch = qk_choose_sweep(c.in.pol, c.in.plan, c.in.set, c.in.set, 256);
    bool ok;
    if (c.err) {
      ok = ch.rc == QK_EINVAL && std::strcmp(ch.err, c.err) == 0;
    } else {
      ok = ch.rc == QK_OK && ch.n_runs == (int)c.runs.size() && ch.launched_grid == c.launched_grid && ch.scratch_bytes == c.scratch;
      for (int i = 0; ok && i < ch.n_runs; ++i) {
        const QkSweepRun& r = ch.run[i];
        const Run& w = c.runs[i];
        ok = r.kernel == w.kernel && r.grid == w.grid && r.lds == w.lds && r.first == w.first && r.count == w.count;
      }
    }
    std::printf("%s  %s: rc %d", ok ? "ok  " : "FAIL", c.name, ch.rc);
    for (int i = 0; ch.rc == QK_OK && i < ch.n_runs; ++i)
      std::printf("  [kernel %d grid %lld lds %zu pairs %lld+%lld]", ch.run[i].kernel, ch.run[i].grid, ch.run[i].lds, ch.run[i].first, ch.run[i].count);
    std::printf("  grid %lld scratch %zu %s\n", ch.launched_grid, ch.scratch_bytes, ch.err);
    bad += !ok;
  }
  return bad ? 1 : 0;
}
