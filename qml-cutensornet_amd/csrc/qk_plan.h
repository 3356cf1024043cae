// qk_plan.h -- the host-side plan of a Gram share (struct qk_plan), the constants the planner shares with the launches, the pure
// functions host and device share (the order of a step's units, the units of an edge product, the segmentation of a chain into plain and
// merged steps), and the choice of the sweep's launches for a plan (qk_choose_sweep).
// Plain C++: no HIP type appears here, so the planner (qk_planner.cpp) also builds as a host-only translation unit
// (tests/host_san: -fsanitize=address,undefined), and the choice is tested on the CPU (tests/host_san/choice_main.cpp).
#pragma once
#include "../../include/qkgram.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

int qk_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));  // sets qk_last_error(), returns code

#ifndef QKF_XCAP_ONE_V
#define QKF_XCAP_ONE_V 8192
#endif
#ifndef QKF_XCAP_TWO_V
#define QKF_XCAP_TWO_V 4608
#endif
#ifndef QKF_TWO_WGS
#define QKF_TWO_WGS 2  // workgroups per CU of the small-site shape (experiment builds: 3 with a 3072-element buffer)
#endif
static constexpr int QKF_XCAP_ONE = QKF_XCAP_ONE_V, QKF_XCAP_TWO = QKF_XCAP_TWO_V;  // elements of the fused sweep's LDS X buffer with one / two workgroups per CU
static constexpr int QK_TILE = 16;                                        // M/N granule of v_mfma_f64_16x16x4_f64
// The residency of X (qk_resident below), two parts behind compile-time switches for A/B builds, both on by default:
//   QKF_RES_PARTIAL  a step whose X and X' each fit the buffer but not together evicts only the panels of X that X' overlaps (0: all of X);
//   QKF_RES_BIG      the 12-wave shapes offer X and X' the LDS the CU has beyond the segmentation's buffer (0: QKF_XCAP_ONE).
#ifndef QKF_RES_PARTIAL
#define QKF_RES_PARTIAL 1
#endif
#ifndef QKF_RES_BIG
#define QKF_RES_BIG 1
#endif
// The large buffer of the 12-wave shapes, from the kernels' static LDS layout: the X buffer first, behind it the queue slot, the overlap's
// partial sums, the step table and (DET) the turn counters -- QKF_META_ROOM bytes are left for those, and a launch whose chain needs more
// runs the instantiation with QKF_XCAP_ONE elements (qk_choose_sweep below: QkSweepRun.big).  The segmentation, the class split, the strip width and the
// switch test keep QKF_XCAP_ONE: only qk_resident sees the larger number.
static constexpr int QKF_LDS_BYTES = 160 * 1024, QKF_META_ROOM = 8 * 1024;
static constexpr int QKF_RCAP_ONE = QKF_RES_BIG ? (QKF_LDS_BYTES - QKF_META_ROOM) / 16 / (QK_TILE * QK_TILE) * (QK_TILE * QK_TILE) : QKF_XCAP_ONE;
static_assert(QKF_RCAP_ONE >= QKF_XCAP_ONE && (long long)QKF_RCAP_ONE * 16 + QKF_META_ROOM <= QKF_LDS_BYTES && QKF_RCAP_ONE % (QK_TILE * QK_TILE) == 0,
              "the large X buffer and the room behind it fit the LDS of a CU; the buffer holds whole 16 x 16 blocks");
static inline int qk_pad16(int x) { return (x + QK_TILE - 1) / QK_TILE * QK_TILE; }
static constexpr int GMAX = 4;  // pairs per group of the group-sweep lab kernel (sizes its X/T scratch)

// ----------------------------------------------------------------------------------------
// The order of a step's units in the site-fused sweep (qk_fused.h).  A step has pd * mt * wc units (ta, tc, p): ta = block of 16 rows of
// A_k (mt of them), p = physical index (pd = 2, or 4 for a merged step), tc = column unit of the strip of X' at hand -- a PAIR of column
// blocks (2 tc, 2 tc + 1) in the dual kernel, wc = ceil(w / 2), one column block in the one-tile kernel, wc = w (qk_unit_cols).  The units
// are dealt to the NW waves of a workgroup in rounds of NW consecutive indices v, so the order decides which operands the waves of a round
// share: unit (ta, tc, p) reads the A block (ta, p) and the B blocks (p, its column blocks).
//   qk_unit_decode:          v = (p * wc + tc) * mt + ta -- p slowest, ta fastest.  A round then lies inside one p (two at a seam) and covers
//                            a few tc with all their ta: the waves that run together share BOTH operands (an A block between the tc of the
//                            round, a B block between its ta).  The plain (arrival-order) form of the one-tile kernel uses it.
//   qk_unit_decode_ordered:  v = pd * (tc * mt + ta) + p -- p fastest, tc slowest: every round takes one or two tc with all their (ta, p), so
//                            an A block is wanted again a whole round later, once per tc.  The ordered (DET) kernels keep it: their turn
//                            index pd * ta + p must rise along v inside a block of rows (qkf_turn_add).  So does the dual kernel in its
//                            plain form: it measured 2 % slower with p slowest (lab/NOTES_r05.md).
// Both are pure functions of the index, host and device, and are checked on the CPU (tests/host_san/units_main.cpp: every unit exactly once,
// the reciprocals against the divisions, and the count of operand blocks per round of the two orders).
// The divisions are multiplications by reciprocals from the step record: inv_mt = ceil(2^20 / mt) (v / mt for v < 4096, mt <= 32) and
// inv_wc = ceil(2^15 / wc) (c / wc for c < 128, wc <= 32): a step has up to two strip widths (W and a shorter last strip), so two 16-bit
// reciprocals share one word of the record (qk_unit_recips).
// ----------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#define QK_HD __host__ __device__
#else
#define QK_HD
#endif
struct QkUnit {
  int ta, tc, p;
};
QK_HD static inline int qk_unit_cols(const int w, const bool dual) { return dual ? (w + 1) >> 1 : w; }
QK_HD static inline int qk_recip20(const int d) { return ((1 << 20) + d - 1) / d; }  // n / d == (n * qk_recip20(d)) >> 20 for n < 4096, d <= 32
QK_HD static inline int qk_recip15(const int d) { return ((1 << 15) + d - 1) / d; }  // n / d == (n * qk_recip15(d)) >> 15 for n < 128, d <= 32
// the record's word [11] of a step with nt column blocks in strips of W: the reciprocal of the column units of a full strip in the low half,
// of the last strip (nt - W * floor((nt - 1) / W) blocks; the same when W divides nt) in the high half
QK_HD static inline int qk_unit_recips(const int nt, const int W, const bool dual) {
  const int wl = nt - (nt - 1) / W * W;
  return qk_recip15(qk_unit_cols(W, dual)) | (qk_recip15(qk_unit_cols(wl, dual)) << 16);
}
QK_HD static inline int qk_unit_recip_of(const int recips, const bool full_strip) { return full_strip ? (recips & 0xffff) : (int)((unsigned)recips >> 16); }
QK_HD static inline QkUnit qk_unit_decode(const int v, const int mt, const int wc, const int inv_mt, const int inv_wc) {
  const int c = (v * inv_mt) >> 20, p = (c * inv_wc) >> 15;
  return QkUnit{v - c * mt, c - p * wc, p};
}
QK_HD static inline QkUnit qk_unit_decode_ordered(const int v, const int ps, const int mt, const int inv_mt) {
  const int u = v >> ps, tc = (u * inv_mt) >> 20;
  return QkUnit{u - tc * mt, tc, v & ((1 << ps) - 1)};
}

// ----------------------------------------------------------------------------------------
// The units of an EDGE product (qk_fused.h: qkf_edge_prefix / qkf_edge_suffix).  The product has mt x nt tiles (ta = block of 16 columns of
// the x block, tb = block of 16 columns of the y block).  A unit is (ta, tb0, has1): the tile (ta, tb0) and, with has1, its neighbour
// (ta, tb0 + 1) -- one fragment of the x block feeds both.  Pair v = tp * mt + ta (ta fastest) covers the column blocks 2 tp, 2 tp + 1; the
// last pair of an odd nt is a single tile.  Units are dealt to the NW waves in rounds of NW consecutive indices u.  When the pairs left for
// the last round fill at most half of the waves, that round is dealt as single tiles (the rule of the dual kernel's rounds): index
// r0 + w is the first tile of pair r0 + w, index r0 + left + w its second one, so the round takes half as long.
//   qk_edge_units: how many indices u a product has (indices without a tile -- `mine` false -- occur only in a round of singles);
//   qk_edge_unit:  index u -> unit.  inv_mt = qk_recip20(mt).
// Pure functions, host and device; checked on the CPU for every mt, nt <= 16 (tests/host_san/edge_units_main.cpp).  The shipped kernels take
// single tiles (they measured faster than pairs at the same matrix work in flight: lab/NOTES_r06.md); the pairs run in builds with
// -DQKF_EDGE_PAIRS_V=1.
// ----------------------------------------------------------------------------------------
struct QkEdgeUnit {
  int ta, tb0;
  bool has1, mine;
};
QK_HD static inline int qk_edge_units(const int mt, const int nt, const int NW) {
  const int pairs = mt * ((nt + 1) >> 1), r0 = (pairs - 1) / NW * NW, left = pairs - r0;
  return 2 * left <= NW ? r0 + 2 * left : pairs;
}
QK_HD static inline QkEdgeUnit qk_edge_unit(const int u, const int mt, const int nt, const int NW, const int inv_mt) {
  const int pairs = mt * ((nt + 1) >> 1), r0 = (pairs - 1) / NW * NW, left = pairs - r0;
  const bool halves = 2 * left <= NW, single = halves && u >= r0, half = halves && u >= r0 + left;
  const int v = u - (half ? left : 0), tp = (v * inv_mt) >> 20;
  const bool second = 2 * tp + 1 < nt;
  return QkEdgeUnit{v - tp * mt, 2 * tp + (half ? 1 : 0), !single && second, u < (halves ? r0 + 2 * left : pairs) && (!half || second)};
}

// ----------------------------------------------------------------------------------------
// The segmentation of a pair's chain into steps of the site-fused sweep (qk_fused.h: qkf_step_table).  The chain's sites [ek, n - ek) are
// walked one at a time (pd = 2) or two at a time through the sets' merged images (pd = 4: sites e, e + 1 contracted over their true middle
// bond once per state, so the sweep neither pads that bond to 16 nor walks it).  A merge at site e is ADMISSIBLE (qk_merge_admissible) when
// it keeps an LDS-resident pair of sites in the LDS of the launch's shape (QkSegRule: the shape's X buffer and its test that one round
// holds all units of a step) and costs no more padded work than the two sites.  qk_segment_chain picks among the admissible merges:
//   greedy  every admissible merge at an allowed start, walking forward (with even starts only: the fixed pairs (ek + 2 t, ek + 2 t + 1));
//   else    the segmentation that minimises the matrix instructions the kernels execute for the steps (qk_step_instr: tiles of 16, K
//           trimmed to the true bond in steps of 4, 3M product) plus QK_STEP_PRICE per step, by dynamic programming from the right end and
//           a forward walk over the starts that are reached.  Ties go to fewer steps, then to the even start.
// The result is a mask of 128 bits: bit i set = the step that starts at site ek + i takes site ek + i + 1 with it (sites beyond bit 127 are
// walked singly).  Pure functions of the bond rows, host and device: the kernel that fills the launches' masks (qkgram.hip:
// qk_segment_kernel), the step table, tools/merge_potential.py and the CPU tests (tests/host_san/segment_main.cpp) all call these.
// ----------------------------------------------------------------------------------------
static constexpr int QK_STEP_PRICE = 375;  // matrix instructions' worth of the fixed cost of a step: two barriers, set-up, load latencies = 2.5 us of a 12-wave workgroup (tools/site_overhead.py); qk_planner.cpp: choose_edge_k
static constexpr int QK_SEG_BITS = 128;
struct QkSegRule {  // a launch's shape: elements of its LDS X buffer; one round holds pd mt ceil(nt / 2) <= cap pairs of tiles (dual) or pd mt nt <= cap tiles
  int xcap, cap;
  bool dual;
  int rcap = 0;          // elements the residency of X may use (qk_resident): the physical buffer, >= xcap; 0 = xcap.  The segmentation never reads it
  bool partial = false;  // ... and whether a step may keep PART of X in LDS (QKF_RES_PARTIAL)
};
struct QkSegMask {
  unsigned long long w[2];
};
QK_HD static inline bool qk_seg_bit(const unsigned long long w0, const unsigned long long w1, const int i) { return i < QK_SEG_BITS && (((i < 64 ? w0 : w1) >> (i & 63)) & 1ull) != 0; }
QK_HD static inline bool qk_seg_one_round(const QkSegRule& r, const int pmt, const int nt) { return pmt * (r.dual ? (nt + 1) / 2 : nt) <= r.cap; }
// LDS-resident step: X and X' fit the buffer and either ONE round holds all units (X' may then overwrite X) or X and X' fit side by side
QK_HD static inline bool qk_seg_small(const QkSegRule& r, const int a, const int a2, const int b, const int b2, const int pd) {
  return a * b <= r.xcap && a2 * b2 <= r.xcap && (qk_seg_one_round(r, pd * (a / QK_TILE), b2 / QK_TILE) || a * b + a2 * b2 <= r.xcap);
}
// THE RESIDENCY OF X IN A STEP: where X' is built and which panels of X (16 columns each, a / 16 of b * 16 elements: qk_fused.h) phase 1
// reads from LDS.  X sits at one END of the buffer of qk_res_cap elements -- at element 0, or at the top (x_top: its last element is the
// buffer's last) -- and X' is built at the other end whenever that lets panels of X live through the step:
//   QK_RES_SIDE     X and X' fit side by side: X' at the other end, every panel stays, nothing is copied;
//   QK_RES_INPLACE  LDS-resident by its single round alone (qk_seg_small, not side by side): every unit reads X from LDS in phase 1, then X'
//                   overwrites it from element 0 behind a barrier;
//   QK_RES_PART     X fits, X' fits, not together, more than one round: X' at the other end; the panels it overlaps go to the global buffer
//                   and their units read them there, the panels [klo, khi) at the far end stay -- a unit with row block ta reads only
//                   panel ta.  As many stay as fit (none when X' needs the whole buffer);
//   QK_RES_NONE     anything else -- X or X' does not fit the segmentation's buffer (strips), or partial residency is off: X goes to the
//                   global buffer whole, X' (or each strip of it) is built at element 0.
// "Fits" is the segmentation's xcap throughout, so the plan, the masks, the strip width and what may switch do not depend on rcap; only
// "together" and the place of X' see the larger buffer.  With rcap = xcap and partial off this is the classification the kernels had
// before the rule (tests/host_san/resident_main.cpp).  Pure, host and device; the step table carries it (qk_step_record, word [7]).
static constexpr int QK_RES_NONE = 0, QK_RES_SIDE = 1, QK_RES_PART = 2, QK_RES_INPLACE = 3;
struct QkResident {
  int kind, ob;  // QK_RES_*; the element of the buffer where X' (or a strip of it) is built
  int klo, khi;  // phase 1 reads the panels [klo, khi) of X from LDS, the others from the global buffer
};
QK_HD static inline int qk_res_cap(const QkSegRule& r) { return r.rcap > r.xcap ? r.rcap : r.xcap; }
// the same as one word for the kernels: bit ta set = the units of row block ta read their panel from the global buffer (a / 16 <= 32 panels)
QK_HD static inline unsigned qk_res_global_mask(const QkResident& s) { return ~(unsigned)(((1ull << s.khi) - 1ull) & ~((1ull << s.klo) - 1ull)); }
QK_HD static inline QkResident qk_resident(const QkSegRule& r, const int a, const int a2, const int b, const int b2, const int pd, const bool x_top) {
  const int rcap = qk_res_cap(r), n_in = a * b, n_out = a2 * b2, mt = a / QK_TILE, panel = b * QK_TILE;
  if (n_in > r.xcap || n_out > r.xcap) return QkResident{QK_RES_NONE, 0, 0, 0};
  const int ob = x_top ? 0 : rcap - n_out;  // the other end
  if (n_in + n_out <= rcap) return QkResident{QK_RES_SIDE, ob, 0, mt};
  if (qk_seg_small(r, a, a2, b, b2, pd)) return QkResident{QK_RES_INPLACE, 0, 0, mt};
  if (!r.partial) return QkResident{QK_RES_NONE, 0, 0, 0};
  if (x_top) {  // X = [rcap - n_in, rcap), X' = [0, n_out): the panels from the first one that starts at or above n_out stay
    const int over = n_out - (rcap - n_in), t0 = (over + panel - 1) / panel;  // (over > 0: they do not fit together)
    return QkResident{QK_RES_PART, ob, t0 < mt ? t0 : mt, mt};
  }
  const int t0 = ob / panel;  // X = [0, n_in), X' = [rcap - n_out, rcap): the panels that end at or below ob stay
  return QkResident{QK_RES_PART, ob, 0, t0 < mt ? t0 : mt};
}
// the rule in the step table's word [7]: the kind, and the boundary panel t0 of a partially resident step for X at the low end ([0, t0) stay)
// and for X at the top ([t0, mt) stay) -- the kind does not depend on the end
static constexpr int QK_REC_KIND_SHIFT = 3, QK_REC_T0_LOW_SHIFT = 8, QK_REC_T0_TOP_SHIFT = 16;
QK_HD static inline int qk_rec_resident_bits(const QkSegRule& r, const int a, const int a2, const int b, const int b2, const int pd) {
  const QkResident lo = qk_resident(r, a, a2, b, b2, pd, false), hi = qk_resident(r, a, a2, b, b2, pd, true);
  return (lo.kind << QK_REC_KIND_SHIFT) | (lo.khi << QK_REC_T0_LOW_SHIFT) | (hi.klo << QK_REC_T0_TOP_SHIFT);
}
QK_HD static inline QkResident qk_rec_resident(const int word, const int mt, const int n_out, const int rcap, const bool x_top) {
  const int kind = (word >> QK_REC_KIND_SHIFT) & 3, t0 = (word >> (x_top ? QK_REC_T0_TOP_SHIFT : QK_REC_T0_LOW_SHIFT)) & 63;
  const bool other_end = kind == QK_RES_SIDE || kind == QK_RES_PART;
  if (kind == QK_RES_NONE) return QkResident{QK_RES_NONE, 0, 0, 0};
  return QkResident{kind, other_end && !x_top ? rcap - n_out : 0, x_top ? t0 : 0, x_top ? mt : t0};
}
// matrix instructions of a step [a][pd][a2] x [b][pd][b2] (padded bonds) with true bonds at, bt on its left: phase 1 pd mt nt tiles of
// ceil(bt / 4) k-steps, phase 2 pd nt nn tiles of ceil(at / 4) k-steps over the blocks of rows, three real products each
QK_HD static inline long long qk_step_instr(const int pd, const int a, const int a2, const int b, const int b2, const int at, const int bt) {
  return 3ll * pd * (b2 / QK_TILE) * ((long long)(a / QK_TILE) * ((bt + 3) >> 2) + (long long)(a2 / QK_TILE) * ((at + 3) >> 2));
}
// xd / yd: padded bond rows of the two states (n_sites + 1 entries); the merge of sites e, e + 1 (the caller keeps e + 2 inside the chain).
// (measured on the two headline sets, same box: allowing 1/8 or 1/4 more padded work per merged step loses what the saved barriers
// gain -- 397.4 / 400.0 against 395.7 ms; merging LDS-resident steps only when that saves 6 % of the work: 406 ms)
QK_HD static inline bool qk_merge_admissible(const QkSegRule& r, const int32_t* const xd, const int32_t* const yd, const int e) {
  const int a = xd[e], am = xd[e + 1], a2 = xd[e + 2], b = yd[e], bm = yd[e + 1], b2 = yd[e + 2];
  const long long work_m = 4ll * a * b2 * (b + a2), work_p = 2ll * a * bm * (b + am) + 2ll * am * b2 * (bm + a2);
  return (qk_seg_small(r, a, a2, b, b2, 4) || (!qk_seg_small(r, a, am, b, bm, 2) && !qk_seg_small(r, am, a2, bm, b2, 2))) && work_m <= work_p;
}
// THE ASSOCIATION OF A STEP.  A step is contracted "B first": T = X^T B, then X' = T^T conj(A) (orientation 0).  "A first" is the same code
// with the two states exchanged, working on W = X^H (orientation 1): the same qk_step_instr, qk_seg_small and qk_merge_admissible with the
// two bond rows exchanged.  A step may END WITH A SWITCH: phase 2 then leaves the block of X'^H (qk_fused.h: the source operands of its
// matrix instructions exchanged) and the chain goes on in the other orientation.  Only an LDS-resident step (qk_seg_small in its own
// orientation: X' is written in one strip) may switch; it then costs QK_SWITCH_PRICE more.  With `assoc`
//   0  every step runs in orientation 0 (the masks of the segmentation alone);
//   1  the dynamic programme runs over (site, orientation); the chain may start in either orientation.  Ties: fewer switches, then fewer
//      steps in orientation 1, then the ties of the merges (fewer steps, the even start);
//   2  a test pattern: orientation 0 first, every admissible merge of the orientation at hand, a switch behind every step that may switch;
//   3  the same pattern starting in orientation 1.
// The orientations come back in a second mask: bit i = the step that starts at site ek + i runs in orientation 1 (the second site of a
// merged step repeats its step's bit), bit m = n_sites - 2 ek, one past the chain, = the orientation the chain ENDS in (the right edge is
// then taken with the states exchanged and the chain yields conj(z)).  A step whose successor bit differs is a switch step.  A chain that
// does not leave room for bit m (m >= QK_SEG_BITS) and the greedy rule keep orientation 0.
static constexpr int QK_SWITCH_PRICE = 40;  // matrix instructions' worth of a switch: the switch variant of phase 2 is the simpler loop (qk_fused.h: qkf_p2_switch)
QK_HD static inline bool qk_seg_small_o(const QkSegRule& r, const int o, const int a, const int a2, const int b, const int b2, const int pd) {
  return o ? qk_seg_small(r, b, b2, a, a2, pd) : qk_seg_small(r, a, a2, b, b2, pd);
}
// parities: bit 0 = merges may start at even i (site ek + i), bit 1 = at odd i.  objective / steps (optional): instructions + price per
// step (+ price per switch) and the number of steps of the segmentation returned.  assoc / switch_price / orient / switches: see above.
QK_HD static inline QkSegMask qk_segment_chain(const int32_t* const xd, const int32_t* const xt, const int32_t* const yd, const int32_t* const yt, const int n_sites, const int ek,
                                               const QkSegRule& rule, const int parities, const bool greedy, long long* const objective = nullptr, int* const steps = nullptr,
                                               const int assoc = 0, const int switch_price = QK_SWITCH_PRICE, QkSegMask* const orient = nullptr, int* const switches = nullptr) {
  const int m = n_sites - 2 * ek;
  const int mode = (greedy || m + 1 > QK_SEG_BITS) ? 0 : assoc;
  // (rows of the state that plays x / y in orientation o)
  auto may = [&](const int i, const int o) {
    return i + 1 < m && i < QK_SEG_BITS && ((parities >> (i & 1)) & 1) != 0 && qk_merge_admissible(rule, o ? yd : xd, o ? xd : yd, ek + i);
  };
  auto step_cost = [&](const int i, const int o, const int len) {
    const int e = ek + i;
    return (o ? qk_step_instr(2 * len, yd[e], yd[e + len], xd[e], xd[e + len], yt[e], xt[e]) : qk_step_instr(2 * len, xd[e], xd[e + len], yd[e], yd[e + len], xt[e], yt[e])) + QK_STEP_PRICE;
  };
  auto may_switch = [&](const int i, const int o, const int len) {
    const int e = ek + i;
    return qk_seg_small_o(rule, o, xd[e], xd[e + len], yd[e], yd[e + len], 2 * len);
  };
  auto bit = [](const QkSegMask& k, const int i) { return qk_seg_bit(k.w[0], k.w[1], i); };
  auto set = [](QkSegMask& k, const int i) { k.w[i >> 6] |= 1ull << (i & 63); };
  QkSegMask take[2] = {{{0ull, 0ull}}, {{0ull, 0ull}}};  // [o] bit i: a step that starts at i in orientation o is a merged one
  QkSegMask swit[2] = {{{0ull, 0ull}}, {{0ull, 0ull}}};  // [o] bit i: ... and ends with a switch
  int o_start = 0;
  if (greedy) {
    for (int i = 0; i < m && i < QK_SEG_BITS; ++i)
      if (may(i, 0)) set(take[0], i);
  } else if (mode <= 1) {
    struct Best {  // of the sites [i, m) when the step at i runs in orientation o: cost, switches, steps in orientation 1, steps
      long long c;
      int sw, n1, st;
    };
    auto less = [](const Best& a, const Best& b) { return a.c != b.c ? a.c < b.c : a.sw != b.sw ? a.sw < b.sw : a.n1 != b.n1 ? a.n1 < b.n1 : a.st < b.st; };
    auto same = [](const Best& a, const Best& b) { return a.c == b.c && a.sw == b.sw && a.n1 == b.n1 && a.st == b.st; };
    Best f1[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, f2[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // of the sites [i + 1, m), [i + 2, m)
    const int no = mode == 1 ? 2 : 1;
    for (int i = m - 1; i >= 0; --i) {
      Best f0[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
      for (int o = 0; o < no; ++o) {
        // a step of `len` sites at i, followed by the best of the rest in this orientation or, behind a switch, in the other one
        auto cand = [&](const int len, bool& sw) {
          const Best* const rest = len == 2 ? f2 : f1;
          const long long c = step_cost(i, o, len);
          Best b{c + rest[o].c, rest[o].sw, rest[o].n1 + o, rest[o].st + 1};
          sw = false;
          if (mode == 1 && may_switch(i, o, len)) {
            const Best s{c + switch_price + rest[1 - o].c, rest[1 - o].sw + 1, rest[1 - o].n1 + o, rest[1 - o].st + 1};
            if (less(s, b)) b = s, sw = true;
          }
          return b;
        };
        bool sw = false, swm = false;
        Best b = cand(1, sw);
        if (may(i, o)) {
          const Best bm = cand(2, swm);
          if (less(bm, b) || (same(bm, b) && (i & 1) == 0)) b = bm, sw = swm, set(take[o], i);
        }
        if (sw) set(swit[o], i);
        f0[o] = b;
      }
      for (int o = 0; o < 2; ++o) f2[o] = f1[o], f1[o] = f0[o];
    }
    if (mode == 1 && less(f1[1], f1[0])) o_start = 1;
  } else {
    o_start = mode == 3 ? 1 : 0;
  }
  QkSegMask out{{0ull, 0ull}}, ori{{0ull, 0ull}};
  long long obj = 0;
  int n_steps = 0, n_sw = 0, o = o_start;
  for (int i = 0; i < m; ++n_steps) {
    const bool mg = mode >= 2 ? may(i, o) : bit(take[o], i);
    const int len = mg ? 2 : 1;
    const bool sw = mode >= 2 ? may_switch(i, o, len) : bit(swit[o], i);
    if (mg) set(out, i);
    if (o)
      for (int s = i; s < i + len; ++s) set(ori, s);
    obj += step_cost(i, o, len) + (sw ? switch_price : 0);
    if (sw) o ^= 1, ++n_sw;
    i += len;
  }
  if (o) set(ori, m);  // (o != 0 only with room for this bit)
  if (objective) *objective = obj;
  if (steps) *steps = n_steps;
  if (orient) *orient = ori;
  if (switches) *switches = n_sw;
  return out;
}

// The record of a step in the pair's step table (qk_fused.h: qkf_step_table), 12 ints:
//   [0] a  [1] a2  [2] b  [3] b2  [4] true a  [5] k-steps of b  [6] W  [7] small | orientation << 1 | switch << 2 | the residency of X (qk_rec_resident_bits)  [8] ceil(2^20 / mt)
//   [9] log2 pd  [10] next step  [11] item_recips: the reciprocals of the strips' column units (qk_unit_recips), else 0
// of the step of `len` sites (1, or 2: merged) that starts at site e.  A step in orientation 1 gets the record of the exchanged states.
struct QkStepRec {
  int w[12];
};
static constexpr int QK_REC_SMALL = 1, QK_REC_ORIENT = 2, QK_REC_SWITCH = 4;
QK_HD static inline QkStepRec qk_step_record(const int32_t* xd, const int32_t* xt, const int32_t* yd, const int32_t* yt, const int e, const int len, const int o, const bool sw,
                                             const QkSegRule& rule, const bool item_recips) {
  if (o) {
    const int32_t* t = xd;
    xd = yd, yd = t, t = xt, xt = yt, yt = t;
  }
  const int a = xd[e], a2 = xd[e + len], b = yd[e], b2 = yd[e + len];
  const bool small = qk_seg_small(rule, a, a2, b, b2, 2 * len);
  const int mt = a / QK_TILE, nt = b2 / QK_TILE;
  const int lim = rule.xcap / (QK_TILE * a2), W = small ? nt : (lim < 1 ? 1 : lim < nt ? lim : nt);  // X' in strips of W blocks of b' (the strip's rows must fit the LDS)
  return QkStepRec{{a, a2, b, b2, xt[e], (yt[e] + 3) >> 2, W, (small ? QK_REC_SMALL : 0) | (o ? QK_REC_ORIENT : 0) | (sw ? QK_REC_SWITCH : 0) | qk_rec_resident_bits(rule, a, a2, b, b2, 2 * len), qk_recip20(mt),
                    len == 2 ? 2 : 1, e + len,
                    item_recips ? qk_unit_recips(nt, W, false) : 0}};
}

struct qk_ctx;

struct qk_plan {
  int n_sites = 0, nx = 0, ny = 0;
  bool symmetric = false;
  bool quad = false;  // pairs come in 2x2 blocks (QK_PLAN_QUADS): [4q..4q+3] = (i1,j1), (i2,j1), (i1,j2), (i2,j2)
  int world = 1, rank = 0;
  int64_t total_pairs = 0, max_per_rank = 0;
  std::vector<int32_t> pairs;   // this rank, (i, j) interleaved
  std::vector<int32_t> groups;  // (first pair, count): runs of <= group pairs that share the x state
  int group = 1;
  qk_stats stats{};
  qk_stats second{};       // pairs / flops / padded_flops / bytes of the class-1 run [n_first, end)
  int64_t n_first = 0;     // pairs [n_first, end) are the class whose sites fit the fused sweep's smaller LDS buffer (== number of pairs: no split)
  int nq = 1;                 // device work queues: 1 = one list; 16 = two classes of pairs x 8 XCD queues (the second class may be empty)
  int64_t qstart[17] = {0};   // queue s = pairs [qstart[s], qstart[s + 1]) of this rank's list; queues 8..15 = the class-1 run
  int edge_k = 0;             // sites at either end of the chain that the fused sweep takes from the sets' edge blocks (0: none)
  bool second_wave2 = false;  // the second run holds the pairs of two states whose bonds are all <= 32: swept by the one-wave kernel (mixed sets)
  double fit_two = 1.0;  // share of this rank's padded work in sites whose X and X' fit the fused sweep's smaller LDS buffer
  double fit_narrow = 1.0;  // ... in sites of at most the narrow size (QK_PLAN_FIT: where the two-workgroup shape still beats the 12-wave dual one)
  double tile_reuse_bytes = 0;  // bytes of this rank's share if every state were read once per plan tile it takes part in (the tile-reuse lower bound)
  double plan_ms = 0;           // host time qk_plan_create spent on this plan
  int plan_threads = 1;         // host threads it used
  // lazily uploaded copy
  qk_ctx* up_ctx = nullptr;
  int32_t* d_pairs = nullptr;
  int32_t* d_groups = nullptr;
  // the segmentation masks of this plan's pairs (qk_segment_chain; four words per pair: merges, orientations), made on the device by the first Gram and kept
  // while the sets, the run-time edge_k, the rule and the launches stay the same (seg_key; qkgram.hip: ensure_segments)
  unsigned long long* d_seg = nullptr;
  unsigned long long seg_key[8] = {0};
};

// ----------------------------------------------------------------------------------------
// The choice of the sweep's launches (qk_gram_values).  Inline and static on purpose: experiment builds recompile qkgram.hip alone with
// other QKF_XCAP_* / QKF_TWO_WGS, and the choice must see the constants of the translation unit that launches.
// ----------------------------------------------------------------------------------------
// the context's switches, read from the environment once per context (ctx_init) -- fused_dual and gang once per call (qk_gram_values)
struct QkSweepPolicy {
  int variant = 20;        // 20 = the shipped kernels.  Anything else exists only in libqklab.so (QK_VARIANT there: 17 = lean register-staged sweep; 0, 2, 12, 13, 14, 16, 21, 23 = other kernels kept for A/B; 9, 19 = instrumented)
  int wgs_per_cu = 2;      // resident workgroups per CU (QK_WGS_PER_CU)
  bool wave_path = true;   // fp64 sets whose bonds are all <= 16 use the one-wave-per-pair register sweep (QK_WAVE=0 opts out)
  bool wave2_ring = true;  // ... with its k-step groups prefetched through a per-wave LDS ring (QK_WAVE2=2: plain loads)
  bool wave2_path = true;  // fp64 sets whose bonds are all <= 32 use the one-wave-per-pair sweep with 2 x 2 register tiles (QK_WAVE2=0 opts out)
  bool small_path = true;  // sets whose bonds are all <= 32 use the LDS-resident small-bond sweep (QK_SMALL=0 opts out)
  int fused_path = 1;      // fp64 sets with a bond > 32 use the site-fused sweep (QK_FUSED=0: ring sweep instead; 2: also for bonds 17..32)
  int fused_split = 1;     // sweep the plan's two runs of pairs with the two shapes of the site-fused kernel: 1 = when the share is long enough for two launches (default), 2 = always, 0 = one shape (QK_FUSED_SPLIT)
  int fused_wgs = 0;       // workgroups per CU of the site-fused sweep: 0 = chosen per launch from the plan, 1 / 2 forced (QK_FUSED_WGS)
  bool deterministic = false;  // QK_DETERMINISTIC=1: only kernels that add in a fixed order (no LDS atomics)
  int merge_mode = 2;          // QK_MERGE: the site-fused sweep walks the chain in merged steps of two sites (qk_segment_chain) -- 0 = never, 1 = every admissible merge of the fixed pairs (k + 2 t, k + 2 t + 1), 2 = at either parity, chosen per pair by dynamic programming
  int assoc_mode = 1;          // QK_ASSOC: the association of the steps of the site-fused sweep (qk_segment_chain; with merge_mode 2 only) -- 0 = "B first" throughout, 1 = chosen per step and pair by the dynamic programme, 2 / 3 = test patterns that switch wherever a switch is allowed; QK_DETERMINISTIC=1 forces 0
  int switch_price = QK_SWITCH_PRICE;  // QK_SWITCH_PRICE: what the programme charges for a switch, in matrix instructions
  bool fused_dual = true;      // QK_FUSED_DUAL (0: single tiles): the 12-wave site-fused shape in its dual form (pairs of tiles per wave)
  bool gang = false;           // QK_GANG=1: gang start of the site-fused launches (qk_device.h: qk_gang_sync)
  bool fused_big = true;       // QK_FUSED_BIG (0: the instantiations with the segmentation's buffer): the 12-wave site-fused shapes with the large X buffer (QKF_RCAP_ONE) when the chain's tables leave it room
};

struct QkSetShape {  // what the choice needs of a set: its largest padded bond, bits of a real, sites
  int max_pad = 0, precision = 64, n_sites = 0;
};

struct QkSweepRun {  // one launch
  int kernel = QK_KERNEL_NONE;
  long long grid = 0;
  size_t lds = 0;                  // dynamic LDS bytes
  long long first = 0, count = 0;  // pairs [first, first + count) of the plan's list
  int nq = 1, gang_n = 0;          // SweepArgs
  bool big = false;                // a 12-wave site-fused launch runs the instantiation with the LARGE X buffer (QKF_RCAP_ONE): its tables fit behind it
  size_t lds_launch = 0;           // the dynamic LDS bytes the launch really asks for (qk_stats.lds_bytes): `lds`, or with `big` the large buffer and the same tables
  bool gang2 = false;              // its gang words lie behind the first launch's (the second launch of a split sweep)
};

struct QkSweepChoice {
  int rc = QK_OK;  // else no launch, and err says why
  char err[192] = {};
  int n_runs = 0;  // 2: the plan's second class of pairs swept by a launch of its own, right behind the first (a split or mixed sweep)
  QkSweepRun run[2];
  long long launched_grid = 0;  // qk_stats.grid (a split or mixed sweep reports the whole share's grid)
  long long x_plane = 0, t_plane = 0;  // SweepArgs
  int turn_ints = 0;                   // SweepArgs
  size_t scratch_bytes = 0;            // global X / T buffers of the launches
  bool interleaved = false;   // the sweep reads the sets' interleaved images
  bool fused_images = false;  // ... and the site-fused sweep's edge blocks and merged steps (as far as the plan's edge_k and merge_mode ask)
  int queues = 1;             // qk_stats.queues (8: the plan's XCD queues)
  bool tails = false;         // the launches record tail clocks
};

static inline QkSweepChoice qk_choose_sweep(const QkSweepPolicy& p, const qk_plan& plan, const QkSetShape& x, const QkSetShape& y, const int num_cus) {
  QkSweepChoice ch;
  const long long np = (long long)plan.pairs.size() / 2;
  const bool f32 = x.precision == 32, quad = plan.quad, det = p.deterministic;
  const int n = x.n_sites, max_pad = std::max(x.max_pad, y.max_pad);
  // X/T scratch: the group sweep (lab) stacks GMAX pairs in one buffer, the duo sweep (lab) keeps two buffer sets, the quad kernel 2 stacked sets
  const bool grouped = p.variant == 14 && !f32 && !quad, duo = p.variant == 16 && !f32 && !quad;
  const long long chains = quad ? 4 : (duo ? 2 : 1);
  const long long units = quad ? np / 4 : grouped ? (long long)plan.groups.size() / 2 : (duo ? (np + 1) / 2 : np);
  ch.x_plane = (grouped ? GMAX : 1) * (long long)x.max_pad * y.max_pad, ch.t_plane = 2 * ch.x_plane;
  // The site-fused sweep (qk_fused.h), fp64.  Two shapes: one 12-wave workgroup per CU (three waves per SIMD, two T slots each) with an 8192-element X buffer, or
  // two 8-wave workgroups (four waves per SIMD, one slot) with 4608 elements each.  The second workgroup fills the first one's barriers and per-site set-up (+24 %
  // on the 40-qubit x 4-layer set), but every site that does not fit the smaller buffer runs in strips from a global X.  A 16-row strip of X' must fit: bonds <= XCAP / 16.
  ch.turn_ints = det ? (y.max_pad / QK_TILE) * (x.max_pad / QK_TILE) : 0;  // DET forms: turn counters per set = blocks of b' x blocks of a' of the largest site
  const size_t lds_meta = 16 + 256 + (size_t)n * (48 + 16) + (det ? (size_t)(2 * ch.turn_ints + 2) * sizeof(int) : 0);  // queue slot, the overlap's accumulator, per-site records and tensor offsets, two sets of turn counters
  const bool can_one = max_pad <= QKF_XCAP_ONE / QK_TILE && (size_t)QKF_XCAP_ONE * 16 + lds_meta <= 160 * 1024;
  const bool can_two = max_pad <= QKF_XCAP_TWO / QK_TILE && (size_t)QKF_XCAP_TWO * 16 + lds_meta <= 160 * 1024 / QKF_TWO_WGS;
  const bool fused = p.variant == 20 && !f32 && !quad && p.fused_path != 0 && max_pad > (p.fused_path >= 2 ? 16 : 32) && (can_one || can_two);
  const bool second_class = fused && plan.n_first > 0 && plan.n_first < np;
  // split: the plan's two runs of pairs with the two shapes (see qk_plan_create), only when the launch is free to choose its shape and the share is long enough -- a
  // short launch ends with a tail of its own (a 1/8 share of the 60-qubit x 6-layer Gram, 61 pairs per CU: two launches 47.2 ms, ONE launch of the 12-wave dual shape
  // 47.1 ms: profiles/r04/share_times_cfg4.txt), so below 100 pairs per CU the share is one launch
  const bool split = second_class && can_one && can_two && p.fused_wgs == 0 && p.fused_split != 0 && !plan.second_wave2 && (p.fused_split == 2 || np >= 100ll * num_cus);
  // mixed: the plan's second run holds the pairs of two small states (every bond <= 32) for the one-wave sweep
  const bool mixed = second_class && plan.second_wave2 && p.wave2_path && p.wave2_ring;
  // one class of pairs: the two-workgroup shape when the work sits in sites that fit its buffer AND most of it in sites of at most the narrow
  // size -- from about 4 x 4 tiles per site the 12-wave dual shape is the faster one although the site would still fit (tools/uniform_ab.py)
  const bool fused_two = fused && can_two && !split && (!can_one || p.fused_wgs == 2 || (p.fused_wgs == 0 && plan.fit_two >= 0.75 && plan.fit_narrow >= 0.5));
  // the dual form (pairs of tiles per wave) against single tiles, uniform bonds 48 / 64 / 96 / 128 / 256: +2 / +4 / +7 / +12 / +19 %
  const bool dual = fused && !fused_two && p.fused_dual;
  const int wgs = fused ? (fused_two ? QKF_TWO_WGS : 1) : p.wgs_per_cu;
  const long long grid = std::min(units, (long long)wgs * num_cus);
  ch.scratch_bytes = (size_t)(split ? 2ll * num_cus : grid) * (size_t)chains * 2 * (size_t)(ch.x_plane + ch.t_plane) * sizeof(double);
  // per-pair site metadata in LDS behind the ring's three slots or the small-bond sweep's X and T: 4 (n+1) ints + 2 n int64 (+ alignment)
  const size_t site_meta = 16 + (size_t)(4 * (n + 1) + 2) * sizeof(int) + (size_t)2 * n * sizeof(long long);
  const size_t lds_ring = 3 * 16 * 1024 + site_meta;
  const size_t esz = f32 ? sizeof(float) : sizeof(double), lds_small = (size_t)(3 * 2 * (64 / esz) * 64 + 6 * 32 * 32) * esz + site_meta;
  if (lds_ring > 80 * 1024)
    return ch.rc = QK_EINVAL, snprintf(ch.err, sizeof ch.err, "qk_gram_values: %d sites need %zu bytes of LDS per workgroup (limit 80 KiB for 2 workgroups per CU)", n, lds_ring), ch;
  QkSweepRun& r = ch.run[0];
  ch.n_runs = 1, ch.launched_grid = r.grid = grid, r.count = np;
  if (quad) {  // 2x2 blocks of pairs per workgroup (QK_PLAN_QUADS plans): an experimental kernel of the lab library
#ifdef QK_LAB
    r.kernel = QK_KERNEL_LAB;
#else
    ch.rc = QK_EINVAL, snprintf(ch.err, sizeof ch.err, "qk_gram_values: QK_PLAN_QUADS plans are swept by an experimental kernel that only libqklab.so contains");
#endif
  } else if (p.variant == 20 && p.wave_path && !f32 && max_pad <= 16) {
    // every bond <= 16: a pair lives in the registers of one wavefront (qk_sweep_wave_kernel); 16 waves per CU
    r.kernel = QK_KERNEL_WAVE, ch.launched_grid = r.grid = std::min(np, 16ll * num_cus);
  } else if (!fused && p.variant == 20 && p.wave2_path && (!f32 || p.wave2_ring) && max_pad <= 32) {
    // every bond <= 32: a pair lives in the registers of one wavefront as 2 x 2 tiles (qk_sweep_wave2_kernel); 8 waves per CU
    r.kernel = (f32 || p.wave2_ring) ? QK_KERNEL_WAVE2 : QK_KERNEL_WAVE2_PLAIN, ch.launched_grid = r.grid = std::min(np, 8ll * num_cus);
    ch.interleaved = ch.tails = true, ch.queues = plan.nq > 1 ? 8 : 1, r.nq = plan.nq;
  } else if (!fused && p.variant == 20 && p.small_path && max_pad <= 32 && lds_small <= 80 * 1024) {
    // every bond <= 32: X and T stay in LDS, only the site tensors stream (qk_sweep_small_kernel); longer chains (several hundred sites) take the ring kernel below
    r.kernel = QK_KERNEL_SMALL, r.lds = lds_small;
  } else if (fused) {
    // X in LDS, T in registers, site tensors read straight into MFMA fragments from the interleaved image
    ch.interleaved = ch.fused_images = ch.tails = true, ch.queues = plan.nq > 1 ? 8 : 1, r.nq = plan.nq;
    r.kernel = fused_two ? (det ? QK_KERNEL_FUSED2_DET : QK_KERNEL_FUSED2) : dual ? (det ? QK_KERNEL_FUSED_DUAL_DET : QK_KERNEL_FUSED_DUAL) : (det ? QK_KERNEL_FUSED1_DET : QK_KERNEL_FUSED1);
    r.lds = (size_t)(fused_two ? QKF_XCAP_TWO : QKF_XCAP_ONE) * 16 + lds_meta;
    // the 12-wave shapes take the large buffer (the residency of X alone sees it: the same plan, masks and step table) whenever the launch's
    // tables fit the room the kernels' LDS layout leaves behind it -- chains of up to about 120 sites; DET: fewer, the turn counters grow with
    // the bonds -- else, and with QK_FUSED_BIG=0, the instantiation with the segmentation's buffer
    r.big = !fused_two && p.fused_big && QKF_RCAP_ONE > QKF_XCAP_ONE && lds_meta <= (size_t)QKF_META_ROOM;
    if (r.big) r.lds_launch = (size_t)QKF_RCAP_ONE * 16 + lds_meta;
    // gang start: the workgroups of an XCD begin their pairs together; workgroups per XCD = grid / 8 (round-robin dispatch)
    auto gang_of = [&](const long long g) { return p.gang && plan.nq > 1 && g >= 16 && g % 8 == 0 ? (int)(g / 8) : 0; };
    if (split || mixed) {  // the first class with the shape above, then the second class, back to back on the stream; 8 queues per class
      QkSweepRun& r2 = ch.run[1];
      ch.n_runs = 2;
      r.count = plan.n_first, r2.first = plan.n_first, r2.count = np - plan.n_first;
      r.nq = r2.nq = plan.nq > 1 ? 8 : plan.nq;
      r.grid = std::min(r.count, (long long)wgs * num_cus);
      if (split) {  // pairs whose sites fit the smaller LDS buffer: two 8-wave workgroups per CU
        r2.kernel = det ? QK_KERNEL_FUSED2_DET : QK_KERNEL_FUSED2, r2.grid = std::min(r2.count, (long long)QKF_TWO_WGS * num_cus);
        r2.lds = (size_t)QKF_XCAP_TWO * 16 + lds_meta, r2.gang_n = gang_of(r2.grid), r2.gang2 = true;
      } else {  // pairs of two small states: the one-wave sweep
        r2.kernel = QK_KERNEL_WAVE2, r2.grid = std::min(r2.count, 8ll * num_cus);
      }
    }
    r.gang_n = gang_of(r.grid);
  } else if (f32 || p.variant == 20) {  // the ring sweep: LDS-DMA staging ring (K-tile 8, three slots) + 3M complex product; complex64 sets too
    r.kernel = QK_KERNEL_RING, r.lds = lds_ring;
  } else {  // experimental / diagnostic kernels (qk_lab.hip, libqklab.so only)
#ifdef QK_LAB
    r.kernel = QK_KERNEL_LAB;
#else
    ch.rc = QK_EINVAL, snprintf(ch.err, sizeof ch.err, "qk_gram_values: no kernel for this call");
#endif
  }
  for (int i = 0; i < ch.n_runs; ++i)
    if (!ch.run[i].big) ch.run[i].lds_launch = ch.run[i].lds;
  return ch;
}
