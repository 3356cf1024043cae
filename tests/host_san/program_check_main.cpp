// Host-only sanitizer driver for the one validation of a gate program (csrc/qk_program.h: qk_program_check_tables, qk_program_check),
// built with -fsanitize=address,undefined and run by tests/test_program_check_san.py in the CPU tier.  One good 4-qubit program that
// uses every table -- each table a heap block exactly as long as its largest index needs, so a read past a table is seen -- must
// pass; every rejection of the matrix-gate, channel, two-qubit-channel and condition families must come back with its kind and the
// gate named; and in a two-state program with per-state matrix tables and branch rows a fault in state 1 alone must be found and
// attributed to state (row) 1.  Test infrastructure: nothing of the product links it.
#include "../../qml-cutensornet_amd/csrc/qk_program.h"

#include <complex>
#include <cstring>
#include <functional>
#include <limits>

using cd = std::complex<double>;
using M = std::vector<cd>;

namespace {
const M I2 = {1, 0, 0, 1}, X = {0, 1, 1, 0}, Y = {0, cd(0, -1), cd(0, 1), 0}, Z = {1, 0, 0, -1};

M kron(const M& a, const M& b, double f) {
  M o(16);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k)
        for (int l = 0; l < 2; ++l) o[(size_t)(i * 2 + k) * 4 + (j * 2 + l)] = f * a[(size_t)i * 2 + j] * b[(size_t)k * 2 + l];
  return o;
}

// The tables of a program for `states` states; every vector is exactly as long as the program reads.
struct Prog {
  int states = 1, n = 4;
  std::vector<int8_t> op;
  std::vector<int32_t> q0, mat, channel, branch, n_kraus, n_kraus2, cond_gate;
  std::vector<uint32_t> cond_mask;
  std::vector<double> alpha;
  std::vector<cd> mats, kraus, kraus2;  // [states][n_mats][4][4], [n_channels][4][2][2], [n_channels2][16][4][4]
  bool rows = true, mask = true, table1 = true, table2 = true, table_m = true;

  qk_program view() const {
    qk_program p = {};
    p.size = sizeof p, p.n_states = states, p.n_qubits = n, p.n_ops = (int32_t)op.size(), p.op = op.data(), p.q0 = q0.data(), p.alpha = alpha.data();
    if (table_m) p.n_mats = 2, p.mats_state_stride = states > 1 ? 2 : 0, p.mats = reinterpret_cast<const double*>(mats.data()), p.mat = mat.data();
    if (table1) p.n_channels = (int32_t)n_kraus.size(), p.kraus = reinterpret_cast<const double*>(kraus.data()), p.n_kraus = n_kraus.data();
    if (table2) p.n_channels2 = (int32_t)n_kraus2.size(), p.kraus2 = reinterpret_cast<const double*>(kraus2.data()), p.n_kraus2 = n_kraus2.data();
    if (table1 || table2) p.channel = channel.data(), p.branch = branch.data(), p.branch_state_stride = states > 1 ? p.n_ops : 0;
    if (rows) p.cond_gate = cond_gate.data(), p.cond_mask = mask ? cond_mask.data() : nullptr;
    return p;
  }
};

// H(0); 2x2 from the table on 1; damping on 1 (drawn); 4x4 from the table on (2, 3); two-qubit depolarising on (0, 1) (drawn, 16
// matrices: the last two-qubit channel); XXPhase(1, 2) if gate 2 took branch 0; one-qubit depolarising on 3, branch 2 forced (4
// matrices: the last channel), if gate 4 took branch 0 or 15; Rz(3) if gate 6 took branch 3.  The last entry of every table is in use.
Prog good(int states) {
  Prog g;
  g.states = states;
  g.op = {0, 8, 10, 9, 11, 2, 10, 1};
  g.q0 = {0, 1, 1, 2, 0, 1, 3, 3};
  g.mat = {-1, 0, -1, 1, -1, -1, -1, -1};
  g.channel = {-1, -1, 0, -1, 1, -1, 1, -1};
  g.cond_gate = {-1, -1, -1, -1, -1, 2, 4, 6};
  g.cond_mask = {0, 0, 0, 0, 0, 1u, 0x8001u, 8u};
  g.alpha.assign((size_t)states * 8, 0.3);
  for (int s = 0; s < states; ++s) {
    const int32_t row[8] = {-1, -1, -1, -1, -1, -1, 2, -1};
    g.branch.insert(g.branch.end(), row, row + 8);
    M slot(32, cd(0, 0));  // entry 0: Y in [:2][:2]; entry 1: CX
    slot[0] = Y[0], slot[1] = Y[1], slot[4] = Y[2], slot[5] = Y[3];
    slot[16 + 0] = slot[16 + 5] = slot[16 + 11] = slot[16 + 14] = 1;
    g.mats.insert(g.mats.end(), slot.begin(), slot.end());
  }
  const double p = 0.4, q = 0.5;
  g.n_kraus = {2, 4};
  g.kraus.assign(2 * 16, cd(0, 0));
  g.kraus[0] = 1, g.kraus[3] = std::sqrt(1 - p), g.kraus[4 + 1] = std::sqrt(p);  // amplitude damping
  const M* paulis[4] = {&I2, &X, &Y, &Z};
  for (int k = 0; k < 4; ++k)
    for (int e = 0; e < 4; ++e) g.kraus[16 + (size_t)k * 4 + e] = (*paulis[k])[(size_t)e] * std::sqrt(k ? q / 4 : 1 - 0.75 * q);
  g.n_kraus2 = {4, 16};
  g.kraus2.assign(2 * 256, cd(0, 0));
  for (int k = 0; k < 4; ++k) g.kraus2[(size_t)k * 16 + (size_t)k * 5] = 1;  // the projective measurement of a pair
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      const M pq = kron(*paulis[a], *paulis[b], std::sqrt(a + b ? q / 16 : 1 - 15 * q / 16));
      std::copy(pq.begin(), pq.end(), g.kraus2.begin() + 256 + (a * 4 + b) * 16);
    }
  return g;
}

int rejected = 0, missed = 0;

// `edit` applied to the good program must be refused with `kind` (-1: by qk_program_check_tables) and a message that holds `text`
void bad(const char* label, int kind, const char* text, const std::function<void(Prog&)>& edit, int states = 1) {
  Prog g = good(states);
  edit(g);
  const qk_program p = g.view();
  std::string what;
  const int got = qk_program_check_tables(p, &what) ? qk_program_check(p, &what) : -1;
  if (got == kind && std::strstr(what.c_str(), text)) {
    ++rejected;
    return;
  }
  ++missed;
  std::printf("MISSED %s: expected kind %d with '%s', got %d (%s)\n", label, kind, text, got, what.c_str());
}
}  // namespace

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int T = QK_PROGRAM_BAD_TABLE, U = QK_PROGRAM_UNKNOWN_OP;
  for (int states = 1; states <= 2; ++states) {
    const Prog g = good(states);
    const qk_program p = g.view();
    std::string what;
    if (!qk_program_check_tables(p, &what) || qk_program_check(p, &what) != QK_PROGRAM_OK) {
      std::printf("FAILED: the good program of %d state(s) was refused: %s\n", states, what.c_str());
      return 1;
    }
  }
  std::printf("accepted: exact tables, 1 and 2 states\n");
  // ---- matrix gates (tests/test_matrix_gates_host.py: bad_programs)
  bad("not unitary", T, "gate 1: the matrix of table entry 0 (state 0) is not unitary", [](Prog& g) { g.mats[0] = 1, g.mats[1] = 1, g.mats[4] = 0, g.mats[5] = 1; });
  bad("not unitary by 2e-9", T, "gate 3: the matrix of table entry 1 (state 0) is not unitary", [](Prog& g) { for (int e = 16; e < 32; ++e) g.mats[(size_t)e] *= 1 + 1e-9; });
  bad("NaN", T, "gate 3: the matrix of table entry 1 (state 0) has an entry that is not finite", [&](Prog& g) { g.mats[16 + 9] = nan; });
  bad("index out of range", T, "gate 3: matrix index 2 outside 0..1", [](Prog& g) { g.mat[3] = 2; });
  bad("negative index", T, "gate 1: matrix index -1", [](Prog& g) { g.mat[1] = -1; });
  bad("M2 on the last qubit", QK_PROGRAM_MATRIX_GATE_OUTSIDE, "gate 3 on a qubit outside the register", [](Prog& g) { g.q0[3] = 3; });
  bad("no table", U, "unknown gate op code 8 at position 1 (valid: 0..7, 10, 11)", [](Prog& g) { g.table_m = false; });
  bad("code 10 with a matrix table only", U, "unknown gate op code 10 at position 2 (valid: 0..9)", [](Prog& g) { g.table1 = g.table2 = g.rows = false; });
  // ---- channels of code 10 (tests/test_channels_host.py: bad_channel_programs)
  bad("channel outside the table", T, "gate 2: channel index 2 outside 0..1", [](Prog& g) { g.channel[2] = 2; });
  bad("negative channel", T, "gate 6: channel index -1", [](Prog& g) { g.channel[6] = -1; });
  bad("no Kraus matrix", T, "gate 2: channel 0 has 0 Kraus matrices (1..4)", [](Prog& g) { g.n_kraus[0] = 0; });
  bad("five Kraus matrices", T, "gate 6: channel 1 has 5 Kraus matrices (1..4)", [](Prog& g) { g.n_kraus[1] = 5; });
  bad("NaN", T, "gate 6: a Kraus matrix of channel 1 has an entry that is not finite", [&](Prog& g) { g.kraus[16 + 5] = nan; });
  bad("inf", T, "gate 2: a Kraus matrix of channel 0 has an entry that is not finite", [&](Prog& g) { g.kraus[7] = cd(0, inf); });
  bad("branch too large", T, "gate 2: branch 2 (row 0) outside -1..1", [](Prog& g) { g.branch[2] = 2; });
  bad("branch below -1", T, "gate 6: branch -2", [](Prog& g) { g.branch[6] = -2; });
  bad("drawn, not trace preserving by 4e-9", T, "gate 2: the drawn channel 0 is not trace preserving", [](Prog& g) { for (int e = 4; e < 8; ++e) g.kraus[(size_t)e] *= 1 + 2e-9; });
  bad("drawn projector", T, "gate 6: the drawn channel 1 is not trace preserving", [](Prog& g) { g.n_kraus[1] = 1, g.branch[6] = -1; });
  bad("outside the register", T, "gate 6: channel on a qubit outside the register", [](Prog& g) { g.q0[6] = 4; });
  bad("code 10 without a table", U, "unknown gate op code 10 at position 2 (valid: 0..9, 11)", [](Prog& g) { g.table1 = false; });
  // ---- channels of code 11 (tests/test_channels2_host.py: bad_channel2_programs)
  bad("channel outside the table", T, "gate 4: two-qubit channel index 2 outside 0..1", [](Prog& g) { g.channel[4] = 2; });
  bad("negative channel", T, "gate 4: two-qubit channel index -1", [](Prog& g) { g.channel[4] = -1; });
  bad("no Kraus matrix", T, "gate 4: two-qubit channel 1 has 0 Kraus matrices (1..16)", [](Prog& g) { g.n_kraus2[1] = 0; });
  bad("seventeen Kraus matrices", T, "gate 4: two-qubit channel 1 has 17 Kraus matrices (1..16)", [](Prog& g) { g.n_kraus2[1] = 17; });
  bad("NaN", T, "gate 4: a Kraus matrix of two-qubit channel 1 has an entry that is not finite", [&](Prog& g) { g.kraus2[256 + 17] = nan; });
  bad("inf", T, "gate 4: a Kraus matrix of two-qubit channel 1 has an entry that is not finite", [&](Prog& g) { g.kraus2[511] = cd(0, inf); });
  bad("branch too large", T, "gate 4: branch 16 (row 0) outside -1..15", [](Prog& g) { g.branch[4] = 16; });
  bad("branch below -1", T, "gate 4: branch -2", [](Prog& g) { g.branch[4] = -2; });
  bad("drawn, not trace preserving by 4e-9", T, "gate 4: the drawn two-qubit channel 1 is not trace preserving", [](Prog& g) { for (int e = 16; e < 32; ++e) g.kraus2[256 + (size_t)e] *= 1 + 2e-9; });
  bad("drawn projector", T, "gate 4: the drawn two-qubit channel 0 is not trace preserving", [](Prog& g) { g.channel[4] = 0, g.n_kraus2[0] = 1, g.cond_mask[6] = 1u; });
  bad("pair outside the register", T, "gate 4: two-qubit channel on a qubit outside the register", [](Prog& g) { g.q0[4] = 3; });
  bad("code 11 without a two-qubit table", U, "unknown gate op code 11 at position 4 (valid: 0..9, 10)", [](Prog& g) { g.table2 = false; });
  // ---- condition rows (tests/test_conditions_host.py: bad_condition_programs)
  bad("rows without a channel table", -1, "gate 0: condition rows need a program with a channel table", [](Prog& g) { g.table1 = g.table2 = false; });
  bad("cond_gate below -1", T, "gate 1: condition on gate -2 outside -1..0", [](Prog& g) { g.cond_gate[1] = -2; });
  bad("a condition on itself", T, "gate 5: condition on gate 5 outside -1..4", [](Prog& g) { g.cond_gate[5] = 5; });
  bad("a condition on a later gate", T, "gate 3: condition on gate 4 outside -1..2", [](Prog& g) { g.cond_gate[3] = 4; });
  bad("a condition on a gate that is no channel", T, "gate 7: condition on gate 3, which is no channel gate (op code 9)", [](Prog& g) { g.cond_gate[7] = 3; });
  bad("a mask bit above the two branches", T, "gate 5: condition mask names a branch at or above the 2 of gate 2", [](Prog& g) { g.cond_mask[5] = 4u; });
  bad("a mask bit above the four branches", T, "gate 7: condition mask names a branch at or above the 4 of gate 6", [](Prog& g) { g.cond_mask[7] = 1u << 4; });
  bad("no cond_mask", -1, "condition rows need cond_gate and cond_mask", [](Prog& g) { g.mask = false; });
  // ---- two states with tables and rows of their own: the fault is in state 1 alone
  bad("state 1: not unitary", T, "gate 3: the matrix of table entry 1 (state 1) is not unitary", [](Prog& g) { g.mats[32 + 16 + 5] = 0.5; }, 2);
  bad("state 1: NaN", T, "gate 1: the matrix of table entry 0 (state 1) has an entry that is not finite", [&](Prog& g) { g.mats[32 + 4] = nan; }, 2);
  bad("row 1: branch too large", T, "gate 6: branch 4 (row 1) outside -1..3", [](Prog& g) { g.branch[8 + 6] = 4; }, 2);
  bad("row 1 draws a channel that row 0 forces", T, "gate 6: the drawn channel 1 is not trace preserving", [](Prog& g) { g.kraus[16 + 4 * 2 + 1] *= 2, g.branch[8 + 6] = -1; }, 2);
  {  // ... which both rows may force
    Prog g = good(2);
    g.kraus[16 + 4 * 2 + 1] *= 2;
    const qk_program p = g.view();
    std::string what;
    if (!qk_program_check_tables(p, &what) || qk_program_check(p, &what) != QK_PROGRAM_OK) ++missed, std::printf("MISSED: a forced branch may be any finite matrix (%s)\n", what.c_str());
  }
  std::printf("%d rejections ok, %d missed\n", rejected, missed);
  return missed ? 1 : 0;
}
