// qk_program.h -- what both MPS builders (qk_build.hip on the device, qk_builder.cpp on the host) know about a gate program
// (qk_program, include/qkgram.h) before they run it: the op codes and the one validation.  Plain C++17, header only, no HIP.
#ifndef QK_PROGRAM_H
#define QK_PROGRAM_H
#include "../../include/qkgram.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

// ansatz.py.  Codes 8 and 9 are the matrix gates: valid only in a program that comes with a matrix table (N_OPS_MAT codes then).
// Code 10 is the one-qubit Kraus channel: valid only in a program that comes with a channel table; code 11 the two-qubit Kraus
// channel on (q0, q0+1): valid only in a program that comes with a two-qubit channel table.
enum { OP_H = 0, OP_RZ = 1, OP_XX = 2, OP_SWAP = 3, OP_RX = 4, OP_RY = 5, OP_YY = 6, OP_ZZ = 7, N_OPS = 8, OP_M1 = 8, OP_M2 = 9, N_OPS_MAT = 10, OP_K1 = 10, OP_K2 = 11 };

// what qk_program_check found (the host builder tells them apart in its return code)
enum { QK_PROGRAM_OK = 0, QK_PROGRAM_UNKNOWN_OP = 1, QK_PROGRAM_BAD_TABLE = 2, QK_PROGRAM_MATRIX_GATE_OUTSIDE = 3 };

template <typename... T>
inline std::string qk_program_text(const char* fmt, T... v) {
  char buf[256];
  std::snprintf(buf, sizeof buf, fmt, v...);
  return buf;
}

// max |G - 1| over the d x d matrix G = sum_{k<m} K_k^H K_k, K row-major [m][d][ld] complex as (re, im) pairs: the deviation of a
// matrix gate (m = 1) from unitary and of a channel from trace preserving
inline double qk_program_gram_deviation(const double* K, int m, int d, int ld) {
  double dev = 0;
  for (int a = 0; a < d; ++a)
    for (int b = 0; b < d; ++b) {
      double gr = (a == b) ? -1.0 : 0.0, gi = 0.0;  // G[a][b] - delta = sum_{k,r} conj(K_k[r][a]) K_k[r][b] - delta
      for (int k = 0; k < m; ++k)
        for (int r = 0; r < d; ++r) {
          const double *x = K + (((size_t)k * d + r) * ld + a) * 2, *y = K + (((size_t)k * d + r) * ld + b) * 2;
          gr += x[0] * y[0] + x[1] * y[1], gi += x[0] * y[1] - x[1] * y[0];
        }
      dev = std::max(dev, std::hypot(gr, gi));
    }
  return dev;
}

// Whether the tables a program names can be read at all: counts, pointers, strides.  `what` takes what is wrong.
inline bool qk_program_check_tables(const qk_program& p, std::string* what) {
  const bool chan = p.n_channels > 0 || p.n_channels2 > 0;
  if (p.cond_gate && !p.cond_mask) *what = "condition rows need cond_gate and cond_mask";
  else if (p.cond_gate && !chan) *what = "gate 0: condition rows need a program with a channel table";
  else if (p.n_channels2 < 0 || (p.n_channels2 > 0 && (!p.kraus2 || !p.n_kraus2 || !p.channel || !p.branch)))
    *what = "a two-qubit channel table needs n_channels2 >= 0, kraus2, n_kraus2, channel and branch";
  else if (p.n_channels < 0 || (p.n_channels > 0 && (!p.kraus || !p.n_kraus || !p.channel || !p.branch)))
    *what = "a channel table needs n_channels >= 0, kraus, n_kraus, channel and branch";
  else if (chan && p.branch_state_stride != 0 && p.branch_state_stride != p.n_ops)
    *what = qk_program_text("branch_state_stride must be 0 (one row for all states) or n_ops = %d, got %d", (int)p.n_ops, (int)p.branch_state_stride);
  else if (p.n_mats < 0 || (p.n_mats > 0 && (!p.mats || !p.mat))) *what = "a matrix table needs n_mats >= 0, mats and mat";
  else if (p.n_mats > 0 && p.mats_state_stride != 0 && p.mats_state_stride != p.n_mats)
    *what = qk_program_text("mats_state_stride must be 0 (one table for all states) or n_mats = %d, got %d", (int)p.n_mats, (int)p.mats_state_stride);
  else return true;
  return false;
}

// The gates of a program against its tables (qk_program_check_tables has passed; op, q0 and the counts are there), before anything
// runs, in this order:
//   * every op code inside the vocabulary: 0..7, 8 and 9 with a matrix table, 10 and 11 with their channel tables;
//   * every matrix gate inside the register; its index inside 0..n_mats-1 and, in the table of every state, its 2x2 ([:2][:2] of
//     the slot) or 4x4 finite and unitary, max |M^H M - 1| <= 1e-12;
//   * every channel gate: the channel inside its table, 1..4 matrices (1..16 for code 11), finite entries, the branch of every row
//     inside -1..m-1, a drawn channel trace preserving, max |sum_k K_k^H K_k - 1| <= 1e-12 (a forced branch may be any finite
//     matrix), the qubit (pair) inside the register;
//   * the condition rows: cond_gate[i] inside -1 .. i-1, the gate it names of op code 10 or 11, no mask bit at or above the number
//     of Kraus matrices of that gate's channel.
// QK_PROGRAM_OK, or the kind of the first fault with `what` naming the gate (and the state or row).
inline int qk_program_check(const qk_program& p, std::string* what) {
  const int n_ops = p.n_ops, n_mats = std::max(0, (int)p.n_mats);
  const bool with_k1 = p.n_channels > 0, with_k2 = p.n_channels2 > 0;
  const int n_codes = n_mats > 0 ? N_OPS_MAT : N_OPS;
  for (int i = 0; i < n_ops; ++i)
    if ((p.op[i] < 0 || p.op[i] >= n_codes) && !(with_k1 && p.op[i] == OP_K1) && !(with_k2 && p.op[i] == OP_K2)) {
      *what = qk_program_text("unknown gate op code %d at position %d (valid: 0..%d%s%s)", (int)p.op[i], i, n_codes - 1, with_k1 ? ", 10" : "", with_k2 ? ", 11" : "");
      return QK_PROGRAM_UNKNOWN_OP;
    }
  const auto bad = [&](const std::string& text) {
    *what = text;
    return QK_PROGRAM_BAD_TABLE;
  };
  for (int i = 0; i < n_ops; ++i)
    if ((p.op[i] == OP_M1 || p.op[i] == OP_M2) && (p.q0[i] < 0 || p.q0[i] + (p.op[i] == OP_M2 ? 1 : 0) >= p.n_qubits)) {
      *what = qk_program_text("gate %d on a qubit outside the register", i);
      return QK_PROGRAM_MATRIX_GATE_OUTSIDE;
    }
  const int tables = p.mats_state_stride ? p.n_states : 1;
  std::vector<char> seen((size_t)n_mats, 0);  // bit 0: checked as a 2x2, bit 1: as a 4x4 -- an entry many gates read is checked once
  for (int i = 0; i < n_ops; ++i) {
    if (p.op[i] != OP_M1 && p.op[i] != OP_M2) continue;
    const int k = p.mat[i], d = p.op[i] == OP_M1 ? 2 : 4;
    if (k < 0 || k >= n_mats) return bad(qk_program_text("gate %d: matrix index %d outside 0..%d", i, k, n_mats - 1));
    if (seen[(size_t)k] & (d == 2 ? 1 : 2)) continue;
    seen[(size_t)k] |= (d == 2 ? 1 : 2);
    for (int s = 0; s < tables; ++s) {
      const double* m = p.mats + ((size_t)s * n_mats + k) * 32;  // [4][4][2]
      bool finite = true;
      for (int a = 0; a < d; ++a)
        for (int b = 0; b < 2 * d; ++b) finite = finite && std::isfinite(m[a * 8 + b]);
      if (!finite) return bad(qk_program_text("gate %d: the matrix of table entry %d (state %d) has an entry that is not finite", i, k, s));
      const double dev = qk_program_gram_deviation(m, 1, d, 4);
      if (!(dev <= 1e-12)) return bad(qk_program_text("gate %d: the matrix of table entry %d (state %d) is not unitary: max |M^H M - 1| = %.3e > 1e-12", i, k, s, dev));
    }
  }
  if (!with_k1 && !with_k2) return QK_PROGRAM_OK;
  const int rows = p.branch_state_stride ? p.n_states : 1;
  for (int i = 0; i < n_ops; ++i) {
    if (p.op[i] != OP_K1 && p.op[i] != OP_K2) continue;
    const bool two = p.op[i] == OP_K2;
    const int d = two ? 4 : 2, n_table = two ? p.n_channels2 : p.n_channels;  // d x d matrices, at most d * d of them
    const char* kind = two ? "two-qubit channel" : "channel";
    const int ch = p.channel[i];
    if (ch < 0 || ch >= n_table) return bad(qk_program_text("gate %d: %s index %d outside 0..%d", i, kind, ch, n_table - 1));
    const int m = (two ? p.n_kraus2 : p.n_kraus)[ch];
    if (m < 1 || m > d * d) return bad(qk_program_text("gate %d: %s %d has %d Kraus matrices (1..%d)", i, kind, ch, m, d * d));
    const double* K = (two ? p.kraus2 : p.kraus) + (size_t)ch * d * d * d * d * 2;  // [d * d][d][d][2]
    for (int e = 0; e < 2 * d * d * m; ++e)
      if (!std::isfinite(K[e])) return bad(qk_program_text("gate %d: a Kraus matrix of %s %d has an entry that is not finite", i, kind, ch));
    bool drawn = false;
    for (int s = 0; s < rows; ++s) {
      const int b = p.branch[(size_t)s * n_ops + i];
      if (b < -1 || b >= m) return bad(qk_program_text("gate %d: branch %d (row %d) outside -1..%d", i, b, s, m - 1));
      drawn = drawn || b < 0;
    }
    if (drawn) {
      const double dev = qk_program_gram_deviation(K, m, d, d);
      if (!(dev <= 1e-12)) return bad(qk_program_text("gate %d: the drawn %s %d is not trace preserving: max |sum K^H K - 1| = %.3e > 1e-12", i, kind, ch, dev));
    }
    if (p.q0[i] < 0 || p.q0[i] + (two ? 1 : 0) >= p.n_qubits) return bad(qk_program_text("gate %d: %s on a qubit outside the register", i, kind));
  }
  for (int i = 0; p.cond_gate && i < n_ops; ++i) {
    const int g = p.cond_gate[i];
    if (g == -1) continue;
    if (g < -1 || g >= i) return bad(qk_program_text("gate %d: condition on gate %d outside -1..%d", i, g, i - 1));
    if (p.op[g] != OP_K1 && p.op[g] != OP_K2) return bad(qk_program_text("gate %d: condition on gate %d, which is no channel gate (op code %d)", i, g, (int)p.op[g]));
    const int m = (p.op[g] == OP_K2 ? p.n_kraus2 : p.n_kraus)[p.channel[g]];
    if (m < 32 && (p.cond_mask[i] >> m) != 0u) return bad(qk_program_text("gate %d: condition mask names a branch at or above the %d of gate %d", i, m, g));
  }
  return QK_PROGRAM_OK;
}
#endif  // QK_PROGRAM_H
