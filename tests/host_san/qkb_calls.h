// The calls the host_san drivers make into the native host MPS builder, spelt with the arguments the drivers hold: each fills a
// qk_program, a qkb_run and a qkb_result and goes through qkb_simulate_program (csrc/qk_builder.h), the one entry of the library.
// Test infrastructure: nothing of the product includes it.
#ifndef QKB_CALLS_H
#define QKB_CALLS_H
#include "../../qml-cutensornet_amd/csrc/qk_builder.h"

// every field a driver can set; a table with count 0 is absent, init_dims null starts from |0...0>, the last three may be null
static inline int qkb_simulate_initial(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                                       int32_t max_bond, int32_t n_mats, const double* mats, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                                       const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate,
                                       int32_t n_channels2, const double* kraus2, const int32_t* n_kraus2, const int32_t* cond_gate, const uint32_t* cond_mask, const int32_t* init_dims,
                                       const double* init_tensors, int32_t init_centre, double init_fidelity, double init_logw, int32_t* dims_out, double** tensors_out,
                                       int64_t* n_complex_out, double* fidelity_out, double* logw_out, int8_t* branches_out, double* margin_out) {
  qk_program p = {};
  p.size = sizeof p, p.n_states = 1, p.n_qubits = n_qubits, p.n_ops = n_ops, p.op = op, p.q0 = q0, p.alpha = alpha;
  p.n_mats = n_mats, p.mats = mats, p.mat = mat;
  p.n_channels = n_channels, p.kraus = kraus, p.n_kraus = n_kraus, p.n_channels2 = n_channels2, p.kraus2 = kraus2, p.n_kraus2 = n_kraus2;
  p.channel = channel, p.branch = branch, p.seed = seed, p.state_index = &state_index, p.trajectory = &trajectory, p.first_gate = first_gate;
  p.cond_gate = cond_gate, p.cond_mask = cond_mask;
  qkb_run r = {};
  r.size = sizeof r, r.max_bond = max_bond, r.trunc_budget = trunc_budget, r.value_of_zero = value_of_zero;
  r.init_dims = init_dims, r.init_tensors = init_tensors, r.init_centre = init_centre, r.init_fidelity = init_fidelity, r.init_logw = init_logw;
  qkb_result out = {};
  out.size = sizeof out, out.dims = dims_out, out.branches = branches_out;
  const int rc = qkb_simulate_program(&p, &r, &out);
  if (rc != 0) return rc;
  *tensors_out = out.tensors, *n_complex_out = out.n_complex, *fidelity_out = out.fidelity;
  if (logw_out) *logw_out = out.logw;
  if (margin_out) *margin_out = out.margin;
  return 0;
}

static inline int qkb_simulate_conditions(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                                          int32_t max_bond, int32_t n_mats, const double* mats, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                                          const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate,
                                          int32_t n_channels2, const double* kraus2, const int32_t* n_kraus2, const int32_t* cond_gate, const uint32_t* cond_mask, int32_t* dims_out,
                                          double** tensors_out, int64_t* n_complex_out, double* fidelity_out, double* logw_out, int8_t* branches_out, double* margin_out) {
  return qkb_simulate_initial(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats, mat, n_channels, kraus, n_kraus, channel, branch, seed, state_index,
                              trajectory, first_gate, n_channels2, kraus2, n_kraus2, cond_gate, cond_mask, nullptr, nullptr, 0, 1.0, 0.0, dims_out, tensors_out, n_complex_out,
                              fidelity_out, logw_out, branches_out, margin_out);
}

static inline int qkb_simulate_channels2(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                                         int32_t max_bond, int32_t n_mats, const double* mats, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                                         const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate,
                                         int32_t n_channels2, const double* kraus2, const int32_t* n_kraus2, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out,
                                         double* fidelity_out, double* logw_out, int8_t* branches_out, double* margin_out) {
  return qkb_simulate_conditions(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats, mat, n_channels, kraus, n_kraus, channel, branch, seed,
                                 state_index, trajectory, first_gate, n_channels2, kraus2, n_kraus2, nullptr, nullptr, dims_out, tensors_out, n_complex_out, fidelity_out, logw_out,
                                 branches_out, margin_out);
}

static inline int qkb_simulate_channels(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                                        int32_t max_bond, int32_t n_mats, const double* mats, const int32_t* mat, int32_t n_channels, const double* kraus, const int32_t* n_kraus,
                                        const int32_t* channel, const int32_t* branch, uint64_t seed, uint32_t state_index, uint32_t trajectory, uint32_t first_gate,
                                        int32_t* dims_out, double** tensors_out, int64_t* n_complex_out, double* fidelity_out, double* logw_out, int8_t* branches_out,
                                        double* margin_out) {
  return qkb_simulate_channels2(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats, mat, n_channels, kraus, n_kraus, channel, branch, seed, state_index,
                                trajectory, first_gate, 0, nullptr, nullptr, dims_out, tensors_out, n_complex_out, fidelity_out, logw_out, branches_out, margin_out);
}

static inline int qkb_simulate_gates(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                                     int32_t max_bond, int32_t n_mats, const double* mats, const int32_t* mat, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out,
                                     double* fidelity_out) {
  return qkb_simulate_channels(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, n_mats, mats, mat, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, dims_out,
                               tensors_out, n_complex_out, fidelity_out, nullptr, nullptr, nullptr);
}

static inline int qkb_simulate_chi(int32_t n_qubits, int32_t n_ops, const int8_t* op, const int32_t* q0, const double* alpha, double trunc_budget, double value_of_zero,
                                   int32_t max_bond, int32_t* dims_out, double** tensors_out, int64_t* n_complex_out, double* fidelity_out) {
  return qkb_simulate_gates(n_qubits, n_ops, op, q0, alpha, trunc_budget, value_of_zero, max_bond, 0, nullptr, nullptr, dims_out, tensors_out, n_complex_out, fidelity_out);
}
#endif  // QKB_CALLS_H
