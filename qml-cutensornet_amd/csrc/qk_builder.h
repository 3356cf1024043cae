/* qk_builder.h -- the C ABI of libqkbuilder.so, the native host MPS builder (qk_builder.cpp).  The library is internal: mps.py
 * (through the ctypes mirror in program.py) and the tests call it.                                                              */
#ifndef QK_BUILDER_H
#define QK_BUILDER_H
#include "../../include/qkgram.h"

#ifdef __cplusplus
extern "C" {
#endif
/* How to run a program on the host.  max_bond > 0: at most that many singular values survive a gate (the chi of pytket-cutensornet's
 * Config, reference gpu_backend/kernel_state_ansatz.py:141-144); the lost weight goes into the fidelity like any other truncation.
 * init_dims not NULL: init_dims [n_qubits + 1] and init_tensors (the sites [l][2][r] complex128 row-major, back to back) replace
 * |0...0>; the state is taken as it stands -- canonical with its orthogonality centre on init_centre -- and the run begins with
 * init_fidelity and init_logw.                                                                                                   */
typedef struct qkb_run {
  uint32_t size; /* sizeof(qkb_run) */
  int32_t max_bond;
  double trunc_budget;
  double value_of_zero;
  const int32_t* init_dims;
  const double* init_tensors;
  int32_t init_centre;
  double init_fidelity;
  double init_logw;
} qkb_run;
/* What comes back.  dims and branches are the caller's buffers; the rest is filled in on success. */
typedef struct qkb_result {
  uint32_t size;     /* sizeof(qkb_result) */
  int32_t* dims;     /* [n_qubits + 1] */
  int8_t* branches;  /* [gates of codes 10 and 11, in program order] the branch taken, -2: skipped by its condition; may be NULL */
  double* tensors;   /* ONE malloc'd block holding the site tensors back to back, complex128 [l][2][r] row-major: free it with qkb_free */
  int64_t n_complex; /* complex elements of the block */
  double fidelity;
  double logw;       /* the initial log-weight plus log(p_b / N) of every channel gate that ran */
  double margin;     /* the smallest |u tot - cum| / tot over the thresholds of all draws, inf without one */
} qkb_result;

const char* qkb_last_error(void);
int qkb_init(const char* openblas_path); /* resolves LAPACK / BLAS from the OpenBLAS that scipy ships; 0 on success */
uint32_t qkb_program_size(void);         /* sizeof(qk_program), sizeof(qkb_run) and sizeof(qkb_result) of this library */
uint32_t qkb_run_size(void);
uint32_t qkb_result_size(void);
/* The MPS of the program (qk_program of include/qkgram.h with n_states = 1: one row of angles, one table, one branch row, one
 * state_index and trajectory) applied to |0...0> or to the initial state: the algorithm of mps.py:_simulate, the channel and
 * condition steps as the fields of qk_program describe them (sums in ascending order of elements and of k).  0, or a negative code
 * with qkb_last_error(): -1 qkb_init has not been called; -3 a gate outside the register; -4, -5 LAPACK; -6 out of memory; -7 an op
 * code outside the program's vocabulary; -8 before a gate is applied: a struct of another size (both sizes named), a null argument,
 * a bad table or condition row (csrc/qk_program.h), an initial state whose bond table does not chain (dims[0] != 1, dims[n] != 1,
 * an entry that is not positive), whose centre lies outside the register or which holds an entry (tensor, fidelity, log-weight) that
 * is not finite; -9 when the probability of the branch is 0 or not finite or the probabilities sum to 0 in a draw, naming the state
 * and the gate.                                                                                                                  */
int qkb_simulate_program(const qk_program* program, const qkb_run* run, qkb_result* result);
void qkb_free(double* p);
#ifdef __cplusplus
}
#endif
#endif /* QK_BUILDER_H */
