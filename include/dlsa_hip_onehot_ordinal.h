/*
 * dlsa_hip_onehot_ordinal.h -- family extension header of libdlsa_hip.so: the structured one-hot sibling of the ordinal
 * (proportional-odds) map step.
 *
 * The entries below live in the same library and follow every convention of dlsa_hip.h and dlsa_hip_ordinal.h (device pointers
 * unless marked host, row-major matrices with leading dimensions in elements, a caller-owned 256-byte aligned workspace of exactly
 * the query's bytes, all device work on `stream`, 0 = DLSA_OK and dlsa_last_error() otherwise).  They are declared apart from both
 * and bound by a table of their own (dlsa_amd/_lib.py: ONEHOT_ORDINAL_SIGNATURES); tests/test_onehot_ordinal_contract_cpu.py holds
 * them to the same workspace and stream contracts as the entries of dlsa_hip.h.
 */
#ifndef DLSA_HIP_ONEHOT_ORDINAL_H
#define DLSA_HIP_ONEHOT_ORDINAL_H

#include "dlsa_hip_ordinal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Structured ordinal (proportional-odds) map step on the raw representation of a one-hot design ---------
 * The pass and fit of dlsa_hip_ordinal.h on num [n, q] fp64 (pitch ldn) and codes [n, f] int32 (pitch ldc) under a
 * dlsa_onehot_plan (dlsa_hip.h: dlsa_onehot_plan_create): the results equal dlsa_ordinal_pass_f64 / dlsa_ordinal_fit_f64 on the
 * n x p matrix dlsa_design_f64 would build, to rounding, and that matrix is never built.  Model, sign convention and layout are
 * those of dlsa_hip_ordinal.h with p = the plan's p: y holds the class codes 0 .. C - 1 as doubles, C = `classes`, 2 <= C <= 8,
 * J = C - 1, logit P(y <= j) = alpha_{j+1} - x'beta, theta = [alpha_1 .. alpha_J | beta] with beta in the plan's column order,
 * d = J + p <= 2048; g, coef and Sig_invMcoef have d entries, H and Sig_inv are d x d with both triangles, bitwise symmetric.  No
 * offsets.
 * THE PLAN MUST HAVE NO CONSTANT COLUMN: the cutpoints are the intercepts.  A plan with one is refused by the pass and by the fit
 * with DLSA_ERR_INVALID and a message that says so, and the query returns 0 for it.  A design that keeps every level of a factor
 * (no baseline) is collinear with the cutpoints: it is legal in a pass and gives DLSA_PART_NOT_SPD in a fit, as the dense fit does
 * for a constant column.  An unknown code (< 0, or >= the factor's levels) and a level without a column contribute nothing.
 * num may be null when the plan reads no numeric column, codes when it has no factor; otherwise ldn / ldc must cover what the plan
 * reads.  Null plan, y or theta, C outside 2 .. 8, d > 2048, n < 1 and ldh < d are DLSA_ERR_INVALID.
 * dlsa_onehot_ordinal_pass_f64 at a fixed theta, one read of the rows (+ ONE structured Gram when H is wanted; + one more read of
 * the rows per cutpoint where (p + J + C p) doubles exceed 32 KiB of LDS, the route without in-pass borders): loglik = sum_i log
 * P(y_i) (1 value, nullable; NaN when the cutpoints are not strictly increasing or a response is not finite, not integral, < 0 or
 * >= C), g (nullable), H (nullable, ldh >= d; columns d .. ldh - 1 are not touched) = the observed information as
 * dlsa_ordinal_pass_f64 defines it, w_out (n, nullable) = A Abar + B Bbar per row.  A class without rows is legal in a pass; the
 * data of the pass are not checked otherwise.  The pass never synchronises the stream.  By default g, loglik and H are
 * bit-reproducible (wave turn-taking in the row pass, the ordered Gram); dlsa_kernel_options.onehot_ordered = 0 gives unordered
 * adds whose last bits vary.
 * dlsa_onehot_ordinal_fit_f64: partition k is the rows part_first_host[k] + j row_step, j < part_rows_host[k], read in place from
 * num and codes with the pitches ldn row_step and ldc row_step; only the responses of a strided partition are gathered into the
 * workspace.  Before any partition is fitted, every partition with rows is checked: a response that is no class code, or a class
 * 0 .. C - 1 without a row, returns DLSA_ERR_INVALID naming the partition (and the class), with no output written.  Start, Newton
 * loop, safeguards, stopping rule, outputs and statuses are those of dlsa_ordinal_fit_f64: coef [K, d], Sig_inv [K, d, d] = H at
 * coef, Sig_invMcoef [K, d], n_iter_host / status_host / loglik_host [K] (host, nullable).  A partition without rows is
 * DLSA_PART_EMPTY with the all-zero block; DLSA_PART_NOT_SPD, DLSA_PART_NOT_CONVERGED and DLSA_PART_NAN as dlsa_poisson_fit_f64.
 * Workspace: dlsa_onehot_ordinal_workspace_bytes(plan, max rows, classes, row_step), 256-aligned and monotone in the rows; 0 for a
 * null plan, a plan with a constant column, C outside 2 .. 8, J + p > 2048, max_rows < 0 or row_step < 1.  The pass takes the same
 * query with row_step = 1.  Arguments are judged before any HIP call. */
size_t dlsa_onehot_ordinal_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int classes, int64_t row_step);
int dlsa_onehot_ordinal_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                 const double* y, const double* theta, int classes, int64_t n, double* H, int64_t ldh,
                                 double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes, void* stream);
int dlsa_onehot_ordinal_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                const double* y, const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step,
                                int K, int classes, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                                int* n_iter_host, int* status_host, double* loglik_host, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DLSA_HIP_ONEHOT_ORDINAL_H */
