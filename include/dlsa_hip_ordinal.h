/*
 * dlsa_hip_ordinal.h -- family extension header of libdlsa_hip.so: the ordinal (proportional-odds) map step.
 *
 * The entries below live in the same library and follow every convention of dlsa_hip.h (device pointers unless marked host,
 * row-major matrices with leading dimensions in elements, a caller-owned 256-byte aligned workspace of exactly the query's
 * bytes, all device work on `stream`, 0 = DLSA_OK and dlsa_last_error() otherwise).  They are declared apart from dlsa_hip.h and
 * bound by a table of their own (dlsa_amd/_lib.py: ORDINAL_SIGNATURES); tests/test_ordinal_contract_cpu.py holds them to the same
 * workspace and stream contracts as the entries of dlsa_hip.h.
 */
#ifndef DLSA_HIP_ORDINAL_H
#define DLSA_HIP_ORDINAL_H

#include "dlsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Ordinal (proportional-odds, cumulative logit) regression map step (a response with C ordered classes: delay bucket,
 * credit grade, severity score) ---------
 * y holds the class codes 0 .. C - 1 as doubles; C = `classes` is given by the caller, 2 <= C <= 8, J = C - 1, p >= 1 and
 * d = J + p <= 2048 (the solver's limit); anything else is DLSA_ERR_INVALID.  logit P(y <= j) = alpha_{j+1} - x'beta, j = 0 ..
 * J - 1 (the sign convention of MASS::polr and statsmodels OrderedModel: a positive beta moves mass to the higher classes).  The
 * parameter is theta = [alpha_1 .. alpha_J | beta_1 .. beta_p], cutpoints first.  There is no intercept argument: the cutpoints are
 * the intercepts, and a design with a constant column is singular (DLSA_PART_NOT_SPD).  g, coef and Sig_invMcoef have d entries, H
 * and Sig_inv are d x d with both triangles, bitwise symmetric.  No offsets, no dispersion.  C = 2 is the logistic model with
 * theta = [-intercept | beta].
 * For a row of class c with eta = x'beta, u = alpha_{c+1} - eta, l = alpha_c - eta and F the logistic cdf: A = F(u), Abar = F(-u),
 * B = F(l), Bbar = F(-l) (the top class has A = 1, Abar = 0, class 0 has B = 0, Bbar = 1), E_c = -expm1(-(alpha_{c+1} - alpha_c))
 * for an interior class and 1 for the two end classes.  Then P(y = c) = A Bbar E, r = A + B - 1, w = A Abar + B Bbar >= 0,
 * s_u = Abar / (Bbar E), s_l = B / (A E), q = s_u s_l.
 * dlsa_ordinal_pass_f64 at a fixed theta, one read of the rows (+ ONE Gram when H is wanted; + one read per cutpoint where C times
 * the 128-column chunks of p, rounded up to a power of two, exceeds 16): loglik = sum_i log P(y_i) (1 value, nullable; NaN when
 * the cutpoints are not strictly increasing or a response is not finite, not integral, < 0 or >= C), g (nullable) with g_beta =
 * X'r and g_alpha_j = sum_{y = j-1} s_u - sum_{y = j} s_l, H (nullable, ldh >= d; columns d .. ldh - 1 are not touched) = the
 * observed information, positive semidefinite: H_bb = X' diag(w) X, H_{alpha_j, beta} = X'v_j with v_j = -(1[y = j-1] A Abar +
 * 1[y = j] B Bbar), H_{alpha_j alpha_j} = sum_{y = j-1} (A Abar + q) + sum_{y = j} (B Bbar + q), H_{alpha_j alpha_j+1} =
 * -sum_{y = j} q, zero elsewhere among the cutpoints; w_out (n, nullable) = w.  A class without rows is legal in a pass; the data
 * of the pass are not checked otherwise.  g and loglik are bit-reproducible.
 * dlsa_ordinal_fit_f64: partitions as dlsa_poisson_fit_f64 (strided i % K partitions read in place, their responses gathered into
 * the workspace).  Before any partition is fitted, every partition with rows is checked: a response that is no class code, or a
 * class 0 .. C - 1 without a row (two cutpoints of that fit merge or run off, and the blocks of different partitions must mean
 * the same parameter), returns DLSA_ERR_INVALID naming the partition (and the class), with no output written.  Newton from beta = 0
 * with alpha_j at the logit of the cumulative class share (the exact MLE of the null model), the safeguards and the stopping rule
 * of dlsa_poisson_fit_f64 (an iterate whose cutpoints cross has loglik NaN and is halved back); outputs as dlsa_poisson_fit_f64 on
 * d coefficients, Sig_inv = H at coef, loglik_host the log-likelihood at coef.  A partition without rows is DLSA_PART_EMPTY with
 * the all-zero block; DLSA_PART_NOT_SPD, DLSA_PART_NOT_CONVERGED and DLSA_PART_NAN as dlsa_poisson_fit_f64.
 * Workspace: dlsa_ordinal_workspace_bytes(max rows, p, classes, row_step) (0 for a shape the entries refuse); the pass takes the
 * same query with row_step = 1.  Arguments are judged before any HIP call. */
size_t dlsa_ordinal_workspace_bytes(int64_t max_rows, int p, int classes, int64_t row_step);
int dlsa_ordinal_pass_f64(const double* X, int64_t ldx, const double* y, const double* theta, int classes, int64_t n, int p,
                          double* H, int64_t ldh, double* g, double* loglik, double* w_out,
                          void* ws, size_t ws_bytes, void* stream);
int dlsa_ordinal_fit_f64(const double* X, int64_t ldx, const double* y, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int p, int classes, double tol, int max_iter,
                         double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                         double* loglik_host, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DLSA_HIP_ORDINAL_H */
