/*
 * dlsa_hip_binary.h -- family extension header of libdlsa_hip.so: the probit and complementary log-log map steps for a 0/1 response.
 *
 * The entries below live in the same library and follow every convention of dlsa_hip.h (device pointers unless marked host,
 * row-major matrices with leading dimensions in elements, a caller-owned 256-byte aligned workspace of exactly the query's
 * bytes, all device work on `stream`, 0 = DLSA_OK and dlsa_last_error() otherwise).  They are declared apart from dlsa_hip.h and
 * bound by a table of their own (dlsa_amd/_lib.py: BINARY_SIGNATURES); tests/test_binary_contract_cpu.py holds them to the same
 * workspace and stream contracts as the entries of dlsa_hip.h.
 */
#ifndef DLSA_HIP_BINARY_H
#define DLSA_HIP_BINARY_H

#include "dlsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Probit and complementary log-log (cloglog) regression map steps: the two binary links beside the logit --------------------
 * probit: P(y = 1) = Phi(eta) (bio-assay, econometrics, latent-Gaussian models).  cloglog: P(y = 1) = 1 - exp(-e^eta), the
 * grouped-time proportional-hazards model: with offset = log(interval length or exposure) it is the model of "any event in the
 * period", and the only binary link under which an exposure offset means what it means in dlsa_poisson_*.
 * The six entries take, argument for argument, what dlsa_poisson_workspace_bytes / dlsa_poisson_pass_f64 / dlsa_poisson_fit_f64
 * take: y holds 0.0 or 1.0 per row, `offset` (n, nullable) enters eta as is, `intercept` != 0 puts an implicit ones column first
 * (pe = p + 1 entries, intercept first; pe = p otherwise), p >= 1 and pe <= 2048 (the solver's limit); anything else is
 * DLSA_ERR_INVALID.  eta = [1 | x]' beta + o.
 * Per row, l = the log-likelihood term, r = dl / deta, w = -d2l / deta2:
 *   probit:   s = 2y - 1, z = s eta, lambda = phi(z) / Phi(z):   l = log Phi(z),  r = s lambda,  w = lambda (z + lambda)
 *   cloglog:  mu = e^eta;   y = 0: l = -mu, r = -mu, w = mu (exactly the row of dlsa_poisson_pass_f64 with y = 0);
 *                           y = 1: l = log(1 - e^-mu),  r = mu / (e^mu - 1),  w = r (mu + r - 1)
 * w is the OBSERVED information (both log-likelihoods are concave, so w >= 0 on every row and H is positive semidefinite).  It is
 * NOT the Fisher (expected) information that R's glm reports as its working weights: under these two non-canonical links the two
 * differ row by row away from the expectation over y (under the logit and the log link of dlsa_poisson_* they coincide).  Sig_inv is
 * therefore the observed information at the MLE; both are consistent for the same matrix.  The terms are evaluated in forms that do
 * not cancel anywhere in the range of eta (dlsa_amd/csrc/binary_terms.h); no finite eta gives a NaN: a cloglog row with mu = inf has
 * l = r = w = 0 for y = 1 and l = -inf for y = 0, a probit row with |z| beyond 1e154 has l = -inf for z < 0.
 * dlsa_{probit,cloglog}_pass_f64 at a fixed beta, one read of the rows (+ ONE Gram when H is wanted): loglik = sum l (1 value,
 * nullable; there is no constant term), g = [1 | X]'r (pe, nullable), H = [1 | X]' diag(w) [1 | X] (nullable, ldh >= pe, both
 * triangles, bitwise symmetric; columns pe .. ldh - 1 are not touched), w_out (n, nullable) = w.  The pass does not check its data;
 * loglik is NaN when a response is not exactly 0 or 1 or an offset is not finite.  g and loglik are bit-reproducible.
 * dlsa_{probit,cloglog}_fit_f64: partitions as dlsa_poisson_fit_f64 (partition k = rows part_first_host[k] + j row_step, j <
 * part_rows_host[k]; strided partitions are read in place, their responses and offsets gathered into the workspace).  The data of a
 * partition are checked once, before it is fitted: a response that is not exactly 0 or 1, or a non-finite offset, returns
 * DLSA_ERR_INVALID naming the partition, and no output is written.  Newton from beta = 0 with the intercept at the link of the
 * response share ybar (Phi^-1(ybar), respectively log(-log(1 - ybar))) less the log of the mean e^o, with the safeguards and the
 * stopping rule of dlsa_poisson_fit_f64 (an iterate whose loglik is -inf or lower than the last is halved back); outputs as
 * dlsa_poisson_fit_f64: Sig_inv = H at coef, loglik_host the log-likelihood at coef.  A partition WITH an intercept whose responses
 * are all 0 or all 1 has its MLE at eta -> -+inf, where H -> 0: it is DLSA_PART_EMPTY with the all-zero block, as is a partition
 * without rows.  WITHOUT an intercept such a partition can have a finite MLE: the loop runs and reports what it finds.
 * DLSA_PART_NOT_SPD, DLSA_PART_NOT_CONVERGED and DLSA_PART_NAN as dlsa_poisson_fit_f64.
 * Workspace: dlsa_{probit,cloglog}_workspace_bytes(max rows, p, intercept, row_step) (0 for a shape the entries refuse); the pass
 * takes the same query with row_step = 1.  Arguments are judged before any HIP call. */
size_t dlsa_probit_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step);
int dlsa_probit_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, int64_t n, int p,
                         int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out,
                         void* ws, size_t ws_bytes, void* stream);
int dlsa_probit_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                        const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double tol, int max_iter,
                        double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                        double* loglik_host, void* ws, size_t ws_bytes, void* stream);
size_t dlsa_cloglog_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step);
int dlsa_cloglog_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, int64_t n, int p,
                          int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out,
                          void* ws, size_t ws_bytes, void* stream);
int dlsa_cloglog_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double tol, int max_iter,
                         double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                         double* loglik_host, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DLSA_HIP_BINARY_H */
