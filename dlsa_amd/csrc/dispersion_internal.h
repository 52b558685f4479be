// The families with a log link and a scalar dispersion phi that enters after a fit at phi = 1 (Gamma: gamma.hip, Tweedie:
// tweedie.hip; their structured one-hot forms: onehot_gamma.hip, onehot_tweedie.hip): beta^ does not depend on phi, so the row pass
// and the Newton loop run at nu = 1 / phi = 1 and the dispersion is one scalar on H, g and loglik afterwards.  One driver
// (dispersion.hip) holds the pass epilogue, the per-partition fit, the workspace layouts and the bodies of the eight C entries;
// a family is the record below, defined next to the kernels it launches (the library is built without relocatable device code,
// so a kernel and its launcher stay in one translation unit), and a row pass is a callable of the unit that instantiates it.
#pragma once
#include "common.h"
#include "block_sums.h"
#include "poisson_internal.h"
#include <functional>

namespace dlsa {

constexpr int DISP_SUM_BLOCKS = 1024;
// the dispersion sums over (y, mu): [the Pearson sum, the deviance]
constexpr int DISP_ND = 2;
enum { DISP_PEARSON = 0, DISP_DEV = 1 };

// the blocks of a per-block sum kernel over n rows: at most DISP_SUM_BLOCKS workgroups of 256 threads
int disp_sum_blocks(int64_t n);
// H (pe x pe, pitch ldh; nullable) and g (pe; nullable) times nu: the unit-dispersion quantities taken to dispersion 1 / nu
int disp_scale(double* H, int64_t ldh, int pe, double* g, double nu, hipStream_t s);

struct DispFamily {
    int nc;                  // the once-per-partition sums (<= 4): cpart holds nc * DISP_SUM_BLOCKS doubles
    double power;            // Tweedie's variance power xi (Gamma: unused)
    const char* bad_param;   // null, or why the family's own parameter is refused (the entries report it after the shape checks)
    // cst[0..nc) = the once-per-partition sums of n rows (off nullable), among them the count of invalid rows
    int (*const_sums)(const DispFamily& f, const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s);
    // dst[0..1] = [P, Dev] of n rows; dpart: DISP_ND * DISP_SUM_BLOCKS doubles of scratch.  Fixed-order: bit-reproducible
    int (*disp_sums)(const DispFamily& f, const double* y, const double* mu, int64_t n, double* dpart, double* dst, hipStream_t s);
    // the fit's data check on the host copy of cst: DLSA_OK, or the refusal of partition k with its message set
    int (*check)(const char* who, int k, const double* cst);
    // the mean of the intercept-only model (the intercept starts at its log)
    double (*start_mean)(const double* cst, int64_t n);
    // the fit's log-likelihood at nu from ll, the row sum at unit dispersion
    double (*loglik)(double nu, double ll, const double* cst, int64_t n);
    // the same on the device for the pass entry: ll[0] in place from the device cst (NaN when a row is not a valid response)
    int (*ll_fix)(double* ll, const double* cst, double nu, int64_t n, hipStream_t s);
};
constexpr int GAMMA_NC = 3, TWEEDIE_NC = 4;  // the two families' nc: what their workspace queries size cpart with
DispFamily gamma_family();                   // gamma.hip
DispFamily tweedie_family(double power);     // tweedie.hip

// The row pass of one partition at a fixed beta and unit dispersion, as the unit that instantiates the kernel binds it: H
// (nullable) needs w (the Gram's weights); g, loglik (the row sum of the family's term) and mu nullable.
// dense: count_pass (count_pass.h) after its row model
template <class T> struct CountScratchOf;   // count_pass.h
using DispDenseRows = std::function<int(const double* X, int64_t ldx, const double* y, const double* off, const double* beta, int64_t n,
                                        int p, int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w, double* mu,
                                        const CountScratchOf<double*>& sc, void* gws, size_t gws_bytes, hipStream_t s)>;
// structured: oh_row_pass (onehot_pass.h) with the family's row model, then onehot_gram_impl(..., false) when H is wanted; ws_oh
// is the structured passes' arena (256-aligned, >= onehot_workspace_bytes_impl(pl, n))
using DispOnehotRows = std::function<int(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                         const double* y, const double* off, const double* beta, int64_t n, double* H, int64_t ldh,
                                         double* g, double* loglik, double* w, double* mu, void* ws_oh, size_t ws_oh_bytes, hipStream_t s)>;

// ---- the bodies of the C entries (`who` prefixes messages: "gamma_pass", "onehot_tweedie_fit", ...) -------------------------
size_t disp_workspace_bytes(int nc, int64_t max_rows, int p, int intercept, int64_t row_step);
size_t disp_onehot_workspace_bytes(int nc, const dlsa_onehot_plan* plan, int64_t max_rows, int64_t row_step);

// One partition at beta and `dispersion`: the row pass, then [P, Dev] into stats_out, H and g times nu = 1 / dispersion, loglik
// the family's log-likelihood at that dispersion.  H, g, loglik, w_out, stats_out nullable.
int disp_pass_entry(const char* who, const DispFamily& f, const DispDenseRows& rows, const double* X, int64_t ldx, const double* y,
                    const double* offset, const double* beta, double dispersion, int64_t n, int p, int intercept, double* H, int64_t ldh,
                    double* g, double* loglik, double* w_out, double* stats_out, void* ws, size_t ws_bytes, void* stream);
int disp_onehot_pass_entry(const char* who, const DispFamily& f, const DispOnehotRows& rows, const dlsa_onehot_plan* plan,
                           const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y, const double* offset,
                           const double* beta, double dispersion, int64_t n, double* H, int64_t ldh, double* g, double* loglik,
                           double* w_out, double* stats_out, void* ws, size_t ws_bytes, void* stream);

// The per-partition fit: the refusal of a partition without degrees of freedom (estimated dispersion, 0 < n <= pe), the family's
// data check and sums, start at beta = 0 with the intercept at log(start_mean), newton_fit_loop with the policy NEWTON_POISSON at
// unit dispersion (the iteration does not depend on it), then the dispersion from the mu of the evaluation that left H,
// Sig_inv = H / dispersion, the family's loglik, and newton_fit_finish.  dispersion_fixed > 0: every block uses it.
int disp_fit_entry(const char* who, const DispFamily& f, const DispDenseRows& rows, const double* X, int64_t ldx, const double* y,
                   const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step, int K, int p,
                   int intercept, double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv,
                   double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host,
                   double* pearson_host, double* deviance_host, void* ws, size_t ws_bytes, void* stream);
int disp_onehot_fit_entry(const char* who, const DispFamily& f, const DispOnehotRows& rows, const dlsa_onehot_plan* plan,
                          const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y, const double* offset,
                          const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step, int K,
                          double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                          int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host,
                          double* deviance_host, void* ws, size_t ws_bytes, void* stream);

}  // namespace dlsa
