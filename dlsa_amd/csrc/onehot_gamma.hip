// Structured Gamma map step for one-hot designs: the Gamma pass and fit of gamma.hip on the RAW representation of a design
// [intercept | standardised numerics | one-hot factor levels] (num [n, q] fp64, codes [n, f] int32) under a dlsa_onehot_plan --
// the dense n x p matrix is never built.  Results equal the dense Gamma entries on the matrix dlsa_design_f64 would build (to
// rounding).
//
// Launches per evaluation at a fixed beta (unit dispersion; the dispersion is one scalar on H and g afterwards):
//   1 oh_row_kernel<OhGammaRow<OFF>>  the one-thread-per-row pass of onehot_pass.h (shared with the logistic, Poisson and NB2
//                           models) with the Gamma terms: eta = d . beta_D + sum_t beta[col(t, code_t)] + o (a gather),
//                           mu = exp_full(eta) (-> the dispersion sums), r = y / mu (-> w), residual r - 1, per-workgroup partials of
//                           g (dense part in registers, level part an LDS histogram with replicated copies and wave turn-taking:
//                           a fixed order of the adds, bit-reproducible) and of sum -(r + eta);
//   2 logit_finish_launch   the fixed-order column sums of those partials (logit.hip, shared);
//   3 the Gram              onehot_gram_impl(plan, num, codes, r) with irls_weights = false: r is unbounded, so the ordered
//                           floating-point mode, never the fixed-point one.
// Traffic per row: 8q + 4f + 8 (y) + 8 (o) + 16 (r, mu written) bytes for the pass, 8q + 4f + 8 for the Gram.
// The once-per-partition sums and the dispersion sums over (y, mu) are gamma.hip's, reached through its family record; the
// entries' bodies, the workspace, the scaling and the fit driver are the dispersion driver's (dispersion.hip,
// dispersion_internal.h); the row checks of num / codes and the plan's constant column are onehot_poisson.hip's.
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include "dispersion_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "poisson_exp.h"  // exp_full
#include "onehot_pass.h"  // oh_row_kernel, oh_row_pass

template <bool OFF>       // OFF = false reads no offsets
struct OhGammaRow {       // eta += o, mu = exp(eta), r = y / mu = w (kept from resid), residual r - 1, term -(r + eta)
    static constexpr bool STORES_MU = true;
    const double* off;
    double r;             // of the row in hand
    __device__ __forceinline__ double mean(int64_t i, double& eta) const {
        if constexpr (OFF) eta += off[i];
        return exp_full(eta);
    }
    __device__ __forceinline__ double resid(double y, double, double mu) {
        r = y / mu;
        return r - 1.0;
    }
    __device__ __forceinline__ double weight(double) const { return r; }
    __device__ __forceinline__ double term(double, double eta, double) const { return -(r + eta); }
};

// ---- host side ---------------------------------------------------------------------------------------------------------
// the structured row pass of the dispersion driver (dispersion_internal.h): w is r per row, loglik the sum of -(r + eta)
static int oh_gamma_rows(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y,
                         const double* off, const double* beta, int64_t n, double* H, int64_t ldh, double* g, double* loglik, double* w,
                         double* mu, void* ws_oh, size_t ws_oh_bytes, hipStream_t s) {
    const char* who = "onehot gamma pass";
    const int rc = off ? oh_row_pass(who, OhGammaRow<true>{off, 0.0}, pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s)
                       : oh_row_pass(who, OhGammaRow<false>{off, 0.0}, pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s);
    if (rc || !H) return rc;
    // (the Gram's partials overwrite the pass's in the same arena: the finish launch above has consumed them, in stream order)
    return onehot_gram_impl(pl, num, ldn, codes, ldc, w, n, H, ldh, ws_oh, ws_oh_bytes, s, false);
}

}  // namespace dlsa

extern "C" {

size_t dlsa_onehot_gamma_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int64_t row_step) {
    return dlsa::disp_onehot_workspace_bytes(dlsa::GAMMA_NC, plan, max_rows, row_step);
}

int dlsa_onehot_gamma_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                               const double* y, const double* offset, const double* beta, double dispersion, int64_t n, double* H,
                               int64_t ldh, double* g, double* loglik, double* w_out, double* stats_out, void* ws, size_t ws_bytes,
                               void* stream) {
    return dlsa::disp_onehot_pass_entry("onehot_gamma_pass", dlsa::gamma_family(), dlsa::oh_gamma_rows, plan, num, ldn, codes, ldc, y,
                                        offset, beta, dispersion, n, H, ldh, g, loglik, w_out, stats_out, ws, ws_bytes, stream);
}

int dlsa_onehot_gamma_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                              const double* y, const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host,
                              int64_t row_step, int K, double dispersion_fixed, double tol, int max_iter, double* coef,
                              double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                              double* dispersion_host, double* pearson_host, double* deviance_host, void* ws, size_t ws_bytes,
                              void* stream) {
    return dlsa::disp_onehot_fit_entry("onehot_gamma_fit", dlsa::gamma_family(), dlsa::oh_gamma_rows, plan, num, ldn, codes, ldc, y,
                                       offset, part_first_host, part_rows_host, row_step, K, dispersion_fixed, tol, max_iter, coef,
                                       Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, dispersion_host, pearson_host,
                                       deviance_host, ws, ws_bytes, stream);
}

}  // extern "C"
