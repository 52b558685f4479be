// Structured Tweedie map step for one-hot designs: the Tweedie pass and fit of tweedie.hip on the RAW representation of a design
// [intercept | standardised numerics | one-hot factor levels] (num [n, q] fp64, codes [n, f] int32) under a dlsa_onehot_plan --
// the dense n x p matrix is never built.  Results equal the dense Tweedie entries on the matrix dlsa_design_f64 would build (to
// rounding).  loglik is the quasi-log-likelihood of tweedie.hip: the series factor of the density is not computed.
//
// Launches per evaluation at a fixed beta (unit dispersion; the dispersion is one scalar on H, g and loglik afterwards):
//   1 oh_row_kernel<OhTweedieRow<OFF>>  the one-thread-per-row pass of onehot_pass.h (unchanged; shared with the logistic, Poisson,
//                           NB2 and Gamma models) with the Tweedie terms: eta = d . beta_D + sum_t beta[col(t, code_t)] + o (a
//                           gather), mu = exp_full(eta) (-> the dispersion sums), a = mu^(1 - xi) by the compensated product of
//                           tweedie.hip, b = mu a, weight (xi - 1) y a + (2 - xi) b (-> w), residual y a - b, per-workgroup
//                           partials of g (dense part in registers, level part an LDS histogram with replicated copies and wave
//                           turn-taking: a fixed order of the adds, bit-reproducible) and of sum q;
//   2 logit_finish_launch   the fixed-order column sums of those partials (logit.hip, shared);
//   3 the Gram              onehot_gram_impl(plan, num, codes, w) with irls_weights = false: the weight is unbounded, so the
//                           ordered floating-point mode, never the fixed-point one.
// Traffic per row: 8q + 4f + 8 (y) + 8 (o) + 16 (w, mu written) bytes for the pass, 8q + 4f + 8 for the Gram.
// The once-per-partition sums and the dispersion sums over (y, mu) are tweedie.hip's, reached through its family record, the
// row's arithmetic tweedie_internal.h's; the entries' bodies, the workspace, the scaling and the fit driver are the dispersion
// driver's (dispersion.hip, dispersion_internal.h); the row checks of num / codes and the plan's constant column are
// onehot_poisson.hip's.
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include "dispersion_internal.h"
#include "tweedie_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "poisson_exp.h"  // exp_full
#include "onehot_pass.h"  // oh_row_kernel, oh_row_pass

template <bool OFF>       // OFF = false reads no offsets
struct OhTweedieRow {     // eta += o, mu = exp(eta); resid keeps y a, b = mu^(2 - xi) and the weight of the row in hand
    static constexpr bool STORES_MU = true;
    const double* off;
    double one_m_xi, two_m_xi, inv_one, inv_two;      // 1 - xi, 2 - xi and their reciprocals
    double ya, b, w;
    __device__ __forceinline__ double mean(int64_t i, double& eta) const {
        if constexpr (OFF) eta += off[i];
        return exp_full(eta);
    }
    __device__ __forceinline__ double resid(double y, double eta, double mu) {
        tweedie_row(one_m_xi, two_m_xi, y, eta, mu, ya, b, w);
        return ya - b;
    }
    __device__ __forceinline__ double weight(double) const { return w; }
    __device__ __forceinline__ double term(double, double, double) const { return fma(ya, inv_one, -(b * inv_two)); }
};

template <bool OFF>
static OhTweedieRow<OFF> oh_tweedie_row(const double* off, double power) {
    const double c1 = 1.0 - power, c2 = 2.0 - power;
    return OhTweedieRow<OFF>{off, c1, c2, 1.0 / c1, 1.0 / c2, 0.0, 0.0, 0.0};
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the structured row pass of the dispersion driver (dispersion_internal.h) at `power`: w is the weight per row, loglik the sum of q
static DispOnehotRows oh_tweedie_rows(double power) {
    return [power](const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y,
                   const double* off, const double* beta, int64_t n, double* H, int64_t ldh, double* g, double* loglik, double* w,
                   double* mu, void* ws_oh, size_t ws_oh_bytes, hipStream_t s) {
        const char* who = "onehot tweedie pass";
        const int rc = off ? oh_row_pass(who, oh_tweedie_row<true>(off, power), pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s)
                           : oh_row_pass(who, oh_tweedie_row<false>(off, power), pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s);
        if (rc || !H) return rc;
        // (the Gram's partials overwrite the pass's in the same arena: the finish launch above has consumed them, in stream order)
        return onehot_gram_impl(pl, num, ldn, codes, ldc, w, n, H, ldh, ws_oh, ws_oh_bytes, s, false);
    };
}

}  // namespace dlsa

extern "C" {

size_t dlsa_onehot_tweedie_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int64_t row_step) {
    return dlsa::disp_onehot_workspace_bytes(dlsa::TWEEDIE_NC, plan, max_rows, row_step);
}

int dlsa_onehot_tweedie_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                 const double* y, const double* offset, const double* beta, double power, double dispersion, int64_t n,
                                 double* H, int64_t ldh, double* g, double* loglik, double* w_out, double* stats_out, void* ws,
                                 size_t ws_bytes, void* stream) {
    return dlsa::disp_onehot_pass_entry("onehot_tweedie_pass", dlsa::tweedie_family(power), dlsa::oh_tweedie_rows(power), plan, num, ldn,
                                        codes, ldc, y, offset, beta, dispersion, n, H, ldh, g, loglik, w_out, stats_out, ws, ws_bytes,
                                        stream);
}

int dlsa_onehot_tweedie_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                const double* y, const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host,
                                int64_t row_step, int K, double power, double dispersion_fixed, double tol, int max_iter, double* coef,
                                double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                                double* dispersion_host, double* pearson_host, double* deviance_host, void* ws, size_t ws_bytes,
                                void* stream) {
    return dlsa::disp_onehot_fit_entry("onehot_tweedie_fit", dlsa::tweedie_family(power), dlsa::oh_tweedie_rows(power), plan, num, ldn,
                                       codes, ldc, y, offset, part_first_host, part_rows_host, row_step, K, dispersion_fixed, tol,
                                       max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, dispersion_host,
                                       pearson_host, deviance_host, ws, ws_bytes, stream);
}

}  // extern "C"
