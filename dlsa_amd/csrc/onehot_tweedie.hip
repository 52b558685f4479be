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
// The once-per-partition sums, the dispersion sums over (y, mu) and the fit driver are tweedie.hip's (tweedie_internal.h), the
// scaling gamma.hip's; the row checks of num / codes and the plan's constant column are onehot_poisson.hip's (poisson_internal.h).
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
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
struct OhTweedieLayout {
    size_t off_oh, oh_bytes, off_w, off_mu, off_y, off_o, off_cpart, off_cst, off_dpart, off_dst, off_state, total;
};

// off_oh: the arena of the structured passes (the pass's partials, then the Gram's: onehot_workspace_bytes_impl sizes both);
// row_step > 1: room for the gathered responses and offsets of a strided partition; then the Newton state
static OhTweedieLayout oh_tweedie_layout(const dlsa_onehot_plan* pl, int64_t max_rows, int64_t row_step) {
    OhTweedieLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.oh_bytes = align_up(onehot_workspace_bytes_impl(pl, n), 256);
    l.off_oh = take(l.oh_bytes);
    l.off_w = take(8 * (size_t)n);
    l.off_mu = take(8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_cpart = take(8 * (size_t)TWEEDIE_NC * GAMMA_SUM_BLOCKS);
    l.off_cst = take(8 * 4);
    l.off_dpart = take(8 * (size_t)TWEEDIE_ND * GAMMA_SUM_BLOCKS);
    l.off_dst = take(8 * 4);
    l.off_state = take(newton_state_bytes(onehot_plan_p(pl)));
    l.total = o;
    return l;
}

// One partition at a fixed beta and unit dispersion.  H (nullable) needs w (the weight per row: the Gram's weights); g, loglik (the
// sum of q) and mu nullable.  ws_oh: the structured passes' arena (256-aligned, >= onehot_workspace_bytes_impl(pl, n)).
static int oh_tweedie_pass_impl(double power, const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes,
                                int64_t ldc, const double* y, const double* off, const double* beta, int64_t n, double* H, int64_t ldh,
                                double* g, double* loglik, double* w, double* mu, void* ws_oh, size_t ws_oh_bytes, hipStream_t s) {
    const char* who = "onehot tweedie pass";
    const int rc = off ? oh_row_pass(who, oh_tweedie_row<true>(off, power), pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s)
                       : oh_row_pass(who, oh_tweedie_row<false>(off, power), pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s);
    if (rc || !H) return rc;
    // (the Gram's partials overwrite the pass's in the same arena: the finish launch above has consumed them, in stream order)
    return onehot_gram_impl(pl, num, ldn, codes, ldc, w, n, H, ldh, ws_oh, ws_oh_bytes, s, false);
}

}  // namespace dlsa

extern "C" {

size_t dlsa_onehot_tweedie_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int64_t row_step) {
    if (!plan || max_rows < 0 || row_step < 1) return 0;
    return dlsa::oh_tweedie_layout(plan, max_rows, row_step).total;
}

int dlsa_onehot_tweedie_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                 const double* y, const double* offset, const double* beta, double power, double dispersion, int64_t n,
                                 double* H, int64_t ldh, double* g, double* loglik, double* w_out, double* stats_out, void* ws,
                                 size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && beta, "onehot_tweedie_pass: null plan, y or beta");
    int rc = oh_pois_check_rows("onehot_tweedie_pass", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    const int p = onehot_plan_p(plan);
    DLSA_REQUIRE(n >= 1 && (!H || ldh >= p), "onehot_tweedie_pass: bad shape n=%lld p=%d ldh=%lld", (long long)n, p, (long long)ldh);
    DLSA_REQUIRE(tweedie_power_ok(power), "onehot_tweedie_pass: the variance power must lie strictly between 1 and 2");
    DLSA_REQUIRE(dispersion > 0 && isfinite(dispersion), "onehot_tweedie_pass: the dispersion must be positive and finite");
    const OhTweedieLayout l = oh_tweedie_layout(plan, n, 1);
    rc = newton_check_ws("onehot_tweedie_pass", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    double* mu = stats_out ? (double*)(wsc + l.off_mu) : nullptr;
    rc = oh_tweedie_pass_impl(power, plan, num, ldn, codes, ldc, y, offset, beta, n, H, ldh, g, loglik, w, mu, wsc + l.off_oh, l.oh_bytes, s);
    if (rc) return rc;
    return tweedie_pass_finish(y, offset, mu, n, p, power, dispersion, H, ldh, g, loglik, stats_out, (double*)(wsc + l.off_cpart),
                               (double*)(wsc + l.off_cst), (double*)(wsc + l.off_dpart), s);
}

int dlsa_onehot_tweedie_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                const double* y, const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host,
                                int64_t row_step, int K, double power, double dispersion_fixed, double tol, int max_iter, double* coef,
                                double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                                double* dispersion_host, double* pearson_host, double* deviance_host, void* ws, size_t ws_bytes,
                                void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "onehot_tweedie_fit: null argument");
    int rc = oh_pois_check_rows("onehot_tweedie_fit", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    DLSA_REQUIRE(K > 0 && row_step >= 1, "onehot_tweedie_fit: bad shape K=%d step=%lld", K, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "onehot_tweedie_fit: bad tol/max_iter");
    DLSA_REQUIRE(tweedie_power_ok(power), "onehot_tweedie_fit: the variance power must lie strictly between 1 and 2");
    DLSA_REQUIRE(!(dispersion_fixed > 0) || isfinite(dispersion_fixed), "onehot_tweedie_fit: a fixed dispersion must be finite");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "onehot_tweedie_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const int p = onehot_plan_p(plan);
    const OhTweedieLayout l = oh_tweedie_layout(plan, max_rows, row_step);
    rc = newton_check_ws("onehot_tweedie_fit", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    TweedieFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.dpart = (double*)(wsc + l.off_dpart); b.dst = (double*)(wsc + l.off_dst);
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.mu = (double*)(wsc + l.off_mu);
    b.st = newton_state_at(wsc + l.off_state, p);
    double* wv = (double*)(wsc + l.off_w);
    void* ws_oh = wsc + l.off_oh;
    const size_t oh_bytes = l.oh_bytes;
    const int64_t pn = ldn * row_step, pc = ldc * row_step;   // rows first, first + step, ...: strided views, num / codes read in place
    const TweedieEval eval = [=](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* Hk, double* g,
                                 double* ll, double* mu) {
        const double* numk = num ? num + part_first_host[k] * ldn : nullptr;
        const int32_t* codesk = codes ? codes + part_first_host[k] * ldc : nullptr;
        return oh_tweedie_pass_impl(power, plan, numk, pn, codesk, pc, yk, ok, beta, nk, Hk, p, g, ll, wv, mu, ws_oh, oh_bytes, s);
    };
    return tweedie_fit_core("onehot_tweedie_fit", y, offset, part_first_host, part_rows_host, row_step, K, p, oh_pois_icpt_col(plan), power,
                            dispersion_fixed, tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host,
                            dispersion_host, pearson_host, deviance_host, b, eval, s);
}

}  // extern "C"
