// Structured negative-binomial (NB2) map step for one-hot designs: the NB2 pass and fit of negbin.hip on the RAW representation
// of a design [intercept | standardised numerics | one-hot factor levels] (num [n, q] fp64, codes [n, f] int32) under a
// dlsa_onehot_plan -- the dense n x p matrix is never built.  Results equal the dense NB2 entries on the matrix dlsa_design_f64
// would build (to rounding).
//
// Launches per evaluation at a fixed (beta, alpha), alpha > 0:
//   1 oh_row_kernel<OhNbRow<OFF>>  the one-thread-per-row pass of onehot_pass.h (shared with the logistic and the Poisson model)
//                           with the terms of NbRow (negbin_internal.h, shared with the dense pass): eta = d . beta_D +
//                           sum_t beta[col(t, code_t)] + o (a gather), mu = exp_full(eta) (-> the theta step), w = mu q (-> the
//                           Gram's weights), r = (y - mu) q, per-workgroup partials of g (dense part in registers, level part an LDS
//                           histogram with replicated copies and wave turn-taking: a fixed order of the adds, bit-reproducible) and
//                           of sum y eta - (y + theta) L;
//   2 logit_finish_launch   the fixed-order column sums of those partials (logit.hip, shared);
//   3 the Gram              onehot_gram_impl(plan, num, codes, w) with irls_weights = false: w is bounded by 1 / alpha but spans many
//                           orders of magnitude, so the ordered floating-point mode, never the fixed-point one.
// Traffic per row: 8q + 4f + 8 (y) + 8 (o) + 16 (w, mu written) bytes for the pass, 8q + 4f + 8 for the Gram.
// alpha = 0 (the fit's look at the Poisson MLE) is the Poisson pass of onehot_poisson.hip with its weight output, mu, aimed at
// the mu buffer.  The theta step (16 bytes per row), its finish, the log-likelihood fix and the fit driver are negbin.hip's
// (negbin_internal.h); the Poisson start is dlsa_onehot_poisson_fit_f64 on one partition.
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include "negbin_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "poisson_exp.h"  // exp_full
#include "onehot_pass.h"  // oh_row_kernel, oh_row_pass

template <bool OFF>       // OFF = false reads no offsets
struct OhNbRow {          // eta += o, mu = exp(eta); weight, residual and term are NbRow's, computed once per row (resid)
    static constexpr bool STORES_MU = true;
    NbRow nb;
    const double* off;
    double wgt, llt;      // of the row in hand
    __device__ __forceinline__ double mean(int64_t i, double& eta) const {
        if constexpr (OFF) eta += off[i];
        return exp_full(eta);
    }
    __device__ __forceinline__ double resid(double y, double eta, double mu) {
        double rs;
        nb.terms(y, eta, mu, wgt, rs, llt);
        return rs;
    }
    __device__ __forceinline__ double weight(double) const { return wgt; }
    __device__ __forceinline__ double term(double, double, double) const { return llt; }
};

// ---- host side ---------------------------------------------------------------------------------------------------------
struct OhNbLayout {
    size_t off_y, off_o, off_pois, off_oh, oh_bytes, off_tpart, off_tst, off_w, off_mu, off_state, total;
};

// [gathered counts | gathered offsets] of a strided partition, then the Poisson start's workspace (pois_bytes: the Poisson
// sibling's whole layout; 0 for the pass) overlaid with the NB scratch -- the two never run at the same time: the arena of the
// structured passes, the theta step's partials, w, mu and the Newton state
static OhNbLayout oh_nb_layout(const dlsa_onehot_plan* pl, int64_t max_rows, int64_t row_step, size_t pois_bytes) {
    OhNbLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_pois = o;
    l.oh_bytes = align_up(onehot_workspace_bytes_impl(pl, n), 256);
    l.off_oh = take(l.oh_bytes);
    l.off_tpart = take(8 * (size_t)NB_NQ * NB_THETA_BLOCKS);
    l.off_tst = take(8 * 16);
    l.off_w = take(8 * (size_t)n);
    l.off_mu = take(8 * (size_t)n);
    l.off_state = take(newton_state_bytes(onehot_plan_p(pl)));
    l.total = std::max(o, align_up(l.off_pois + pois_bytes, 256));
    return l;
}

// One partition at a fixed (beta, alpha).  alpha > 0: w is mu q per row, loglik the row sum of y eta - (y + theta) L, without
// c(theta); H (nullable) needs w.  alpha = 0 (the fit's look at the Poisson MLE): the Poisson pass with its weight output, mu,
// aimed at the mu buffer; w is not written.  ws_oh: the structured passes' arena.
static int oh_nb_pass_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                           const double* y, const double* off, const double* beta, double alpha, int64_t n, double* H, int64_t ldh,
                           double* g, double* loglik, double* w, double* mu, void* ws_oh, size_t ws_oh_bytes, hipStream_t s) {
    if (!(alpha > 0.0)) return oh_pois_pass_impl(pl, num, ldn, codes, ldc, y, off, beta, n, H, ldh, g, loglik, mu, ws_oh, ws_oh_bytes, s);
    const char* who = "onehot negbin pass";
    const NbRow nb{alpha, 1.0 / alpha, log(alpha)};
    const int rc = off ? oh_row_pass(who, OhNbRow<true>{nb, off}, pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s)
                       : oh_row_pass(who, OhNbRow<false>{nb, off}, pl, num, ldn, codes, ldc, y, beta, n, w, mu, g, loglik, ws_oh, ws_oh_bytes, s);
    if (rc || !H) return rc;
    // (the Gram's partials overwrite the pass's in the same arena: the finish launch above has consumed them, in stream order)
    return onehot_gram_impl(pl, num, ldn, codes, ldc, w, n, H, ldh, ws_oh, ws_oh_bytes, s, false);
}

}  // namespace dlsa

extern "C" {

size_t dlsa_onehot_negbin_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int64_t row_step) {
    if (!plan || max_rows < 0 || row_step < 1) return 0;
    const size_t pois = dlsa_onehot_poisson_workspace_bytes(plan, max_rows, row_step);
    return dlsa::oh_nb_layout(plan, max_rows, row_step, pois).total;
}

int dlsa_onehot_negbin_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                const double* y, const double* offset, const double* beta, double alpha, int64_t n, double* H,
                                int64_t ldh, double* g, double* loglik, double* w_out, double* mu_out, double* theta_terms, void* ws,
                                size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && beta, "onehot_negbin_pass: null plan, y or beta");
    int rc = oh_pois_check_rows("onehot_negbin_pass", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    const int p = onehot_plan_p(plan);
    DLSA_REQUIRE(n >= 1 && (!H || ldh >= p), "onehot_negbin_pass: bad shape n=%lld p=%d ldh=%lld", (long long)n, p, (long long)ldh);
    DLSA_REQUIRE(alpha > 0 && isfinite(alpha),
                 "onehot_negbin_pass: alpha must be positive and finite (alpha = 0 is dlsa_onehot_poisson_pass_f64)");
    const OhNbLayout l = oh_nb_layout(plan, n, 1, 0);
    rc = newton_check_ws("onehot_negbin_pass", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    const bool want_theta = loglik || theta_terms;
    double* mu = mu_out ? mu_out : (want_theta ? (double*)(wsc + l.off_mu) : nullptr);
    rc = oh_nb_pass_impl(plan, num, ldn, codes, ldc, y, offset, beta, alpha, n, H, ldh, g, loglik, w, mu, wsc + l.off_oh, l.oh_bytes, s);
    if (rc || !want_theta) return rc;
    double* tst = (double*)(wsc + l.off_tst);
    rc = nb_theta_launch(y, mu, offset, n, alpha, loglik ? 1 : 0, (double*)(wsc + l.off_tpart), tst, s);
    if (rc) return rc;
    if (theta_terms) DLSA_HIP_CHECK(hipMemcpyAsync(theta_terms, tst + NB_S, 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (loglik) return nb_ll_fix(loglik, tst, s);
    return DLSA_OK;
}

int dlsa_onehot_negbin_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                               const double* y, const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host,
                               int64_t row_step, int K, double alpha_fixed, double tol, int max_iter, double* coef, double* Sig_inv,
                               double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, double* alpha_host,
                               double* alpha_info_host, double* pearson_host, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "onehot_negbin_fit: null argument");
    int rc = oh_pois_check_rows("onehot_negbin_fit", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    DLSA_REQUIRE(K > 0 && row_step >= 1, "onehot_negbin_fit: bad shape K=%d step=%lld", K, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "onehot_negbin_fit: bad tol/max_iter");
    DLSA_REQUIRE(!(alpha_fixed > 0) || isfinite(alpha_fixed), "onehot_negbin_fit: a fixed alpha must be finite");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "onehot_negbin_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const int p = onehot_plan_p(plan);
    const size_t pois_bytes = dlsa_onehot_poisson_workspace_bytes(plan, max_rows, row_step);
    const OhNbLayout l = oh_nb_layout(plan, max_rows, row_step, pois_bytes);
    rc = newton_check_ws("onehot_negbin_fit", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    NbFitBufs b{};
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.w = (double*)(wsc + l.off_w); b.mu = (double*)(wsc + l.off_mu);
    b.tpart = (double*)(wsc + l.off_tpart); b.tst = (double*)(wsc + l.off_tst);
    b.st = newton_state_at(wsc + l.off_state, p);
    void* ws_oh = wsc + l.off_oh;
    const size_t oh_bytes = l.oh_bytes;
    const int64_t pn = ldn * row_step, pc = ldc * row_step;   // rows first, first + step, ...: strided views, num / codes read in place
    const NbPoisFit pois = [=](int k, double* ck, double* Hk, double* sk, int* iters, int* st_k, double* ll) {
        return dlsa_onehot_poisson_fit_f64(plan, num, ldn, codes, ldc, y, offset, part_first_host + k, part_rows_host + k, row_step, 1,
                                           tol, max_iter, ck, Hk, sk, iters, st_k, ll, wsc + l.off_pois, l.total - l.off_pois, stream);
    };
    const NbEval eval = [=](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double alpha, double* Hk, double* g,
                            double* ll, double* w, double* mu) {
        const double* numk = num ? num + part_first_host[k] * ldn : nullptr;
        const int32_t* codesk = codes ? codes + part_first_host[k] * ldc : nullptr;
        return oh_nb_pass_impl(plan, numk, pn, codesk, pc, yk, ok, beta, alpha, nk, Hk, p, g, ll, w, mu, ws_oh, oh_bytes, s);
    };
    return nb_fit_core("onehot_negbin_fit", y, offset, part_first_host, part_rows_host, row_step, K, p, alpha_fixed, tol, max_iter, coef,
                       Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, alpha_host, alpha_info_host, pearson_host, b, pois,
                       eval, s);
}

}  // extern "C"
