// Structured Poisson map step for one-hot designs: the Poisson pass and fit of poisson.hip on the RAW representation of a
// design [intercept | standardised numerics | one-hot factor levels] (num [n, q] fp64, codes [n, f] int32) under a
// dlsa_onehot_plan -- the dense n x p matrix is never built.  Results equal the dense Poisson entries on the matrix
// dlsa_design_f64 would build (to rounding).
//
// Launches per evaluation at a fixed beta:
//   1 oh_row_kernel<OhPoisRow<OFF>>  the one-thread-per-row pass of onehot_pass.h (shared with the logistic model,
//                           onehot.hip) with the Poisson terms: eta = d . beta_D + sum_t beta[col(t, code_t)] + o (a gather),
//                           mu = exp_full(eta) (-> w), r = y - mu, per-workgroup partials of g (dense part in registers, level
//                           part an LDS histogram with replicated copies and wave turn-taking: a fixed order of the adds,
//                           bit-reproducible) and of sum y eta - mu;
//   2 logit_finish_launch   the fixed-order column sums of those partials (logit.hip, shared);
//   3 the Gram              onehot_gram_impl(plan, num, codes, mu) with irls_weights = false: mu is unbounded, so the ordered
//                           floating-point mode (full relative accuracy at any scale, bit-reproducible), never the fixed-point one.
// Traffic per row: 8q + 4f + 8 (y) + 8 (o) + 8 (mu written) bytes for the pass, 8q + 4f + 8 for the Gram.
// The constant sum lgamma(y + 1), the data check, the gather of a strided partition's counts / offsets and the Newton loop
// are poisson.hip's (poisson_internal.h).  The NB2 sibling (onehot_negbin.hip) takes the pass and the row checks from here.
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "poisson_exp.h"  // exp_full
#include "onehot_pass.h"  // oh_row_kernel, oh_row_pass

template <bool OFF>       // OFF = false reads no offsets
struct OhPoisRow {        // eta += o, mu = exp(eta) = w, term = y eta - mu
    static constexpr bool STORES_MU = false;
    const double* off;
    __device__ __forceinline__ double mean(int64_t i, double& eta) const {
        if constexpr (OFF) eta += off[i];
        return exp_full(eta);
    }
    __device__ __forceinline__ double resid(double y, double, double mu) const { return y - mu; }
    __device__ __forceinline__ double weight(double mu) const { return mu; }
    __device__ __forceinline__ double term(double y, double eta, double mu) const { return y * eta - mu; }
};

// ---- host side ---------------------------------------------------------------------------------------------------------
struct OhPoisLayout {
    size_t off_oh, oh_bytes, off_w, off_y, off_o, off_cpart, off_cst, off_state, total;
};

// off_oh: the arena of the structured passes (the pass's partials, then the Gram's: onehot_workspace_bytes_impl sizes both);
// row_step > 1: room for the gathered counts and offsets of a strided partition; then the Newton state
static OhPoisLayout oh_pois_layout(const dlsa_onehot_plan* pl, int64_t max_rows, int64_t row_step) {
    OhPoisLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.oh_bytes = align_up(onehot_workspace_bytes_impl(pl, n), 256);
    l.off_oh = take(l.oh_bytes);
    l.off_w = take(8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_cpart = take(8 * 4 * (size_t)POIS_CONST_BLOCKS);
    l.off_cst = take(8 * 4);
    l.off_state = take(newton_state_bytes(onehot_plan_p(pl)));
    l.total = o;
    return l;
}

static int oh_pois_ldn_min(const dlsa_onehot_plan* pl) {       // columns of num the plan reads
    int m = 0;
    for (int a = 0; a < pl->desc.D; ++a)
        if (pl->desc.dense_kind[a] == 1) m = std::max(m, pl->desc.dense_src[a] + 1);
    return m;
}

int oh_pois_icpt_col(const dlsa_onehot_plan* pl) {      // the plan's constant column, -1 without one
    for (int a = 0; a < pl->desc.D; ++a)
        if (pl->desc.dense_kind[a] == 0) return pl->desc.dense_col[a];
    return -1;
}

// One partition at a fixed beta.  H (nullable) needs w (mu per row: the Gram's weights); g, loglik (the sum of y eta - mu,
// without the constant) nullable.  ws_oh: the structured passes' arena (256-aligned, >= onehot_workspace_bytes_impl(pl, n)).
int oh_pois_pass_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                             const double* y, const double* off, const double* beta, int64_t n, double* H, int64_t ldh, double* g,
                             double* loglik, double* w, void* ws_oh, size_t ws_oh_bytes, hipStream_t s) {
    const char* who = "onehot poisson pass";
    const int rc = off ? oh_row_pass(who, OhPoisRow<true>{off}, pl, num, ldn, codes, ldc, y, beta, n, w, nullptr, g, loglik, ws_oh, ws_oh_bytes, s)
                       : oh_row_pass(who, OhPoisRow<false>{off}, pl, num, ldn, codes, ldc, y, beta, n, w, nullptr, g, loglik, ws_oh, ws_oh_bytes, s);
    if (rc || !H) return rc;
    // (the Gram's partials overwrite the pass's in the same arena: the finish launch above has consumed them, in stream order)
    return onehot_gram_impl(pl, num, ldn, codes, ldc, w, n, H, ldh, ws_oh, ws_oh_bytes, s, false);
}

int oh_pois_check_rows(const char* who, const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes,
                              int64_t ldc) {
    DLSA_REQUIRE(num || !pl->needs_num, "%s: null num (the plan has numeric columns)", who);
    DLSA_REQUIRE(codes || pl->desc.f == 0, "%s: null codes (the plan has factors)", who);
    DLSA_REQUIRE((!pl->needs_num || ldn >= oh_pois_ldn_min(pl)) && (pl->desc.f == 0 || ldc >= pl->desc.f),
                 "%s: bad shape ldn=%lld (the plan reads %d numeric columns) ldc=%lld (%d factors)", who, (long long)ldn,
                 oh_pois_ldn_min(pl), (long long)ldc, pl->desc.f);
    return DLSA_OK;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_onehot_poisson_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int64_t row_step) {
    if (!plan || max_rows < 0 || row_step < 1) return 0;
    return dlsa::oh_pois_layout(plan, max_rows, row_step).total;
}

int dlsa_onehot_poisson_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                 const double* y, const double* offset, const double* beta, int64_t n, double* H, int64_t ldh,
                                 double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && beta, "onehot_poisson_pass: null plan, y or beta");
    int rc = oh_pois_check_rows("onehot_poisson_pass", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    const int p = onehot_plan_p(plan);
    DLSA_REQUIRE(n >= 1 && (!H || ldh >= p), "onehot_poisson_pass: bad shape n=%lld p=%d ldh=%lld", (long long)n, p, (long long)ldh);
    const OhPoisLayout l = oh_pois_layout(plan, n, 1);
    rc = newton_check_ws("onehot_poisson_pass", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    rc = oh_pois_pass_impl(plan, num, ldn, codes, ldc, y, offset, beta, n, H, ldh, g, loglik, w, wsc + l.off_oh, l.oh_bytes, s);
    if (rc || !loglik) return rc;
    rc = pois_const(y, offset, n, (double*)(wsc + l.off_cpart), (double*)(wsc + l.off_cst), s);
    if (rc) return rc;
    return pois_ll_fix(loglik, (const double*)(wsc + l.off_cst), s);
}

int dlsa_onehot_poisson_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                const double* y, const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host,
                                int64_t row_step, int K, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                                int* n_iter_host, int* status_host, double* loglik_host, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "onehot_poisson_fit: null argument");
    int rc = oh_pois_check_rows("onehot_poisson_fit", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    DLSA_REQUIRE(K > 0 && row_step >= 1, "onehot_poisson_fit: bad shape K=%d step=%lld", K, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "onehot_poisson_fit: bad tol/max_iter");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "onehot_poisson_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const int p = onehot_plan_p(plan);
    const OhPoisLayout l = oh_pois_layout(plan, max_rows, row_step);
    rc = newton_check_ws("onehot_poisson_fit", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    PoisFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.st = newton_state_at(wsc + l.off_state, p);
    double* wv = (double*)(wsc + l.off_w);
    void* ws_oh = wsc + l.off_oh;
    const size_t oh_bytes = l.oh_bytes;
    const int64_t pn = ldn * row_step, pc = ldc * row_step;   // rows first, first + step, ...: strided views, num / codes read in place
    const PoisEval eval = [=](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* Hk, double* g,
                              double* ll) {
        const double* numk = num ? num + part_first_host[k] * ldn : nullptr;
        const int32_t* codesk = codes ? codes + part_first_host[k] * ldc : nullptr;
        return oh_pois_pass_impl(plan, numk, pn, codesk, pc, yk, ok, beta, nk, Hk, p, g, ll, wv, ws_oh, oh_bytes, s);
    };
    return pois_fit_core("onehot_poisson_fit", y, offset, part_first_host, part_rows_host, row_step, K, p, oh_pois_icpt_col(plan), tol,
                         max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, b, eval, s);
}

}  // extern "C"
