// Probit and complementary log-log regression map steps for a 0/1 response (the two binary links beside the logit; optional offsets /
// exposure): one partition's log-likelihood, score and OBSERVED information at a fixed beta, and the per-partition Newton fit on
// top of it.  The block a partition returns (coef, Sig_inv = the information at coef, Sig_inv coef) feeds the unchanged one-round
// combine.  include/dlsa_hip_binary.h holds the contract.
//
// Algebra (one partition; the design is [1 | X] with the implicit intercept, X otherwise; o = offset, 0 when absent):
//   eta = [1 | x]' beta + o,  l = the row's log-likelihood term,  r = dl / deta,  w = -d2l / deta2 >= 0,
//   loglik = sum l (no constant term),  g = X'r,  H = X' diag(w) X.
//   probit:   s = 2y - 1, z = s eta, lambda = phi(z) / Phi(z):  l = log Phi(z),  r = s lambda,  w = lambda (z + lambda)
//   cloglog:  mu = e^eta;  y = 0: l = -mu, r = -mu, w = mu (the Poisson row);  y = 1: l = log(1 - e^-mu), r = mu / (e^mu - 1),
//             w = r (mu + r - 1)
// binary_terms.h evaluates them without the cancellations of these forms.
//
// Launches per evaluation: those of poisson.hip -- count_pass_kernel (count_pass.h) with the terms of ProbitRow / CloglogRow,
// logit_finish_launch, the Gram dispatch on (X, w).  The probit row does not use the pass's mu = exp_full(eta): it is dead code in
// those instantiations and the compiler removes it.  Once per partition: binary_check_kernel + block_sum_finish (the rows that are
// not 0/1 or have a non-finite offset, sum y and sum e^o for the intercept's start value).  The fit is newton_fit_loop (newton_fit.h)
// with Poisson's policy, on the gather, start and finish helpers of poisson_internal.h.
#include "common.h"
#include "block_sums.h"
#include "poisson_internal.h"
#include "../../include/dlsa_hip_binary.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"        // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "poisson_exp.h"   // exp_full
#include "count_pass.h"    // count_pass_kernel, count_pass, CountScratch
#include "binary_terms.h"  // probit_terms, cloglog_terms
#include "binary_start.h"  // dlsa_probit_quantile

struct ProbitRow {
    static constexpr bool STORES_MU = false;
    static constexpr const char* NAME = "probit";
    __device__ __forceinline__ void terms(double yv, double eta, double, double& wgt, double& rs, double& llt) const {
        probit_terms(yv, eta, wgt, rs, llt);
    }
    // Phi^-1(ones / rows), 0 < ones < rows: the bracketed quantile of binary_start.h
    static double link(double ones, double rows) { return dlsa_probit_quantile(ones, rows); }
};

struct CloglogRow {
    static constexpr bool STORES_MU = false;
    static constexpr const char* NAME = "cloglog";
    __device__ __forceinline__ void terms(double yv, double eta, double mu, double& wgt, double& rs, double& llt) const {
        cloglog_terms(yv, eta, mu, wgt, rs, llt);
    }
    static double link(double ones, double rows) { return log(-log1p(-ones / rows)); }
};

// ---- once per partition: [rows, sum y, sum e^o, rows whose y is not exactly 0 or 1 or whose offset is not finite] ------------
constexpr int BIN_NQ = 4;
__global__ __launch_bounds__(256) void binary_check_kernel(const double* __restrict__ y, const double* __restrict__ off, int64_t n,
                                                           double* __restrict__ part) {
    double rows = 0.0, sy = 0.0, se = 0.0, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yv = y[i], ov = off ? off[i] : 0.0;
        rows += 1.0;
        if ((yv == 0.0 || yv == 1.0) && isfinite(ov)) {         // (NaN fails both comparisons)
            sy += yv;
            se += exp_full(ov);
        } else {
            bad += 1.0;
        }
    }
    const double acc[BIN_NQ] = {rows, sy, se, bad};
    block_partials_store(acc, part);
}

// the pass entries' log-likelihood: NaN when a row is not a valid response
__global__ void binary_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ cst) {
    if (threadIdx.x == 0 && cst[3] > 0.0) ll[0] = NAN;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct BinLayout {
    CountScratchOff sc;
    size_t off_cpart, off_cst, off_w, off_y, off_o, off_gram, total;
};

// pass scratch; row_step > 1: room for the gathered responses and offsets of a strided partition
static BinLayout bin_layout(int64_t max_rows, int p, int64_t row_step) {
    BinLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.sc = count_scratch_take(take, p);
    l.off_cpart = take(8 * BIN_NQ * (size_t)POIS_CONST_BLOCKS);
    l.off_cst = take(8 * BIN_NQ);
    l.off_w = take(8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_gram = take(gram_workspace_bytes_impl(n, p, 8));
    l.total = o;
    return l;
}

static size_t bin_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    if (p <= 0 || p + (intercept ? 1 : 0) > 2048 || max_rows < 0 || row_step < 1) return 0;
    return align_up(bin_layout(max_rows, p, row_step).total, 256) + newton_state_bytes(p + (intercept ? 1 : 0));
}

static int bin_check(const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s) {
    const int blocks = (int)std::min<int64_t>(POIS_CONST_BLOCKS, std::max<int64_t>(1, (n + 255) / 256));
    hipLaunchKernelGGL(binary_check_kernel, dim3(blocks), dim3(256), 0, s, y, off, n, cpart);
    return block_sum_finish(cpart, blocks, BIN_NQ, cst, s);
}

template <class M>
static int bin_pass_impl(const double* X, int64_t ldx, const double* y, const double* off, const double* beta, int64_t n, int p,
                         int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w, char* ws, const BinLayout& l,
                         hipStream_t s) {
    return count_pass(M{}, X, ldx, y, off, beta, n, p, intercept, H, ldh, g, loglik, w, nullptr, count_scratch_at(ws, l.sc),
                      ws + l.off_gram, l.total - l.off_gram, s);
}

template <class M>
static int bin_pass_entry(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, int64_t n, int p,
                          int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes,
                          void* stream) {
    DLSA_REQUIRE(X && y && beta, "%s_pass: null X, y or beta", M::NAME);
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(n >= 1 && p > 0 && pe <= 2048 && ldx >= p && (!H || ldh >= pe), "%s_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld",
                 M::NAME, (long long)n, p, (long long)ldx, (long long)ldh);
    const BinLayout l = bin_layout(n, p, 1);
    char who[32];
    snprintf(who, sizeof(who), "%s_pass", M::NAME);
    // (the pass carves l.total of it; the contract is the query, which also holds a fit's Newton state)
    int rc = newton_check_ws(who, ws, ws_bytes, bin_workspace_bytes(n, p, intercept, 1));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    rc = bin_pass_impl<M>(X, ldx, y, offset, beta, n, p, intercept, H, ldh, g, loglik, w, wsc, l, s);
    if (rc || !loglik) return rc;
    rc = bin_check(y, offset, n, (double*)(wsc + l.off_cpart), (double*)(wsc + l.off_cst), s);
    if (rc) return rc;
    hipLaunchKernelGGL(binary_ll_fix_kernel, dim3(1), dim3(64), 0, s, loglik, (const double*)(wsc + l.off_cst));
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

// The per-partition driver, after pois_fit_core: the data check, the degenerate partitions, the start and newton_fit_loop.
template <class M>
static int bin_fit_entry(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double tol, int max_iter,
                         double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                         void* ws, size_t ws_bytes, void* stream) {
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "%s_fit: null argument", M::NAME);
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(K > 0 && p > 0 && pe <= 2048 && ldx >= p && row_step >= 1, "%s_fit: bad shape K=%d p=%d ldx=%lld step=%lld", M::NAME, K,
                 p, (long long)ldx, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "%s_fit: bad tol/max_iter", M::NAME);
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "%s_fit: negative partition shape (partition %d)", M::NAME, k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const BinLayout l = bin_layout(max_rows, p, row_step);
    char who[32];
    snprintf(who, sizeof(who), "%s_fit", M::NAME);
    const int rcw = newton_check_ws(who, ws, ws_bytes, bin_workspace_bytes(max_rows, p, intercept, row_step));
    if (rcw) return rcw;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* cpart = (double*)(wsc + l.off_cpart);
    double* cstd = (double*)(wsc + l.off_cst);
    double* ybuf = (double*)(wsc + l.off_y);
    double* obuf = (double*)(wsc + l.off_o);
    double* wv = (double*)(wsc + l.off_w);
    const NewtonState st = newton_state_at(wsc + align_up(l.total, 256), pe);
    const int64_t pitch = ldx * row_step;                     // rows first, first + step, ...: a strided view, no copy of X
    int overall = DLSA_OK;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_rows_host[k];
        const double *yk = nullptr, *ok = nullptr;
        double* Hk = Sig_inv + (size_t)k * pe * pe;
        int st_k = DLSA_PART_EMPTY, iters = 0;
        double ll = 0.0, cst[BIN_NQ] = {0.0, 0.0, 0.0, 0.0};
        if (nk > 0) {
            int rc = pois_gather_rows(y, offset, part_first_host[k], row_step, nk, ybuf, obuf, yk, ok, s);
            if (rc) return rc;
            rc = bin_check(yk, ok, nk, cpart, cstd, s);
            if (rc) return rc;
            DLSA_HIP_CHECK(hipMemcpyAsync(cst, cstd, sizeof(cst), hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            if (cst[3] > 0.0) {
                set_error("%s: partition %d has %.0f rows whose response is not 0 or 1 or whose offset is not finite", who, k, cst[3]);
                return DLSA_ERR_INVALID;
            }
        }
        // with an intercept, all responses 0 or all 1: the MLE lies at eta -> -+inf, where H -> 0 and H theta -> 0: the zero block is
        // the block's limit.  Without an intercept such a partition can have a finite MLE: the loop runs.
        const bool one_class = cst[1] == 0.0 || cst[1] == cst[0];
        if (nk > 0 && !(intercept && one_class)) {
            // the intercept starts at the link of the response share, less the log of the mean e^o (cloglog: the exact MLE of the
            // intercept-only model under a common offset; probit: a start)
            double b0 = 0.0;
            if (intercept) {
                b0 = M::link(cst[1], cst[0]);
                if (ok && cst[2] > 0.0 && isfinite(cst[2])) b0 -= log(cst[2] / cst[0]);
                if (!isfinite(b0)) b0 = 0.0;
            }
            const int rcs = pois_start(st.beta, pe, intercept ? 0 : -1, b0, s);
            if (rcs) return rcs;
            const NewtonDevice dev{st, Hk, pe, s};
            NewtonOutcome o;
            const double* Xk = X + part_first_host[k] * ldx;
            const int rcl = newton_fit_loop(NEWTON_POISSON, tol, max_iter + 1,
                                            [&](bool&) {
                                                return bin_pass_impl<M>(Xk, pitch, yk, ok, st.beta, nk, p, intercept, Hk, pe, st.g, st.stats + 3, wv,
                                                                        wsc, l, s);
                                            },
                                            dev, newton_no_hook, o);
            if (rcl) return rcl;
            st_k = o.status; iters = o.n_iter; ll = o.ll;
        }
        const int rcf = newton_fit_finish(st_k, iters, ll, st.beta, pe, Hk, coef + (size_t)k * pe, Sig_invMcoef + (size_t)k * pe, k,
                                          n_iter_host, status_host, loglik_host, overall, s);
        if (rcf) return rcf;
    }
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    return overall;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_probit_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    return dlsa::bin_workspace_bytes(max_rows, p, intercept, row_step);
}

int dlsa_probit_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, int64_t n, int p,
                         int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes,
                         void* stream) {
    return dlsa::bin_pass_entry<dlsa::ProbitRow>(X, ldx, y, offset, beta, n, p, intercept, H, ldh, g, loglik, w_out, ws, ws_bytes, stream);
}

int dlsa_probit_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                        const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double tol, int max_iter,
                        double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                        void* ws, size_t ws_bytes, void* stream) {
    return dlsa::bin_fit_entry<dlsa::ProbitRow>(X, ldx, y, offset, part_first_host, part_rows_host, row_step, K, p, intercept, tol, max_iter,
                                                coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, ws, ws_bytes, stream);
}

size_t dlsa_cloglog_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    return dlsa::bin_workspace_bytes(max_rows, p, intercept, row_step);
}

int dlsa_cloglog_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, int64_t n, int p,
                          int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes,
                          void* stream) {
    return dlsa::bin_pass_entry<dlsa::CloglogRow>(X, ldx, y, offset, beta, n, p, intercept, H, ldh, g, loglik, w_out, ws, ws_bytes, stream);
}

int dlsa_cloglog_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double tol, int max_iter,
                         double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                         void* ws, size_t ws_bytes, void* stream) {
    return dlsa::bin_fit_entry<dlsa::CloglogRow>(X, ldx, y, offset, part_first_host, part_rows_host, row_step, K, p, intercept, tol, max_iter,
                                                 coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, ws, ws_bytes, stream);
}

}  // extern "C"
