// Gamma regression map step (log link, optional offsets / exposure, estimated or fixed dispersion) for positive, right-skewed
// continuous responses: one partition's log-likelihood, score and observed information at a fixed beta and dispersion, the
// Pearson and deviance sums, and the per-partition Newton fit on top of them.  The block a partition returns (coef, Sig_inv = the
// information at coef and the partition's dispersion, Sig_inv coef) feeds the unchanged one-round combine.
//
// Algebra (one partition; D = [1 | X] with the implicit intercept, X otherwise; o = offset, 0 when absent; nu = 1 / phi):
//   eta = D beta + o,  mu = exp(eta),  r = y / mu,
//   loglik = nu sum(-r - eta) + n (nu log nu - lgamma nu) + (nu - 1) sum log y,
//   g = nu D'(r - 1),  H = nu D' diag(r) D   (the observed information: r >= 0, so the negative log-likelihood is convex in beta),
//   P = sum (r - 1)^2,  Dev = 2 sum (r - 1 - log r),  phi^ = P / (n - pe).
// beta^ does not depend on phi, so the row pass and the Newton loop run at nu = 1 and the dispersion enters afterwards, as one
// scalar on H and g.
//
// Launches per evaluation (every partial combines in a fixed order: no float atomics, no waits between workgroups):
//   1 count_pass_kernel     (count_pass.h, shared with poisson.hip and negbin.hip, here with the terms of GammaRow) one read of
//                           the rows: r (-> w, the Gram's weights), mu (-> the dispersion sums), per-block partials of g,
//                           sum (r - 1), sum -(r + eta) and, with the intercept and H wanted, of X'r and sum r;
//   2 logit_finish_launch   the fixed-order column sums of those partials (logit.hip, shared);
//   3 the Gram              dlsa_gram_f64's dispatch on (X, r) into the p x p block (gram_icpt_impl with the border).
// Once per partition: gamma_const_kernel + gamma_sum_finish_kernel (sum log y, sum y e^-o for the intercept's start, the data
// check).  Once per fit (and per pass that asks): gamma_disp_kernel + the same finish over (y, mu), 16 bytes per row, and
// gamma_scale_kernel on the pe x pe block.
// The fit driver (gamma_fit_core) takes the evaluation as a callable and is shared with the structured one-hot fit
// (onehot_gamma.hip) through gamma_internal.h; the Newton iteration is newton_fit.h's with the policy of the Poisson fit, the
// gather of a strided partition's responses and offsets poisson_internal.h's.
#include "common.h"
#include "poisson_internal.h"
#include "gamma_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"       // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "poisson_exp.h"  // exp_full
#include "count_pass.h"   // count_pass_kernel, count_pass, CountScratch

// the Gamma row at unit dispersion: weight r = y / mu, residual r - 1, term -(r + eta)
struct GammaRow {
    static constexpr bool STORES_MU = true;
    __device__ __forceinline__ void terms(double yv, double eta, double mu, double& wgt, double& rs, double& llt) const {
        const double r = yv / mu;
        wgt = r;
        rs = r - 1.0;
        llt = -(r + eta);
    }
};

// ---- once per partition: [sum log y, sum y e^-o, rows with y <= 0 or a non-finite y / o] ---------------------------------
__global__ __launch_bounds__(256) void gamma_const_kernel(const double* __restrict__ y, const double* __restrict__ off, int64_t n,
                                                          double* __restrict__ part) {
    __shared__ double red[4][GAMMA_NC];
    double acc[GAMMA_NC] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yv = y[i], ov = off ? off[i] : 0.0;
        if (yv > 0.0 && isfinite(yv) && isfinite(ov)) {       // (NaN fails yv > 0)
            acc[GAMMA_LOGY] += log(yv);
            acc[GAMMA_YEO] += yv * exp_full(-ov);
        } else {
            acc[GAMMA_BAD] += 1.0;
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < GAMMA_NC; ++j) {
        const double t = wave_allreduce_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) red[wave][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < GAMMA_NC) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) t += red[k][threadIdx.x];
        part[(int64_t)blockIdx.x * GAMMA_NC + threadIdx.x] = t;
    }
}

// ---- the dispersion sums over (y, mu): [sum (r - 1)^2, 2 sum (r - 1 - log r)] ---------------------------------------------
__global__ __launch_bounds__(256) void gamma_disp_kernel(const double* __restrict__ y, const double* __restrict__ mu, int64_t n,
                                                         double* __restrict__ part) {
    __shared__ double red[4][GAMMA_ND];
    double ps = 0.0, dv = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double r = y[i] / mu[i], d = r - 1.0;
        ps = fma(d, d, ps);
        dv += d - log(r);
    }
    ps = wave_allreduce_sum(ps);
    dv = wave_allreduce_sum(dv);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][GAMMA_PEARSON] = ps; red[wave][GAMMA_DEV] = dv; }
    __syncthreads();
    if (threadIdx.x < GAMMA_ND) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) t += red[k][threadIdx.x];
        part[(int64_t)blockIdx.x * GAMMA_ND + threadIdx.x] = threadIdx.x == GAMMA_DEV ? 2.0 * t : t;
    }
}

// one wave per quantity (nq <= 4 of them), the block partials in a fixed order
__global__ __launch_bounds__(256) void gamma_sum_finish_kernel(const double* __restrict__ part, int nblocks, int nq,
                                                               double* __restrict__ out) {
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (j >= nq) return;
    double s = 0.0;
    for (int b = lane; b < nblocks; b += 64) s += part[(int64_t)b * nq + j];
    s = wave_allreduce_sum(s);
    if (lane == 0) out[j] = s;
}

// H (pe x pe, pitch ldh) and g (pe) times nu; either may be null
__global__ void gamma_scale_kernel(double* __restrict__ H, int64_t ldh, int pe, double* __restrict__ g, double nu) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (H && i < (int64_t)pe * pe) H[(i / pe) * ldh + i % pe] *= nu;
    if (g && i < pe) g[i] *= nu;
}

// the pass entry's full log-likelihood from the row sum of -(r + eta): nu ll + c + (nu - 1) sum log y (NaN when a row is not a
// valid response)
__global__ void gamma_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ cst, double nu, double c) {
    if (threadIdx.x == 0) ll[0] = cst[GAMMA_BAD] > 0.0 ? NAN : fma(nu, ll[0], c) + (nu - 1.0) * cst[GAMMA_LOGY];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int gamma_sum_blocks(int64_t n) { return (int)std::min<int64_t>(GAMMA_SUM_BLOCKS, std::max<int64_t>(1, (n + 255) / 256)); }

int gamma_sum_finish(const double* part, int nblocks, int nq, double* out, hipStream_t s) {
    hipLaunchKernelGGL(gamma_sum_finish_kernel, dim3(1), dim3(256), 0, s, part, nblocks, nq, out);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int gamma_const(const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s) {
    const int blocks = gamma_sum_blocks(n);
    hipLaunchKernelGGL(gamma_const_kernel, dim3(blocks), dim3(256), 0, s, y, off, n, cpart);
    return gamma_sum_finish(cpart, blocks, GAMMA_NC, cst, s);
}

int gamma_disp(const double* y, const double* mu, int64_t n, double* dpart, double* dst, hipStream_t s) {
    const int blocks = gamma_sum_blocks(n);
    hipLaunchKernelGGL(gamma_disp_kernel, dim3(blocks), dim3(256), 0, s, y, mu, n, dpart);
    return gamma_sum_finish(dpart, blocks, GAMMA_ND, dst, s);
}

int gamma_scale(double* H, int64_t ldh, int pe, double* g, double nu, hipStream_t s) {
    if (!H && !g) return DLSA_OK;
    const int64_t items = H ? (int64_t)pe * pe : pe;
    hipLaunchKernelGGL(gamma_scale_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, H, ldh, pe, g, nu);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

double gamma_ll_const(double nu, int64_t n) { return (double)n * (nu * log(nu) - lgamma(nu)); }

int gamma_pass_finish(const double* y, const double* off, const double* mu, int64_t n, int pe, double dispersion, double* H,
                      int64_t ldh, double* g, double* loglik, double* stats_out, double* cpart, double* cst, double* dpart,
                      hipStream_t s) {
    const double nu = 1.0 / dispersion;
    int rc = DLSA_OK;
    if (stats_out) {
        rc = gamma_disp(y, mu, n, dpart, stats_out, s);
        if (rc) return rc;
    }
    if (nu != 1.0) {
        rc = gamma_scale(H, ldh, pe, g, nu, s);
        if (rc) return rc;
    }
    if (!loglik) return DLSA_OK;
    rc = gamma_const(y, off, n, cpart, cst, s);
    if (rc) return rc;
    hipLaunchKernelGGL(gamma_ll_fix_kernel, dim3(1), dim3(64), 0, s, loglik, (const double*)cst, nu, gamma_ll_const(nu, n));
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

struct GammaLayout {
    CountScratchOff sc;
    size_t off_cpart, off_cst, off_dpart, off_dst, off_w, off_mu, off_y, off_o, off_gram, total;
};

// pass scratch; row_step > 1: room for the gathered responses and offsets of a strided partition
static GammaLayout gamma_layout(int64_t max_rows, int p, int64_t row_step) {
    GammaLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.sc = count_scratch_take(take, p);
    l.off_cpart = take(8 * (size_t)GAMMA_NC * GAMMA_SUM_BLOCKS);
    l.off_cst = take(8 * 4);
    l.off_dpart = take(8 * (size_t)GAMMA_ND * GAMMA_SUM_BLOCKS);
    l.off_dst = take(8 * 4);
    l.off_w = take(8 * (size_t)n);
    l.off_mu = take(8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_gram = take(gram_workspace_bytes_impl(n, p, 8));
    l.total = o;
    return l;
}

// One partition at a fixed beta and unit dispersion (count_pass with the Gamma row): w is r per row, loglik the sum of
// -(r + eta), mu (nullable) mu per row.
static int gamma_pass_impl(const double* X, int64_t ldx, const double* y, const double* off, const double* beta, int64_t n, int p,
                           int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w, double* mu, char* ws,
                           const GammaLayout& l, hipStream_t s) {
    return count_pass(GammaRow{}, X, ldx, y, off, beta, n, p, intercept, H, ldh, g, loglik, w, mu, count_scratch_at(ws, l.sc),
                      ws + l.off_gram, l.total - l.off_gram, s);
}

// The driver of the Gamma fits (dense rows here, raw one-hot rows in onehot_gamma.hip): `eval` is the only part that knows the
// representation of the design; the iteration is newton_fit_loop (newton_fit.h).
int gamma_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host,
                   const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double dispersion_fixed, double tol,
                   int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                   double* loglik_host, double* dispersion_host, double* pearson_host, double* deviance_host, const GammaFitBufs& b,
                   const GammaEval& eval, hipStream_t s) {
    const bool fixed = dispersion_fixed > 0;
    if (!fixed) {
        for (int k = 0; k < K; ++k) {
            if (part_rows_host[k] > 0 && part_rows_host[k] <= pe) {
                set_error("%s: partition %d has %lld rows for %d coefficients: the estimated dispersion has no degrees of freedom",
                          who, k, (long long)part_rows_host[k], pe);
                return DLSA_ERR_INVALID;
            }
        }
    }
    int overall = DLSA_OK;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_rows_host[k];
        double* Hk = Sig_inv + (size_t)k * pe * pe;
        double* ck = coef + (size_t)k * pe;
        double* sk = Sig_invMcoef + (size_t)k * pe;
        int st_k = DLSA_PART_EMPTY, iters = 0;
        double ll = 0.0, phi = 0.0, d[GAMMA_ND] = {0.0, 0.0};
        if (nk > 0) {
            const double *yk, *ok;
            int rc = pois_gather_rows(y, offset, part_first_host[k], row_step, nk, b.ybuf, b.obuf, yk, ok, s);
            if (rc) return rc;
            rc = gamma_const(yk, ok, nk, b.cpart, b.cst, s);
            if (rc) return rc;
            double cst[GAMMA_NC];
            DLSA_HIP_CHECK(hipMemcpyAsync(cst, b.cst, sizeof(cst), hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            if (cst[GAMMA_BAD] > 0.0) {
                set_error("%s: partition %d has %.0f rows with a non-positive or non-finite response or a non-finite offset", who, k,
                          cst[GAMMA_BAD]);
                return DLSA_ERR_INVALID;
            }
            // the intercept starts at log(sum y e^-o / n), the exact MLE of the intercept-only model
            const double m0 = cst[GAMMA_YEO] / (double)nk;
            const double b0 = (icpt_col >= 0 && m0 > 0.0 && isfinite(m0)) ? log(m0) : 0.0;
            rc = pois_start(b.st.beta, pe, icpt_col, b0, s);
            if (rc) return rc;
            const NewtonDevice dev{b.st, Hk, pe, s};
            NewtonOutcome o;
            rc = newton_fit_loop(NEWTON_POISSON, tol, max_iter + 1,
                                 [&](bool&) { return eval(k, yk, ok, nk, b.st.beta, Hk, b.st.g, b.st.stats + 3, b.mu); }, dev,
                                 newton_no_hook, o);
            if (rc) return rc;
            st_k = o.status; iters = o.n_iter;
            // the dispersion of the point H was evaluated at: b.mu is that evaluation's
            rc = gamma_disp(yk, b.mu, nk, b.dpart, b.dst, s);
            if (rc) return rc;
            DLSA_HIP_CHECK(hipMemcpyAsync(d, b.dst, sizeof(d), hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            phi = fixed ? dispersion_fixed : d[GAMMA_PEARSON] / (double)(nk - pe);
            ll = o.ll;
            if (phi > 0.0 && isfinite(phi)) {              // (else: Sig_inv and loglik stay those of unit dispersion)
                const double nu = 1.0 / phi;
                rc = gamma_scale(Hk, pe, pe, nullptr, nu, s);
                if (rc) return rc;
                ll = nu * o.ll + gamma_ll_const(nu, nk) + (nu - 1.0) * cst[GAMMA_LOGY];
            }
        }
        const int rcf = newton_fit_finish(st_k, iters, ll, b.st.beta, pe, Hk, ck, sk, k, n_iter_host, status_host, loglik_host, overall, s);
        if (rcf) return rcf;
        if (dispersion_host) dispersion_host[k] = phi;
        if (pearson_host) pearson_host[k] = d[GAMMA_PEARSON];
        if (deviance_host) deviance_host[k] = d[GAMMA_DEV];
    }
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    return overall;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_gamma_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    if (p <= 0 || p + (intercept ? 1 : 0) > 2048 || max_rows < 0 || row_step < 1) return 0;
    return dlsa::align_up(dlsa::gamma_layout(max_rows, p, row_step).total, 256) + dlsa::newton_state_bytes(p + (intercept ? 1 : 0));
}

int dlsa_gamma_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, double dispersion,
                        int64_t n, int p, int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out,
                        double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && beta, "gamma_pass: null X, y or beta");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(n >= 1 && p > 0 && pe <= 2048 && ldx >= p && (!H || ldh >= pe), "gamma_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld",
                 (long long)n, p, (long long)ldx, (long long)ldh);
    DLSA_REQUIRE(dispersion > 0 && isfinite(dispersion), "gamma_pass: the dispersion must be positive and finite");
    const GammaLayout l = gamma_layout(n, p, 1);
    // (the pass carves l.total of it; the contract is the query, which also holds a fit's Newton state)
    int rc = newton_check_ws("gamma_pass", ws, ws_bytes, dlsa_gamma_workspace_bytes(n, p, intercept, 1));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    double* mu = stats_out ? (double*)(wsc + l.off_mu) : nullptr;
    rc = gamma_pass_impl(X, ldx, y, offset, beta, n, p, intercept, H, ldh, g, loglik, w, mu, wsc, l, s);
    if (rc) return rc;
    return gamma_pass_finish(y, offset, mu, n, pe, dispersion, H, ldh, g, loglik, stats_out, (double*)(wsc + l.off_cpart),
                             (double*)(wsc + l.off_cst), (double*)(wsc + l.off_dpart), s);
}

int dlsa_gamma_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                       const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double dispersion_fixed,
                       double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host,
                       int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host, double* deviance_host,
                       void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "gamma_fit: null argument");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(K > 0 && p > 0 && pe <= 2048 && ldx >= p && row_step >= 1, "gamma_fit: bad shape K=%d p=%d ldx=%lld step=%lld", K, p,
                 (long long)ldx, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "gamma_fit: bad tol/max_iter");
    DLSA_REQUIRE(!(dispersion_fixed > 0) || isfinite(dispersion_fixed), "gamma_fit: a fixed dispersion must be finite");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "gamma_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const GammaLayout l = gamma_layout(max_rows, p, row_step);
    const size_t need = dlsa_gamma_workspace_bytes(max_rows, p, intercept, row_step);
    const int rcw = newton_check_ws("gamma_fit", ws, ws_bytes, need);
    if (rcw) return rcw;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    GammaFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.dpart = (double*)(wsc + l.off_dpart); b.dst = (double*)(wsc + l.off_dst);
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.mu = (double*)(wsc + l.off_mu);
    b.st = newton_state_at(wsc + align_up(l.total, 256), pe);
    double* wv = (double*)(wsc + l.off_w);
    const int64_t pitch = ldx * row_step;                     // rows first, first + step, ...: a strided view, no copy of X
    const GammaEval eval = [=](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* Hk, double* g,
                               double* ll, double* mu) {
        return gamma_pass_impl(X + part_first_host[k] * ldx, pitch, yk, ok, beta, nk, p, intercept, Hk, pe, g, ll, wv, mu, wsc, l, s);
    };
    return gamma_fit_core("gamma_fit", y, offset, part_first_host, part_rows_host, row_step, K, pe, intercept ? 0 : -1, dispersion_fixed,
                          tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, dispersion_host,
                          pearson_host, deviance_host, b, eval, s);
}

}  // extern "C"
