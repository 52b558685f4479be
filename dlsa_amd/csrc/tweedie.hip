// Tweedie (compound Poisson-Gamma) regression map step, log link, variance power 1 < xi < 2 given by the caller, optional offsets /
// exposure, estimated or fixed dispersion: the family of a response that is exactly zero for many rows and positive, right-skewed
// for the rest (pure premium, cost per policy, rainfall).  One partition's quasi-log-likelihood, score and observed information at
// a fixed beta and dispersion, the Pearson and deviance sums, and the per-partition Newton fit on top of them.  The block a
// partition returns (coef, Sig_inv = the information at coef and the partition's dispersion, Sig_inv coef) feeds the unchanged
// one-round combine.
//
// Algebra (one partition; D = [1 | X] with the implicit intercept, X otherwise; o = offset, 0 when absent; nu = 1 / phi):
//   eta = D beta + o,  mu = exp(eta),  a = mu^(1 - xi) = exp((1 - xi) eta),  b = mu^(2 - xi) = mu a,
//   q = y a / (1 - xi) - b / (2 - xi),  loglik = nu sum q,
//   g = nu D'(y a - b),  H = nu D' diag((xi - 1) y a + (2 - xi) b) D   (the observed information: y >= 0 and a, b > 0, so every
//   weight is positive and the negative log-likelihood is convex in beta),
//   P = sum (y - mu)^2 mu^-xi,  Dev = 2 sum [y^(2 - xi) / ((1 - xi)(2 - xi)) - y a / (1 - xi) + b / (2 - xi)],  phi^ = P / (n - pe).
// loglik is the QUASI-log-likelihood: the part of the log density that depends on beta.  The series factor log a(y, phi, xi) of
// the Tweedie density is not computed, so loglik compares values of beta at one (xi, phi) only -- no AIC across xi, no profile of xi.
// beta^ does not depend on phi (it does on xi), so the row pass and the Newton loop run at nu = 1 with xi in the row model and the
// dispersion enters afterwards, as one scalar on H, g and loglik.
//
// a is exp of a rounded product; at |eta| = 300 that rounding alone is 3e-14 of a.  The rows take hi = (1 - xi) eta, lo = fma(1 - xi,
// eta, -hi), a = exp_full(hi) (1 + lo): one fma and one multiply, and a stays within an ulp or two of the exact value.
//
// Launches per evaluation (every partial combines in a fixed order: no float atomics, no waits between workgroups):
//   1 count_pass_kernel     (count_pass.h, unchanged, here with the terms of TweedieRow) one read of the rows: the weight (-> w, the
//                           Gram's weights), mu (-> the dispersion sums), per-block partials of g, sum (y a - b), sum q and, with
//                           the intercept and H wanted, of X'w and sum w;
//   2 logit_finish_launch   the fixed-order column sums of those partials (logit.hip, shared);
//   3 the Gram              dlsa_gram_f64's dispatch on (X, w) into the p x p block (gram_icpt_impl with the border).
// Once per partition: tweedie_const_kernel + the sum finish of gamma.hip (sum y e^((1 - xi) o) and sum e^((2 - xi) o) for the
// intercept's start, the data check, the count of positive responses).  Once per fit (and per pass that asks): tweedie_disp_kernel
// + the same finish over (y, mu), 16 bytes per row, and gamma.hip's scaling of the pe x pe block.
// The fit driver (tweedie_fit_core) takes the evaluation as a callable and is shared with the structured one-hot fit
// (onehot_tweedie.hip) through tweedie_internal.h; the Newton iteration is newton_fit.h's with the policy of the Poisson fit, the
// gather of a strided partition's responses and offsets poisson_internal.h's.
#include "common.h"
#include "poisson_internal.h"
#include "gamma_internal.h"
#include "tweedie_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"       // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "poisson_exp.h"  // exp_full
#include "count_pass.h"   // count_pass_kernel, count_pass, CountScratch

// the Tweedie row at unit dispersion (tweedie_row, tweedie_internal.h): weight (xi - 1) y a + (2 - xi) b, residual y a - b, term
// y a / (1 - xi) - b / (2 - xi)
struct TweedieRow {
    static constexpr bool STORES_MU = true;
    double one_m_xi, two_m_xi;
    double inv_one, inv_two;            // 1 / (1 - xi), 1 / (2 - xi)
    __device__ __forceinline__ void terms(double yv, double eta, double mu, double& wgt, double& rs, double& llt) const {
        double ya, b;
        tweedie_row(one_m_xi, two_m_xi, yv, eta, mu, ya, b, wgt);
        rs = ya - b;
        llt = fma(ya, inv_one, -(b * inv_two));
    }
};

static TweedieRow tweedie_row_model(double power) {
    const double c1 = 1.0 - power, c2 = 2.0 - power;
    return TweedieRow{c1, c2, 1.0 / c1, 1.0 / c2};
}

// ---- once per partition: [sum y e^((1 - xi) o), sum e^((2 - xi) o), rows with y < 0 or a non-finite y / o, rows with y > 0] ---
__global__ __launch_bounds__(256) void tweedie_const_kernel(const double* __restrict__ y, const double* __restrict__ off, int64_t n,
                                                            double one_m_xi, double* __restrict__ part) {
    __shared__ double red[4][TWEEDIE_NC];
    double acc[TWEEDIE_NC] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yv = y[i], ov = off ? off[i] : 0.0;
        if (yv >= 0.0 && isfinite(yv) && isfinite(ov)) {      // (NaN fails yv >= 0)
            const double e1 = tweedie_exp_prod(one_m_xi, ov);
            acc[TWEEDIE_YEO] = fma(yv, e1, acc[TWEEDIE_YEO]);
            acc[TWEEDIE_EO] += e1 * exp_full(ov);
            acc[TWEEDIE_POS] += yv > 0.0 ? 1.0 : 0.0;
        } else {
            acc[TWEEDIE_BAD] += 1.0;
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < TWEEDIE_NC; ++j) {
        const double t = wave_allreduce_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) red[wave][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < TWEEDIE_NC) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) t += red[k][threadIdx.x];
        part[(int64_t)blockIdx.x * TWEEDIE_NC + threadIdx.x] = t;
    }
}

// ---- the dispersion sums over (y, mu): [sum (y - mu)^2 mu^-xi, 2 sum (y^(2 - xi) / ((1 - xi)(2 - xi)) - y a / (1 - xi) + b / (2 - xi))]
// a = mu^(1 - xi) = exp((1 - xi) log mu).  A row with y = 0 has y^(2 - xi) = 0 exactly: the power is taken of 1 in its place and
// the result selected away, so no log(0) is formed and no lane branches.
__global__ __launch_bounds__(256) void tweedie_disp_kernel(const double* __restrict__ y, const double* __restrict__ mu, int64_t n,
                                                           double one_m_xi, double two_m_xi, double* __restrict__ part) {
    __shared__ double red[4][TWEEDIE_ND];
    const double inv_one = 1.0 / one_m_xi, inv_two = 1.0 / two_m_xi, inv_both = inv_one * inv_two;
    double ps = 0.0, dv = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yv = y[i], m = mu[i];
        const double a = tweedie_exp_prod(one_m_xi, log(m));
        const double b = m * a, d = yv - m;
        ps = fma(d * d, a / m, ps);
        const bool pos = yv > 0.0;
        const double yp = tweedie_exp_prod(two_m_xi, log(pos ? yv : 1.0));
        dv += fma(pos ? yp : 0.0, inv_both, fma(b, inv_two, -(yv * a * inv_one)));
    }
    ps = wave_allreduce_sum(ps);
    dv = wave_allreduce_sum(dv);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][GAMMA_PEARSON] = ps; red[wave][GAMMA_DEV] = dv; }
    __syncthreads();
    if (threadIdx.x < TWEEDIE_ND) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) t += red[k][threadIdx.x];
        part[(int64_t)blockIdx.x * TWEEDIE_ND + threadIdx.x] = threadIdx.x == GAMMA_DEV ? 2.0 * t : t;
    }
}

// the pass entry's quasi-log-likelihood from the row sum of q: nu ll (NaN when a row is not a valid response)
__global__ void tweedie_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ cst, double nu) {
    if (threadIdx.x == 0) ll[0] = cst[TWEEDIE_BAD] > 0.0 ? NAN : nu * ll[0];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int tweedie_const(const double* y, const double* off, int64_t n, double power, double* cpart, double* cst, hipStream_t s) {
    const int blocks = gamma_sum_blocks(n);
    hipLaunchKernelGGL(tweedie_const_kernel, dim3(blocks), dim3(256), 0, s, y, off, n, 1.0 - power, cpart);
    return gamma_sum_finish(cpart, blocks, TWEEDIE_NC, cst, s);
}

int tweedie_disp(const double* y, const double* mu, int64_t n, double power, double* dpart, double* dst, hipStream_t s) {
    const int blocks = gamma_sum_blocks(n);
    hipLaunchKernelGGL(tweedie_disp_kernel, dim3(blocks), dim3(256), 0, s, y, mu, n, 1.0 - power, 2.0 - power, dpart);
    return gamma_sum_finish(dpart, blocks, TWEEDIE_ND, dst, s);
}

int tweedie_pass_finish(const double* y, const double* off, const double* mu, int64_t n, int pe, double power, double dispersion,
                        double* H, int64_t ldh, double* g, double* loglik, double* stats_out, double* cpart, double* cst,
                        double* dpart, hipStream_t s) {
    const double nu = 1.0 / dispersion;
    int rc = DLSA_OK;
    if (stats_out) {
        rc = tweedie_disp(y, mu, n, power, dpart, stats_out, s);
        if (rc) return rc;
    }
    if (nu != 1.0) {
        rc = gamma_scale(H, ldh, pe, g, nu, s);
        if (rc) return rc;
    }
    if (!loglik) return DLSA_OK;
    rc = tweedie_const(y, off, n, power, cpart, cst, s);
    if (rc) return rc;
    hipLaunchKernelGGL(tweedie_ll_fix_kernel, dim3(1), dim3(64), 0, s, loglik, (const double*)cst, nu);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

struct TweedieLayout {
    CountScratchOff sc;
    size_t off_cpart, off_cst, off_dpart, off_dst, off_w, off_mu, off_y, off_o, off_gram, total;
};

// pass scratch; row_step > 1: room for the gathered responses and offsets of a strided partition
static TweedieLayout tweedie_layout(int64_t max_rows, int p, int64_t row_step) {
    TweedieLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.sc = count_scratch_take(take, p);
    l.off_cpart = take(8 * (size_t)TWEEDIE_NC * GAMMA_SUM_BLOCKS);
    l.off_cst = take(8 * 4);
    l.off_dpart = take(8 * (size_t)TWEEDIE_ND * GAMMA_SUM_BLOCKS);
    l.off_dst = take(8 * 4);
    l.off_w = take(8 * (size_t)n);
    l.off_mu = take(8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_gram = take(gram_workspace_bytes_impl(n, p, 8));
    l.total = o;
    return l;
}

// One partition at a fixed beta and unit dispersion (count_pass with the Tweedie row): w is the weight per row, loglik the sum of
// q, mu (nullable) mu per row.
static int tweedie_pass_impl(double power, const double* X, int64_t ldx, const double* y, const double* off, const double* beta,
                             int64_t n, int p, int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w,
                             double* mu, char* ws, const TweedieLayout& l, hipStream_t s) {
    return count_pass(tweedie_row_model(power), X, ldx, y, off, beta, n, p, intercept, H, ldh, g, loglik, w, mu, count_scratch_at(ws, l.sc),
                      ws + l.off_gram, l.total - l.off_gram, s);
}

// The driver of the Tweedie fits (dense rows here, raw one-hot rows in onehot_tweedie.hip): `eval` is the only part that knows the
// representation of the design; the iteration is newton_fit_loop (newton_fit.h).
int tweedie_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host,
                     const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double power,
                     double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                     int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host,
                     double* deviance_host, const TweedieFitBufs& b, const TweedieEval& eval, hipStream_t s) {
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
        double ll = 0.0, phi = 0.0, d[TWEEDIE_ND] = {0.0, 0.0};
        if (nk > 0) {
            const double *yk, *ok;
            int rc = pois_gather_rows(y, offset, part_first_host[k], row_step, nk, b.ybuf, b.obuf, yk, ok, s);
            if (rc) return rc;
            rc = tweedie_const(yk, ok, nk, power, b.cpart, b.cst, s);
            if (rc) return rc;
            double cst[TWEEDIE_NC];
            DLSA_HIP_CHECK(hipMemcpyAsync(cst, b.cst, sizeof(cst), hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            if (cst[TWEEDIE_BAD] > 0.0) {
                set_error("%s: partition %d has %.0f rows with a negative or non-finite response or a non-finite offset", who, k,
                          cst[TWEEDIE_BAD]);
                return DLSA_ERR_INVALID;
            }
            if (!(cst[TWEEDIE_POS] > 0.0)) {
                set_error("%s: partition %d has no positive response: its maximum-likelihood fit runs off to mu = 0", who, k);
                return DLSA_ERR_INVALID;
            }
            // the intercept starts at log(sum y e^((1 - xi) o) / sum e^((2 - xi) o)), the exact MLE of the intercept-only model
            const double m0 = cst[TWEEDIE_YEO] / cst[TWEEDIE_EO];
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
            rc = tweedie_disp(yk, b.mu, nk, power, b.dpart, b.dst, s);
            if (rc) return rc;
            DLSA_HIP_CHECK(hipMemcpyAsync(d, b.dst, sizeof(d), hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            phi = fixed ? dispersion_fixed : d[GAMMA_PEARSON] / (double)(nk - pe);
            ll = o.ll;
            if (phi > 0.0 && isfinite(phi)) {              // (else: Sig_inv and loglik stay those of unit dispersion)
                const double nu = 1.0 / phi;
                rc = gamma_scale(Hk, pe, pe, nullptr, nu, s);
                if (rc) return rc;
                ll = nu * o.ll;
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

size_t dlsa_tweedie_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    if (p <= 0 || p + (intercept ? 1 : 0) > 2048 || max_rows < 0 || row_step < 1) return 0;
    return dlsa::align_up(dlsa::tweedie_layout(max_rows, p, row_step).total, 256) + dlsa::newton_state_bytes(p + (intercept ? 1 : 0));
}

int dlsa_tweedie_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, double power,
                          double dispersion, int64_t n, int p, int intercept, double* H, int64_t ldh, double* g, double* loglik,
                          double* w_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && beta, "tweedie_pass: null X, y or beta");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(n >= 1 && p > 0 && pe <= 2048 && ldx >= p && (!H || ldh >= pe), "tweedie_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld",
                 (long long)n, p, (long long)ldx, (long long)ldh);
    DLSA_REQUIRE(tweedie_power_ok(power), "tweedie_pass: the variance power must lie strictly between 1 and 2");
    DLSA_REQUIRE(dispersion > 0 && isfinite(dispersion), "tweedie_pass: the dispersion must be positive and finite");
    const TweedieLayout l = tweedie_layout(n, p, 1);
    // (the pass carves l.total of it; the contract is the query, which also holds a fit's Newton state)
    int rc = newton_check_ws("tweedie_pass", ws, ws_bytes, dlsa_tweedie_workspace_bytes(n, p, intercept, 1));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    double* mu = stats_out ? (double*)(wsc + l.off_mu) : nullptr;
    rc = tweedie_pass_impl(power, X, ldx, y, offset, beta, n, p, intercept, H, ldh, g, loglik, w, mu, wsc, l, s);
    if (rc) return rc;
    return tweedie_pass_finish(y, offset, mu, n, pe, power, dispersion, H, ldh, g, loglik, stats_out, (double*)(wsc + l.off_cpart),
                               (double*)(wsc + l.off_cst), (double*)(wsc + l.off_dpart), s);
}

int dlsa_tweedie_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double power,
                         double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                         int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host,
                         double* deviance_host, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "tweedie_fit: null argument");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(K > 0 && p > 0 && pe <= 2048 && ldx >= p && row_step >= 1, "tweedie_fit: bad shape K=%d p=%d ldx=%lld step=%lld", K, p,
                 (long long)ldx, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "tweedie_fit: bad tol/max_iter");
    DLSA_REQUIRE(tweedie_power_ok(power), "tweedie_fit: the variance power must lie strictly between 1 and 2");
    DLSA_REQUIRE(!(dispersion_fixed > 0) || isfinite(dispersion_fixed), "tweedie_fit: a fixed dispersion must be finite");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "tweedie_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const TweedieLayout l = tweedie_layout(max_rows, p, row_step);
    const size_t need = dlsa_tweedie_workspace_bytes(max_rows, p, intercept, row_step);
    const int rcw = newton_check_ws("tweedie_fit", ws, ws_bytes, need);
    if (rcw) return rcw;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    TweedieFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.dpart = (double*)(wsc + l.off_dpart); b.dst = (double*)(wsc + l.off_dst);
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.mu = (double*)(wsc + l.off_mu);
    b.st = newton_state_at(wsc + align_up(l.total, 256), pe);
    double* wv = (double*)(wsc + l.off_w);
    const int64_t pitch = ldx * row_step;                     // rows first, first + step, ...: a strided view, no copy of X
    const TweedieEval eval = [=](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* Hk, double* g,
                                 double* ll, double* mu) {
        return tweedie_pass_impl(power, X + part_first_host[k] * ldx, pitch, yk, ok, beta, nk, p, intercept, Hk, pe, g, ll, wv, mu, wsc, l, s);
    };
    return tweedie_fit_core("tweedie_fit", y, offset, part_first_host, part_rows_host, row_step, K, pe, intercept ? 0 : -1, power,
                            dispersion_fixed, tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host,
                            dispersion_host, pearson_host, deviance_host, b, eval, s);
}

}  // extern "C"
