// Negative-binomial (NB2) regression map step for overdispersed counts (log link, optional offsets / exposure, estimated or
// fixed dispersion): one partition's log-likelihood, score and Fisher information at a fixed (beta, alpha), the dispersion
// terms at a fixed theta = 1 / alpha, and the per-partition fit that alternates the two.  The block a partition returns
// (coef, Sig_inv = the information about beta at (coef, alpha), Sig_inv coef) feeds the unchanged one-round combine: beta and
// alpha are information-orthogonal in NB2, so the beta block needs no cross term.
//
// Algebra (one partition; D = [1 | X] with the implicit intercept, X otherwise; o = offset, 0 when absent; theta = 1/alpha):
//   eta = D beta + o,  mu = exp(eta),  L = log1p(alpha mu),  q = 1 / (1 + alpha mu),
//   loglik = sum [ y eta - (y + theta) L ]                                           (the row pass)
//          + sum [ lgamma(y + theta) - lgamma(theta) - y log(theta) - lgamma(y + 1) ] (beta-free: the theta step)
//   g = D'[(y - mu) q],  H = D' diag(mu q) D    (expected information),
//   s(theta) = sum [ psi(y+theta) - psi(theta) - L + (mu - y) alpha q ]                         = d loglik / d theta
//   i(theta) = sum [ psi'(theta) - psi'(y+theta) - alpha + alpha q (2 - (1 + alpha y) q) ]      = -d2 loglik / d theta2
// (s and i are the textbook forms with log(theta) + 1 - log(theta + mu) - (y+theta)/(mu+theta) and -1/theta + 2/(mu+theta)
// - (y+theta)/(mu+theta)^2 rewritten in alpha, so every term is O(alpha) as theta grows and nothing is formed at theta itself).
//
// Launches per evaluation at (beta, alpha) (every partial combines in a fixed order: no float atomics):
//   1 count_pass_kernel     (count_pass.h, shared with poisson.hip: rowdot.h, RB rows per wave, non-temporal 16-byte loads, any row
//                           pitch) with the terms of NbRow (negbin_internal.h): w = mu q (-> the Gram's weights), mu (-> the theta step), per-block partials
//                           of g, sum (y - mu) q, sum y eta - (y + theta) L and, with the intercept and H wanted, X'w and sum w;
//   2 logit_finish_launch   the fixed-order column sums (shared with logit.hip / poisson.hip);
//   3 the Gram              dlsa_gram_f64's dispatch on (X, w).
// The theta step reads y and mu only (16 bytes per row): negbin_theta_kernel + its finish, once per Newton iteration on log theta.
//
// Range: mu = exp_full(eta) is finite up to eta = 709.78 and 0 below -746.  alpha mu overflows before mu does; the kernel then
// takes w = 1 / alpha, q = 0 and L = eta + log(alpha) (exact to 2^-53 once alpha mu > 2^53), so w, g and loglik are finite for
// every eta <= 709.78 and every alpha.  Above that mu = +inf and loglik = -inf: the driver's failed step, as in the Poisson fit.
#include "common.h"
#include "poisson_internal.h"
#include "negbin_internal.h"   // NbRow, the NB_* sums, nb_fit_core (shared with onehot_negbin.hip)
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"          // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "poisson_exp.h"     // exp_full
#include "negbin_special.h"  // nb_gamma_parts, nb_diffs
#include "count_pass.h"      // count_pass_kernel, count_pass, CountScratch

// ---- the dispersion step: the NB_NQ sums over (y, mu) at one theta -----------------------------------------------------
// alpha = 0 (the fit's look at the Poisson MLE) skips the special functions: only Pearson, the two moment sums and the check.
// want_lg: also sum lgamma(y + 1) (theta-free: the fit asks once per partition).  off (nullable) is read for the data check only.
__global__ __launch_bounds__(256) void negbin_theta_kernel(const double* __restrict__ y, const double* __restrict__ mu,
                                                           const double* __restrict__ off, int64_t n, double alpha, double theta,
                                                           int want_lg, double* __restrict__ part) {
    __shared__ double red[4][NB_NQ];
    double acc[NB_NQ];
#pragma unroll
    for (int j = 0; j < NB_NQ; ++j) acc[j] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yv = y[i], m = mu[i], ov = off ? off[i] : 0.0;
        if (!(yv >= 0.0 && isfinite(yv) && isfinite(ov))) { acc[NB_BAD] += 1.0; continue; }     // (NaN fails yv >= 0)
        const double d = yv - m, d2 = d * d;
        const double den = m * fma(alpha, m, 1.0);
        acc[NB_PEARSON] += den > 0.0 ? d2 / den : (yv > 0.0 ? INFINITY : 0.0);
        acc[NB_D0] += d2 - yv;
        acc[NB_M1] += d2 - m;
        acc[NB_M2] = fma(m, m, acc[NB_M2]);
        if (want_lg) acc[NB_LG] += lgamma(yv + 1.0);
        if (alpha > 0.0) {
            double D1, D2, C;
            nb_diffs(yv, theta, alpha, D1, D2, C);
            const double amu = alpha * m;
            const bool big = !(amu <= 1e300);
            const double q = big ? 0.0 : 1.0 / (1.0 + amu);
            const double L = amu < 9007199254740992.0 ? log1p(amu) : (m < INFINITY ? log(m) + log(alpha) : INFINITY);
            const double aq = alpha * q;
            acc[NB_C] += C;
            acc[NB_YL] += (yv + theta) * L;
            acc[NB_S] += D1 - L + (big ? 1.0 : (m - yv) * aq);              // (mu - y) / (mu + theta) -> 1
            acc[NB_I] += D2 - alpha + aq * (2.0 - fma(alpha, yv, 1.0) * q);
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NB_NQ; ++j) {
        const double t = wave_allreduce_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) red[wave][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < NB_NQ) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) t += red[k][threadIdx.x];
        part[(int64_t)blockIdx.x * NB_NQ + threadIdx.x] = t;
    }
}

// one wave per quantity, the block partials in a fixed order
__global__ __launch_bounds__(64 * NB_NQ) void negbin_theta_finish_kernel(const double* __restrict__ part, int nblocks,
                                                                         double* __restrict__ out) {
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int b = lane; b < nblocks; b += 64) s += part[(int64_t)b * NB_NQ + j];
    s = wave_allreduce_sum(s);
    if (lane == 0) out[j] = s;
}

// the pass entry's full log-likelihood: the row sum plus c(theta) (NaN when a row is not a valid count)
__global__ void negbin_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ tst) {
    if (threadIdx.x == 0) ll[0] = tst[NB_BAD] > 0.0 ? NAN : ll[0] + (tst[NB_C] - tst[NB_LG]);
}

// test entry: out[4 i ..] = psi(theta_i), psi'(theta_i), psi(y_i + theta_i) - psi(theta_i), lgamma(y_i + theta_i) - lgamma(theta_i) - y_i log theta_i
__global__ void negbin_special_kernel(const double* __restrict__ theta, const double* __restrict__ y, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double D1, D2, C;
    nb_diffs(y[i], theta[i], 1.0 / theta[i], D1, D2, C);
    out[4 * i] = nb_digamma(theta[i]);
    out[4 * i + 1] = nb_trigamma(theta[i]);
    out[4 * i + 2] = D1;
    out[4 * i + 3] = C;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct NbLayout {
    CountScratchOff sc;
    size_t off_y, off_o, off_pois, off_tpart, off_tst, off_w, off_mu, off_gram, off_state, total;
};

// [gathered counts | gathered offsets] of a strided partition, then the Poisson start's workspace (pois_bytes; 0 for the pass)
// overlaid with the NB scratch: the two never run at the same time
static NbLayout nb_layout(int64_t max_rows, int p, int intercept, int64_t row_step, size_t pois_bytes) {
    NbLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    const int pe = p + (intercept ? 1 : 0);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_pois = o;
    l.sc = count_scratch_take(take, p);
    l.off_tpart = take(8 * (size_t)NB_NQ * NB_THETA_BLOCKS);
    l.off_tst = take(8 * 16);
    l.off_w = take(8 * (size_t)n);
    l.off_mu = take(8 * (size_t)n);
    l.off_state = take(newton_state_bytes(pe));
    l.off_gram = take(gram_workspace_bytes_impl(n, p, 8));
    l.total = std::max(o, align_up(l.off_pois + pois_bytes, 256));
    return l;
}

// One partition at a fixed (beta, alpha) (count_pass with the NB2 row): w is mu q per row, loglik the row sum of
// y eta - (y + theta) L, without c(theta).
static int nb_pass_impl(const double* X, int64_t ldx, const double* y, const double* off, const double* beta, double alpha, int64_t n,
                        int p, int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w, double* mu, char* ws,
                        const NbLayout& l, hipStream_t s) {
    return count_pass(NbRow{alpha, 1.0 / alpha, log(alpha)}, X, ldx, y, off, beta, n, p, intercept, H, ldh, g, loglik, w, mu,
                      count_scratch_at(ws, l.sc), ws + l.off_gram, l.total - l.off_gram, s);
}

// the NB_NQ sums at theta = 1 / alpha (alpha = 0: no special functions) into tst (device)
int nb_theta_launch(const double* y, const double* mu, const double* off, int64_t n, double alpha, int want_lg, double* tpart,
                    double* tst, hipStream_t s) {
    const int blocks = (int)std::min<int64_t>(NB_THETA_BLOCKS, std::max<int64_t>(1, (n + 255) / 256));
    hipLaunchKernelGGL(negbin_theta_kernel, dim3(blocks), dim3(256), 0, s, y, mu, off, n, alpha, 1.0 / alpha, want_lg, tpart);
    hipLaunchKernelGGL(negbin_theta_finish_kernel, dim3(1), dim3(64 * NB_NQ), 0, s, (const double*)tpart, blocks, tst);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int nb_ll_fix(double* ll, const double* tst, hipStream_t s) {
    hipLaunchKernelGGL(negbin_ll_fix_kernel, dim3(1), dim3(64), 0, s, ll, tst);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

constexpr double NB_ALPHA_START_MIN = 1e-3;     // floor of the moment start
constexpr double NB_ALPHA_POISSON = 1e-8;       // the theta iteration below this alpha: the partition is Poisson (alpha = 0)

struct NbFitCtx : NewtonState {                // (stats, beta, prev, delta, g, Lf: the Newton state)
    const double* yk; const double* ok; int64_t nk;
    double tol;
    double* w; double* mu; double* tpart; double* tst;
    hipStream_t s;
};

static int nb_theta_eval(const NbFitCtx& c, double alpha, int want_lg, double* t) {
    const int rc = nb_theta_launch(c.yk, c.mu, nullptr, c.nk, alpha, want_lg, c.tpart, c.tst, c.s);
    if (rc) return rc;
    DLSA_HIP_CHECK(hipMemcpyAsync(t, c.tst, NB_NQ * sizeof(double), hipMemcpyDeviceToHost, c.s));
    DLSA_HIP_CHECK(hipStreamSynchronize(c.s));
    return DLSA_OK;
}

// Newton on log theta at the current mu: step s / (i theta), clamped to [-1, 1]; stops (without stepping) at |step| <= 100 tol, or
// where the step has stopped shrinking below 1e-8 (the rounding floor of the score).  t holds the sums at the returned alpha,
// first_step the size of the first step (0 <=> alpha did not move), yl_first sum (y + theta) L at the alpha it came in with.
// poisson = true: alpha fell below NB_ALPHA_POISSON.
static int nb_theta_solve(const NbFitCtx& c, double& alpha, double* t, int& theta_iters, bool& poisson, double& first_step,
                          double& yl_first) {
    double prev_step = INFINITY;
    poisson = false;
    first_step = 0.0;
    for (int it = 0; it < 60; ++it) {
        const int rc = nb_theta_eval(c, alpha, 0, t);
        if (rc) return rc;
        ++theta_iters;
        if (it == 0) yl_first = t[NB_YL];
        const double theta = 1.0 / alpha;
        double step = t[NB_S] / (t[NB_I] * theta);
        if (!(t[NB_I] > 0.0) || !isfinite(step)) step = t[NB_S] > 0.0 ? 1.0 : -1.0;
        step = std::min(1.0, std::max(-1.0, step));
        const double as = fabs(step);
        if (it == 0) first_step = as;
        if (as <= 100.0 * c.tol || (as <= 1e-8 && as >= 0.5 * prev_step)) return DLSA_OK;
        prev_step = as;
        alpha *= exp(-step);                                  // log theta += step
        if (alpha < NB_ALPHA_POISSON) { poisson = true; return DLSA_OK; }
    }
    return DLSA_OK;
}

// The per-partition driver of the NB2 fits (negbin_internal.h): the dense entry below and the structured one (onehot_negbin.hip)
// differ in `pois` (the Poisson block of partition k) and `evalk` (the evaluation at (beta, alpha)) alone.
int nb_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host,
                int64_t row_step, int K, int pe, double alpha_fixed, double tol, int max_iter, double* coef, double* Sig_inv,
                double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, double* alpha_host,
                double* alpha_info_host, double* pearson_host, const NbFitBufs& b, const NbPoisFit& pois, const NbEval& evalk,
                hipStream_t s) {
    const bool fixed = alpha_fixed > 0;
    NbFitCtx c{};
    c.tol = tol;
    // (NbFitCtx derives from NewtonState so that the passes keep reading c.beta, c.g, ... while the carving has one copy)
    static_cast<NewtonState&>(c) = b.st;
    c.w = b.w; c.mu = b.mu; c.tpart = b.tpart; c.tst = b.tst;
    c.s = s;
    int overall = DLSA_OK;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_rows_host[k];
        double* Hk = Sig_inv + (size_t)k * pe * pe;
        double* ck = coef + (size_t)k * pe;
        double* sk = Sig_invMcoef + (size_t)k * pe;
        // 1. the Poisson fit of the partition: the start, the data check, the EMPTY block, and the answer where alpha = 0
        int st_k = DLSA_PART_EMPTY, iters = 0;
        double ll = 0.0, alpha = 0.0, info = 0.0, pearson = 0.0;
        int rc = pois(k, ck, Hk, sk, &iters, &st_k, &ll);
        if (rc == DLSA_ERR_INVALID) {
            set_error("%s: partition %d has rows with a negative or non-finite count or offset", who, k);
            return rc;
        }
        if (rc && rc != DLSA_ERR_NOT_CONVERGED && rc != DLSA_ERR_NOT_SPD && rc != DLSA_ERR_NAN) return rc;
        if (st_k == DLSA_PART_OK) {
            c.nk = nk;
            // the partition's counts and offsets, gathered once when it is strided
            rc = pois_gather_rows(y, offset, part_first_host[k], row_step, nk, b.ybuf, b.obuf, c.yk, c.ok, s);
            if (rc) return rc;
            DLSA_HIP_CHECK(hipMemcpyAsync(c.beta, ck, (size_t)pe * sizeof(double), hipMemcpyDeviceToDevice, s));
            // mu at the Poisson MLE (alpha = 0: the Poisson limit; no H, no g), then the moment sums
            rc = evalk(k, c.yk, c.ok, nk, c.beta, 0.0, nullptr, nullptr, nullptr, nullptr, c.mu);
            if (rc) return rc;
            int passes = 1, theta_iters = 0;
            double t[NB_NQ];
            rc = nb_theta_eval(c, 0.0, 1, t);
            if (rc) return rc;
            const double lg1 = t[NB_LG];
            pearson = t[NB_PEARSON];
            bool poisson = !fixed && !(t[NB_D0] > 0.0);        // 3. not overdispersed: the MLE is alpha = 0, the Poisson block stands
            if (!poisson) {
                alpha = fixed ? alpha_fixed : std::max(t[NB_M1] / t[NB_M2], NB_ALPHA_START_MIN);
                if (!isfinite(alpha)) alpha = NB_ALPHA_START_MIN;
                const int max_passes = max_iter + 2;
                double ll1 = 0.0, fs = 0.0, yl = 0.0;
                if (!fixed) {                                  // theta for the Poisson fit's mu
                    rc = nb_theta_solve(c, alpha, t, theta_iters, poisson, fs, yl);
                    if (rc) return rc;
                }
                if (!poisson) {
                    // The fit proper, from the Poisson MLE in c.beta and the start alpha, is newton_fit_loop with the policy
                    // NEWTON_NB2 and this hook: after every ACCEPTED evaluation at (beta, alpha) -- H, g, the row log-likelihood, w,
                    // mu -- theta is solved for that mu (16 bytes per row and iteration), then beta takes the Newton step that
                    // evaluation gave..  H is the expected information, so at alpha > 0 the beta iteration is Fisher scoring (linear
                    // convergence); one theta solve per step keeps the two in lockstep instead of nesting one iteration in the
                    // other..  A step is halved while the row log-likelihood at the SAME alpha drops or is not finite: the previous
                    // point's value is moved to the new alpha with sum (y + theta) L of its mu (ll_shift)..  Converged where the step of
                    // beta meets the IRLS rule and theta did not move (first_step): then H, g and t are at the returned (beta,
                    // alpha)..  fixed: no theta steps.
                    const auto eval = [&](bool&) {
                        return evalk(k, c.yk, c.ok, nk, c.beta, alpha, Hk, c.g, c.stats + 3, c.w, c.mu);
                    };
                    const auto theta_hook = [&](bool& leave, double& first_step, double& ll_shift) {
                        if (fixed) return (int)DLSA_OK;
                        double yl_old = 0.0;
                        const int rch = nb_theta_solve(c, alpha, t, theta_iters, poisson, first_step, yl_old);
                        leave = poisson;                           // alpha fell to 0: the Poisson block, below
                        ll_shift = yl_old - t[NB_YL];              // this point's row log-likelihood at the new alpha
                        return rch;
                    };
                    NewtonOutcome o;
                    rc = newton_fit_loop(NEWTON_NB2, tol, max_passes - passes, eval, NewtonDevice{c, Hk, pe, s}, theta_hook, o);
                    if (rc) return rc;
                    passes += o.evals; ll1 = o.ll; st_k = o.status;
                }
                if (poisson && passes == 1) {                  // the dispersion iterate ran off to 0 before H was touched
                    alpha = 0.0;
                } else if (poisson) {                          // ... or later: the Poisson block again
                    rc = pois(k, ck, Hk, sk, nullptr, &st_k, &ll);
                    if (rc && rc != DLSA_ERR_NOT_CONVERGED && rc != DLSA_ERR_NOT_SPD && rc != DLSA_ERR_NAN) return rc;
                    alpha = 0.0;
                } else {
                    if (fixed && st_k == DLSA_PART_OK) {
                        rc = nb_theta_eval(c, alpha, 0, t);
                        if (rc) return rc;
                    }
                    ll = ll1 + (t[NB_C] - lg1);
                    info = t[NB_I] / (alpha * alpha);
                    pearson = t[NB_PEARSON];
                    DLSA_HIP_CHECK(hipMemcpyAsync(ck, c.beta, (size_t)pe * sizeof(double), hipMemcpyDeviceToDevice, s));
                    rc = launch_matvec(Hk, pe, c.beta, pe, sk, s);
                    if (rc) return rc;
                }
            }
            iters += passes;
        } else if (st_k != DLSA_PART_EMPTY) {
            alpha = NAN; info = NAN; pearson = NAN;
        }
        if (n_iter_host) n_iter_host[k] = iters;
        if (status_host) status_host[k] = st_k;
        if (loglik_host) loglik_host[k] = ll;
        if (alpha_host) alpha_host[k] = alpha;
        if (alpha_info_host) alpha_info_host[k] = info;
        if (pearson_host) pearson_host[k] = pearson;
        newton_fold_status(st_k, overall);
    }
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    return overall;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_negbin_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    if (p <= 0 || p + (intercept ? 1 : 0) > 2048 || max_rows < 0 || row_step < 1) return 0;
    const size_t pois = dlsa_poisson_workspace_bytes(max_rows, p, intercept, row_step);
    return dlsa::nb_layout(max_rows, p, intercept, row_step, pois).total;
}

int dlsa_negbin_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, double alpha,
                         int64_t n, int p, int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out,
                         double* mu_out, double* theta_terms, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && beta, "negbin_pass: null X, y or beta");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(n >= 1 && p > 0 && pe <= 2048 && ldx >= p && (!H || ldh >= pe), "negbin_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld",
                 (long long)n, p, (long long)ldx, (long long)ldh);
    DLSA_REQUIRE(alpha > 0 && isfinite(alpha), "negbin_pass: alpha must be positive and finite (alpha = 0 is dlsa_poisson_pass_f64)");
    const NbLayout l = nb_layout(n, p, intercept, 1, 0);
    int rc = newton_check_ws("negbin_pass", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    const bool want_theta = loglik || theta_terms;
    double* mu = mu_out ? mu_out : (want_theta ? (double*)(wsc + l.off_mu) : nullptr);
    rc = nb_pass_impl(X, ldx, y, offset, beta, alpha, n, p, intercept, H, ldh, g, loglik, w, mu, wsc, l, s);
    if (rc || !want_theta) return rc;
    double* tst = (double*)(wsc + l.off_tst);
    rc = nb_theta_launch(y, mu, offset, n, alpha, loglik ? 1 : 0, (double*)(wsc + l.off_tpart), tst, s);
    if (rc) return rc;
    if (theta_terms) DLSA_HIP_CHECK(hipMemcpyAsync(theta_terms, tst + NB_S, 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (loglik) return nb_ll_fix(loglik, tst, s);
    return DLSA_OK;
}

int dlsa_negbin_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                        const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double alpha_fixed, double tol,
                        int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                        double* loglik_host, double* alpha_host, double* alpha_info_host, double* pearson_host, void* ws,
                        size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "negbin_fit: null argument");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(K > 0 && p > 0 && pe <= 2048 && ldx >= p && row_step >= 1, "negbin_fit: bad shape K=%d p=%d ldx=%lld step=%lld", K, p,
                 (long long)ldx, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "negbin_fit: bad tol/max_iter");
    DLSA_REQUIRE(!(alpha_fixed > 0) || isfinite(alpha_fixed), "negbin_fit: a fixed alpha must be finite");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "negbin_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const size_t pois_bytes = dlsa_poisson_workspace_bytes(max_rows, p, intercept, row_step);
    const NbLayout l = nb_layout(max_rows, p, intercept, row_step, pois_bytes);
    const int rcw = newton_check_ws("negbin_fit", ws, ws_bytes, l.total);
    if (rcw) return rcw;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    NbFitBufs b{};
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.w = (double*)(wsc + l.off_w); b.mu = (double*)(wsc + l.off_mu);
    b.tpart = (double*)(wsc + l.off_tpart); b.tst = (double*)(wsc + l.off_tst);
    b.st = newton_state_at(wsc + l.off_state, pe);
    const int64_t pitch = ldx * row_step;
    const NbPoisFit pois = [=](int k, double* ck, double* Hk, double* sk, int* iters, int* st_k, double* ll) {
        return dlsa_poisson_fit_f64(X, ldx, y, offset, part_first_host + k, part_rows_host + k, row_step, 1, p, intercept, tol, max_iter,
                                    ck, Hk, sk, iters, st_k, ll, wsc + l.off_pois, l.total - l.off_pois, stream);
    };
    const NbEval eval = [=](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double alpha, double* H, double* g,
                            double* ll, double* w, double* mu) {
        return nb_pass_impl(X + part_first_host[k] * ldx, pitch, yk, ok, beta, alpha, nk, p, intercept, H, pe, g, ll, w, mu, wsc, l, s);
    };
    return nb_fit_core("negbin_fit", y, offset, part_first_host, part_rows_host, row_step, K, pe, alpha_fixed, tol, max_iter, coef,
                       Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, alpha_host, alpha_info_host, pearson_host, b, pois,
                       eval, s);
}

int dlsa_negbin_special_f64(const double* theta, const double* y, int64_t n, double* out, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(theta && y && out && n >= 1, "negbin_special: null argument or n < 1");
    hipLaunchKernelGGL(negbin_special_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, theta, y, n, out);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

}  // extern "C"
