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
// Once per partition: tweedie_const_kernel + block_sum_finish_kernel (sum y e^((1 - xi) o) and sum e^((2 - xi) o) for the
// intercept's start, the data check, the count of positive responses).  Once per fit (and per pass that asks): tweedie_disp_kernel
// + the same finish over (y, mu), 16 bytes per row, and disp_scale_kernel on the pe x pe block.
// This file holds what is the Tweedie family's: the row model, the two sum kernels, the log-likelihood and the record that hands
// them to the driver of the dispersion families (dispersion.hip, dispersion_internal.h), which owns the entries' bodies, the
// workspace and the fit; onehot_tweedie.hip brings the same record with its own row pass and shares the row's arithmetic through
// tweedie_internal.h.
#include "common.h"
#include "poisson_internal.h"
#include "dispersion_internal.h"
#include "tweedie_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"       // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "poisson_exp.h"  // exp_full
#include "count_pass.h"   // count_pass_kernel, count_pass, CountScratch

// once per partition, TWEEDIE_NC sums: [sum y e^((1 - xi) o), sum e^((2 - xi) o), rows with y < 0 or a non-finite y / o, rows with y > 0]
enum { TWEEDIE_YEO = 0, TWEEDIE_EO = 1, TWEEDIE_BAD = 2, TWEEDIE_POS = 3 };

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

// ---- once per partition: the TWEEDIE_NC sums ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tweedie_const_kernel(const double* __restrict__ y, const double* __restrict__ off, int64_t n,
                                                            double one_m_xi, double* __restrict__ part) {
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
    block_partials_store(acc, part);
}

// ---- the dispersion sums over (y, mu): [sum (y - mu)^2 mu^-xi, 2 sum (y^(2 - xi) / ((1 - xi)(2 - xi)) - y a / (1 - xi) + b / (2 - xi))]
// a = mu^(1 - xi) = exp((1 - xi) log mu).  A row with y = 0 has y^(2 - xi) = 0 exactly: the power is taken of 1 in its place and
// the result selected away, so no log(0) is formed and no lane branches.
__global__ __launch_bounds__(256) void tweedie_disp_kernel(const double* __restrict__ y, const double* __restrict__ mu, int64_t n,
                                                           double one_m_xi, double two_m_xi, double* __restrict__ part) {
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
    const double acc[DISP_ND] = {ps, 2.0 * dv};               // (the doubling is exact, so it commutes with the sums)
    block_partials_store(acc, part);
}

// the pass entry's quasi-log-likelihood from the row sum of q: nu ll (NaN when a row is not a valid response)
__global__ void tweedie_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ cst, double nu) {
    if (threadIdx.x == 0) ll[0] = cst[TWEEDIE_BAD] > 0.0 ? NAN : nu * ll[0];
}

// ---- host side: the family record ------------------------------------------------------------------------------------------
static int tweedie_const(const DispFamily& f, const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s) {
    const int blocks = disp_sum_blocks(n);
    hipLaunchKernelGGL(tweedie_const_kernel, dim3(blocks), dim3(256), 0, s, y, off, n, 1.0 - f.power, cpart);
    return block_sum_finish(cpart, blocks, TWEEDIE_NC, cst, s);
}

static int tweedie_disp(const DispFamily& f, const double* y, const double* mu, int64_t n, double* dpart, double* dst, hipStream_t s) {
    const int blocks = disp_sum_blocks(n);
    hipLaunchKernelGGL(tweedie_disp_kernel, dim3(blocks), dim3(256), 0, s, y, mu, n, 1.0 - f.power, 2.0 - f.power, dpart);
    return block_sum_finish(dpart, blocks, DISP_ND, dst, s);
}

static int tweedie_check(const char* who, int k, const double* cst) {
    if (cst[TWEEDIE_BAD] > 0.0) {
        set_error("%s: partition %d has %.0f rows with a negative or non-finite response or a non-finite offset", who, k,
                  cst[TWEEDIE_BAD]);
        return DLSA_ERR_INVALID;
    }
    if (!(cst[TWEEDIE_POS] > 0.0)) {
        set_error("%s: partition %d has no positive response: its maximum-likelihood fit runs off to mu = 0", who, k);
        return DLSA_ERR_INVALID;
    }
    return DLSA_OK;
}

// sum y e^((1 - xi) o) / sum e^((2 - xi) o)
static double tweedie_start_mean(const double* cst, int64_t) { return cst[TWEEDIE_YEO] / cst[TWEEDIE_EO]; }

// (not the Gamma expression with zero coefficients: cst[0] can be infinite here, and 0 * inf would make a finite result NaN)
static double tweedie_loglik(double nu, double ll, const double*, int64_t) { return nu * ll; }

static int tweedie_ll_fix(double* ll, const double* cst, double nu, int64_t, hipStream_t s) {
    hipLaunchKernelGGL(tweedie_ll_fix_kernel, dim3(1), dim3(64), 0, s, ll, cst, nu);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

DispFamily tweedie_family(double power) {
    // 1 < power < 2 (a NaN fails both comparisons)
    const char* bad = power > 1.0 && power < 2.0 ? nullptr : "the variance power must lie strictly between 1 and 2";
    return {TWEEDIE_NC, power, bad, tweedie_const, tweedie_disp, tweedie_check, tweedie_start_mean, tweedie_loglik, tweedie_ll_fix};
}

// the dense row pass: count_pass with the Tweedie row at `power` (w is the weight per row, loglik the sum of q)
static DispDenseRows tweedie_rows(double power) {
    return [power](const auto&... a) { return count_pass(tweedie_row_model(power), a...); };
}

}  // namespace dlsa

extern "C" {

size_t dlsa_tweedie_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    return dlsa::disp_workspace_bytes(dlsa::TWEEDIE_NC, max_rows, p, intercept, row_step);
}

int dlsa_tweedie_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, double power,
                          double dispersion, int64_t n, int p, int intercept, double* H, int64_t ldh, double* g, double* loglik,
                          double* w_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    return dlsa::disp_pass_entry("tweedie_pass", dlsa::tweedie_family(power), dlsa::tweedie_rows(power), X, ldx, y, offset, beta,
                                 dispersion, n, p, intercept, H, ldh, g, loglik, w_out, stats_out, ws, ws_bytes, stream);
}

int dlsa_tweedie_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double power,
                         double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                         int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host,
                         double* deviance_host, void* ws, size_t ws_bytes, void* stream) {
    return dlsa::disp_fit_entry("tweedie_fit", dlsa::tweedie_family(power), dlsa::tweedie_rows(power), X, ldx, y, offset,
                                part_first_host, part_rows_host, row_step, K, p, intercept, dispersion_fixed, tol, max_iter, coef,
                                Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, dispersion_host, pearson_host,
                                deviance_host, ws, ws_bytes, stream);
}

}  // extern "C"
