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
// Once per partition: gamma_const_kernel + block_sum_finish_kernel (sum log y, sum y e^-o for the intercept's start, the data
// check).  Once per fit (and per pass that asks): gamma_disp_kernel + the same finish over (y, mu), 16 bytes per row, and
// disp_scale_kernel on the pe x pe block.
// This file holds what is the Gamma family's: the row model, the two sum kernels, the log-likelihood and the record that hands
// them to the driver of the dispersion families (dispersion.hip, dispersion_internal.h), which owns the entries' bodies, the
// workspace and the fit; onehot_gamma.hip brings the same record with its own row pass.
#include "common.h"
#include "poisson_internal.h"
#include "dispersion_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"       // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "poisson_exp.h"  // exp_full
#include "count_pass.h"   // count_pass_kernel, count_pass, CountScratch

// once per partition, GAMMA_NC sums: [sum log y, sum y e^-o, rows with y <= 0 or a non-finite y / o]
enum { GAMMA_LOGY = 0, GAMMA_YEO = 1, GAMMA_BAD = 2 };

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

// ---- once per partition: the GAMMA_NC sums ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gamma_const_kernel(const double* __restrict__ y, const double* __restrict__ off, int64_t n,
                                                          double* __restrict__ part) {
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
    block_partials_store(acc, part);
}

// ---- the dispersion sums over (y, mu): [sum (r - 1)^2, 2 sum (r - 1 - log r)] ---------------------------------------------
__global__ __launch_bounds__(256) void gamma_disp_kernel(const double* __restrict__ y, const double* __restrict__ mu, int64_t n,
                                                         double* __restrict__ part) {
    double ps = 0.0, dv = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double r = y[i] / mu[i], d = r - 1.0;
        ps = fma(d, d, ps);
        dv += d - log(r);
    }
    const double acc[DISP_ND] = {ps, 2.0 * dv};               // (the doubling is exact, so it commutes with the sums)
    block_partials_store(acc, part);
}

// the pass entry's full log-likelihood from the row sum of -(r + eta): nu ll + c + (nu - 1) sum log y (NaN when a row is not a
// valid response)
__global__ void gamma_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ cst, double nu, double c) {
    if (threadIdx.x == 0) ll[0] = cst[GAMMA_BAD] > 0.0 ? NAN : fma(nu, ll[0], c) + (nu - 1.0) * cst[GAMMA_LOGY];
}

// ---- host side: the family record ------------------------------------------------------------------------------------------
static int gamma_const(const DispFamily&, const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s) {
    const int blocks = disp_sum_blocks(n);
    hipLaunchKernelGGL(gamma_const_kernel, dim3(blocks), dim3(256), 0, s, y, off, n, cpart);
    return block_sum_finish(cpart, blocks, GAMMA_NC, cst, s);
}

static int gamma_disp(const DispFamily&, const double* y, const double* mu, int64_t n, double* dpart, double* dst, hipStream_t s) {
    const int blocks = disp_sum_blocks(n);
    hipLaunchKernelGGL(gamma_disp_kernel, dim3(blocks), dim3(256), 0, s, y, mu, n, dpart);
    return block_sum_finish(dpart, blocks, DISP_ND, dst, s);
}

static int gamma_check(const char* who, int k, const double* cst) {
    if (cst[GAMMA_BAD] > 0.0) {
        set_error("%s: partition %d has %.0f rows with a non-positive or non-finite response or a non-finite offset", who, k,
                  cst[GAMMA_BAD]);
        return DLSA_ERR_INVALID;
    }
    return DLSA_OK;
}

// sum y e^-o / n
static double gamma_start_mean(const double* cst, int64_t n) { return cst[GAMMA_YEO] / (double)n; }

// n (nu log nu - lgamma nu): the beta-free part of the log-likelihood that does not depend on y
static double gamma_ll_const(double nu, int64_t n) { return (double)n * (nu * log(nu) - lgamma(nu)); }

static double gamma_loglik(double nu, double ll, const double* cst, int64_t n) {
    return nu * ll + gamma_ll_const(nu, n) + (nu - 1.0) * cst[GAMMA_LOGY];
}

static int gamma_ll_fix(double* ll, const double* cst, double nu, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(gamma_ll_fix_kernel, dim3(1), dim3(64), 0, s, ll, cst, nu, gamma_ll_const(nu, n));
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

DispFamily gamma_family() {
    return {GAMMA_NC, 0.0, nullptr, gamma_const, gamma_disp, gamma_check, gamma_start_mean, gamma_loglik, gamma_ll_fix};
}

// the dense row pass: count_pass with the Gamma row (w is r per row, loglik the sum of -(r + eta))
static DispDenseRows gamma_rows() {
    return [](const auto&... a) { return count_pass(GammaRow{}, a...); };
}

}  // namespace dlsa

extern "C" {

size_t dlsa_gamma_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    return dlsa::disp_workspace_bytes(dlsa::GAMMA_NC, max_rows, p, intercept, row_step);
}

int dlsa_gamma_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, double dispersion,
                        int64_t n, int p, int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out,
                        double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    return dlsa::disp_pass_entry("gamma_pass", dlsa::gamma_family(), dlsa::gamma_rows(), X, ldx, y, offset, beta, dispersion, n, p,
                                 intercept, H, ldh, g, loglik, w_out, stats_out, ws, ws_bytes, stream);
}

int dlsa_gamma_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                       const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double dispersion_fixed,
                       double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host,
                       int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host, double* deviance_host,
                       void* ws, size_t ws_bytes, void* stream) {
    return dlsa::disp_fit_entry("gamma_fit", dlsa::gamma_family(), dlsa::gamma_rows(), X, ldx, y, offset, part_first_host, part_rows_host,
                                row_step, K, p, intercept, dispersion_fixed, tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host,
                                status_host, loglik_host, dispersion_host, pearson_host, deviance_host, ws, ws_bytes, stream);
}

}  // extern "C"
