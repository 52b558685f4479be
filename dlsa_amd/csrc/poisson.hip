// Poisson regression map step (log link, optional offsets / exposure): one partition's log-likelihood, score and Fisher
// information at a fixed beta, and the per-partition Newton fit on top of it.  The block a partition returns (coef,
// Sig_inv = the information at coef, Sig_inv coef) feeds the unchanged one-round combine.
//
// Algebra (one partition; the design is [1 | X] with the implicit intercept, X otherwise; o = offset, 0 when absent):
//   eta = [1 | x]' beta + o,  mu = exp(eta),
//   loglik = sum y eta - mu - lgamma(y + 1),  g = X'(y - mu),  H = X' diag(mu) X.
//
// Launches per evaluation (every partial combines in a fixed order: no float atomics, no waits between workgroups):
//   1 count_pass_kernel     (count_pass.h, shared with negbin.hip, here with the terms of PoisRow) one read of the rows in the
//                           logit pass's layout (rowdot.h: RB rows per wave, one merged butterfly for their dot products,
//                           non-temporal 16-byte loads): mu (-> w), per-block partials of g, sum (y - mu), sum (y eta - mu)
//                           and, with the intercept and H wanted, of X'mu and sum mu (the Hessian's border, so no extra pass);
//   2 logit_finish_launch   the fixed-order column sums of those partials (the finish step of logit.hip, shared);
//   3 the Gram              dlsa_gram_f64's dispatch on (X, mu) into the p x p block (gram_icpt_impl with the border).
// The constant sum lgamma(y + 1) is a small reduction of its own, once per partition (poisson_const_kernel), which also
// counts the rows with a negative or non-finite count or offset and sums y and e^o for the intercept's start value.
// The fit driver (pois_fit_core) takes the evaluation at beta as a callable and is shared with the structured one-hot fit
// (onehot_poisson.hip) through poisson_internal.h, as are the constant-term, log-likelihood-fix and gather launchers; the Newton
// iteration itself is newton_fit.h's, shared with negbin.hip and cox.hip.
#include "common.h"
#include "block_sums.h"
#include "poisson_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"       // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "poisson_exp.h"  // exp_full
#include "count_pass.h"   // count_pass_kernel, count_pass, CountScratch

// the Poisson row: weight mu, residual y - mu, term y eta - mu
struct PoisRow {
    static constexpr bool STORES_MU = false;
    __device__ __forceinline__ void terms(double yv, double eta, double mu, double& wgt, double& rs, double& llt) const {
        wgt = mu;
        rs = yv - mu;
        llt = yv * eta - mu;
    }
};

// ---- once per partition: [sum lgamma(y + 1), sum y, sum e^o, rows with y < 0 or a non-finite y / o] --------------------
__global__ __launch_bounds__(256) void poisson_const_kernel(const double* __restrict__ y, const double* __restrict__ off,
                                                            int64_t n, double* __restrict__ part) {
    double lg = 0.0, sy = 0.0, se = 0.0, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yv = y[i], ov = off ? off[i] : 0.0;
        if (yv >= 0.0 && isfinite(yv) && isfinite(ov)) {      // (NaN fails yv >= 0)
            lg += lgamma(yv + 1.0);
            sy += yv;
            se += exp_full(ov);
        } else {
            bad += 1.0;
        }
    }
    const double acc[4] = {lg, sy, se, bad};
    block_partials_store(acc, part);
}

// one wave per quantity (nq <= 4 of them), the block partials in a fixed order
__global__ __launch_bounds__(256) void block_sum_finish_kernel(const double* __restrict__ part, int nblocks, int nq,
                                                              double* __restrict__ out) {
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (j >= nq) return;
    double s = 0.0;
    for (int b = lane; b < nblocks; b += 64) s += part[(int64_t)b * nq + j];
    s = wave_allreduce_sum(s);
    if (lane == 0) out[j] = s;
}

// the pass entry's full log-likelihood: the kernel's sum of y eta - mu minus the constant (NaN when a row is not a valid count)
__global__ void poisson_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ cst) {
    if (threadIdx.x == 0) ll[0] = cst[3] > 0.0 ? NAN : ll[0] - cst[0];
}

// out[j] = v[first + j * step]
__global__ void poisson_gather_kernel(const double* __restrict__ v, int64_t first, int64_t step, int64_t n, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = v[first + j * step];
}

// Newton start: beta = 0, the intercept (entry icpt_col; -1: none) at b0
__global__ void poisson_start_kernel(double* __restrict__ beta, int pe, int icpt_col, double b0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < pe) beta[i] = i == icpt_col ? b0 : 0.0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct PoisLayout {
    CountScratchOff sc;
    size_t off_cpart, off_cst, off_w, off_y, off_o, off_gram, total;
};

// pass scratch; row_step > 1: room for the gathered counts and offsets of a strided partition
static PoisLayout pois_layout(int64_t max_rows, int p, int64_t row_step) {
    PoisLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.sc = count_scratch_take(take, p);
    l.off_cpart = take(8 * 4 * (size_t)POIS_CONST_BLOCKS);
    l.off_cst = take(8 * 4);
    l.off_w = take(8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_gram = take(gram_workspace_bytes_impl(n, p, 8));
    l.total = o;
    return l;
}

int block_sum_finish(const double* part, int nblocks, int nq, double* out, hipStream_t s) {
    hipLaunchKernelGGL(block_sum_finish_kernel, dim3(1), dim3(256), 0, s, part, nblocks, nq, out);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int pois_const(const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s) {
    const int blocks = (int)std::min<int64_t>(POIS_CONST_BLOCKS, std::max<int64_t>(1, (n + 255) / 256));
    hipLaunchKernelGGL(poisson_const_kernel, dim3(blocks), dim3(256), 0, s, y, off, n, cpart);
    return block_sum_finish(cpart, blocks, 4, cst, s);
}

int pois_ll_fix(double* ll, const double* cst, hipStream_t s) {
    hipLaunchKernelGGL(poisson_ll_fix_kernel, dim3(1), dim3(64), 0, s, ll, cst);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int pois_start(double* beta, int pe, int icpt_col, double b0, hipStream_t s) {
    hipLaunchKernelGGL(poisson_start_kernel, dim3((pe + 255) / 256), dim3(256), 0, s, beta, pe, icpt_col, b0);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int pois_gather(const double* v, int64_t first, int64_t step, int64_t n, double* out, hipStream_t s) {
    hipLaunchKernelGGL(poisson_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, first, step, n, out);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

// One partition at a fixed beta (count_pass with the Poisson row): w is mu per row, loglik the sum of y eta - mu, without the
// constant.
static int pois_pass_impl(const double* X, int64_t ldx, const double* y, const double* off, const double* beta, int64_t n, int p,
                          int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w, char* ws, const PoisLayout& l,
                          hipStream_t s) {
    return count_pass(PoisRow{}, X, ldx, y, off, beta, n, p, intercept, H, ldh, g, loglik, w, nullptr, count_scratch_at(ws, l.sc),
                      ws + l.off_gram, l.total - l.off_gram, s);
}

// The driver of the Poisson fits (dense rows here, raw one-hot rows in onehot_poisson.hip): `eval` is the only part that knows
// the representation of the design; the iteration is newton_fit_loop (newton_fit.h).
int pois_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host,
                  const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double tol, int max_iter,
                  double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                  const PoisFitBufs& b, const PoisEval& eval, hipStream_t s) {
    int overall = DLSA_OK;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_rows_host[k];
        const double* yk = y + part_first_host[k];
        const double* ok = offset ? offset + part_first_host[k] : nullptr;
        double* Hk = Sig_inv + (size_t)k * pe * pe;
        double* ck = coef + (size_t)k * pe;
        double* sk = Sig_invMcoef + (size_t)k * pe;
        int st_k = DLSA_PART_EMPTY, iters = 0;
        double ll = 0.0, cst[4] = {0.0, 0.0, 0.0, 0.0};
        if (nk > 0) {
            // a strided partition's counts and offsets are gathered once (8 bytes per row each)
            int rc = pois_gather_rows(y, offset, part_first_host[k], row_step, nk, b.ybuf, b.obuf, yk, ok, s);
            if (rc) return rc;
            rc = pois_const(yk, ok, nk, b.cpart, b.cst, s);
            if (rc) return rc;
            DLSA_HIP_CHECK(hipMemcpyAsync(cst, b.cst, sizeof(cst), hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            if (cst[3] > 0.0) {
                set_error("%s: partition %d has %.0f rows with a negative or non-finite count or offset", who, k, cst[3]);
                return DLSA_ERR_INVALID;
            }
        }
        // sum y = 0: the MLE lies at eta -> -inf, where H -> 0 and H theta -> 0: the zero block is the block's limit
        if (nk > 0 && cst[1] > 0.0) {
            // the intercept starts at log(sum y / sum e^o), the exact MLE of the intercept-only model
            const double b0 = (icpt_col >= 0 && cst[2] > 0.0 && isfinite(cst[2])) ? log(cst[1] / cst[2]) : 0.0;
            const int rcs = pois_start(b.st.beta, pe, icpt_col, b0, s);
            if (rcs) return rcs;
            const NewtonDevice dev{b.st, Hk, pe, s};
            NewtonOutcome o;
            const int rcl = newton_fit_loop(NEWTON_POISSON, tol, max_iter + 1,
                                            [&](bool&) { return eval(k, yk, ok, nk, b.st.beta, Hk, b.st.g, b.st.stats + 3); }, dev, newton_no_hook, o);
            if (rcl) return rcl;
            st_k = o.status; iters = o.n_iter; ll = o.ll;
        }
        const int rcf = newton_fit_finish(st_k, iters, ll - cst[0], b.st.beta, pe, Hk, ck, sk, k, n_iter_host, status_host, loglik_host, overall, s);
        if (rcf) return rcf;
    }
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    return overall;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_poisson_workspace_bytes(int64_t max_rows, int p, int intercept, int64_t row_step) {
    if (p <= 0 || p + (intercept ? 1 : 0) > 2048 || max_rows < 0 || row_step < 1) return 0;
    return dlsa::align_up(dlsa::pois_layout(max_rows, p, row_step).total, 256) + dlsa::newton_state_bytes(p + (intercept ? 1 : 0));
}

int dlsa_poisson_pass_f64(const double* X, int64_t ldx, const double* y, const double* offset, const double* beta, int64_t n, int p,
                          int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes,
                          void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && beta, "poisson_pass: null X, y or beta");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(n >= 1 && p > 0 && pe <= 2048 && ldx >= p && (!H || ldh >= pe), "poisson_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld",
                 (long long)n, p, (long long)ldx, (long long)ldh);
    const PoisLayout l = pois_layout(n, p, 1);
    // (the pass carves l.total of it; the contract is the query, which also holds a fit's Newton state)
    int rc = newton_check_ws("poisson_pass", ws, ws_bytes, dlsa_poisson_workspace_bytes(n, p, intercept, 1));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* w = w_out ? w_out : (H ? (double*)(wsc + l.off_w) : nullptr);
    rc = pois_pass_impl(X, ldx, y, offset, beta, n, p, intercept, H, ldh, g, loglik, w, wsc, l, s);
    if (rc || !loglik) return rc;
    rc = pois_const(y, offset, n, (double*)(wsc + l.off_cpart), (double*)(wsc + l.off_cst), s);
    if (rc) return rc;
    return pois_ll_fix(loglik, (const double*)(wsc + l.off_cst), s);
}

int dlsa_poisson_fit_f64(const double* X, int64_t ldx, const double* y, const double* offset, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, double tol, int max_iter,
                         double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                         void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "poisson_fit: null argument");
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(K > 0 && p > 0 && pe <= 2048 && ldx >= p && row_step >= 1, "poisson_fit: bad shape K=%d p=%d ldx=%lld step=%lld", K, p,
                 (long long)ldx, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "poisson_fit: bad tol/max_iter");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "poisson_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const PoisLayout l = pois_layout(max_rows, p, row_step);
    const size_t need = dlsa_poisson_workspace_bytes(max_rows, p, intercept, row_step);
    const int rcw = newton_check_ws("poisson_fit", ws, ws_bytes, need);
    if (rcw) return rcw;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    PoisFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.st = newton_state_at(wsc + align_up(l.total, 256), pe);
    double* wv = (double*)(wsc + l.off_w);
    const int64_t pitch = ldx * row_step;                     // rows first, first + step, ...: a strided view, no copy of X
    const PoisEval eval = [=](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* Hk, double* g,
                              double* ll) {
        return pois_pass_impl(X + part_first_host[k] * ldx, pitch, yk, ok, beta, nk, p, intercept, Hk, pe, g, ll, wv, wsc, l, s);
    };
    return pois_fit_core("poisson_fit", y, offset, part_first_host, part_rows_host, row_step, K, pe, intercept ? 0 : -1, tol, max_iter,
                         coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, b, eval, s);
}

}  // extern "C"
