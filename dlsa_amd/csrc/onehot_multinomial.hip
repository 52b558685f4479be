// Structured multinomial logistic (softmax) map step for one-hot designs: the pass and fit of multinomial.hip on the RAW
// representation of a design [intercept | standardised numerics | one-hot factor levels] (num [n, q] fp64, codes [n, f] int32)
// under a dlsa_onehot_plan -- the dense n x p matrix is never built.  Results equal the dense multinomial entries (intercept = 0) on
// the matrix dlsa_design_f64 would build (to rounding); an intercept is the plan's constant column, one column of every class block.
//
// Layout: as multinomial.hip with pe = the plan's p: y holds the class codes 0 .. C - 1 as doubles, class 0 is the reference,
// J = C - 1, theta is class-major (theta[j p + c], c in the plan's column order), g has J p entries, H is (J p) x (J p) with both
// triangles, P is class-major [J][ldprob].
//
// Launches per evaluation at a fixed theta:
//   1 oh_mn_row_kernel<J>   one thread per row on the skeleton of oh_row_kernel (onehot_pass.h), a second kernel beside it because
//                           a row has J linear predictors, J residuals and no single weight: J gathers eta_j = d . beta_{j,D} +
//                           sum_t beta_j[col(t, code_t)] from the coefficients in LDS (J p doubles), the softmax of the row
//                           (mn_softmax_row, shared with the dense pass), J residuals 1[y = j] - p_j; per-workgroup partials of g
//                           (dense part in J x OH_MAXD registers, level part J f LDS adds per row into the thread's copy of a
//                           J p-cell histogram; wave turn-taking: a fixed order of the adds, bit-reproducible) and of loglik; P
//                           (when wanted);
//   1 logit_finish_launch   the fixed-order column sums of the partials over all J p columns at once (logit.hip, shared): g is
//                           contiguous because the intercept is a plan column;
//   per pair j <= k         mn_weight (w = p_j (delta_jk - p_k) into ONE reused n-vector) and onehot_gram_impl(plan, num, codes, w)
//                           straight into H at row j p, column k p with the pitch of H: a table accumulation in ordered floating
//                           point (the weights of an off-diagonal block are negative), no border pass;
//   1 mn_mirror             the blocks (j, k), j < k, copied to (k, j).
// Traffic per row: 8q + 4f + 8 (y) + 8J (P written) bytes for the pass, 8q + 4f + 8 per Gram and 16 or 24 per weight kernel.
// The once-per-partition check, the weight / mirror / start kernels and the fit driver are multinomial.hip's
// (multinomial_internal.h); the row checks of num / codes and the plan's constant column are onehot_poisson.hip's.
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include "multinomial_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

// copies of the J p-cell residual histogram: oh_logit_rep's rule on J p cells (J p <= 2048: at least one copy fits 32 KiB)
static int oh_mn_rep(int jp) { return oh_logit_rep(jp); }

// One thread per row; every thread runs the same number of rounds (the ordered mode has barriers inside): rows past n are clamped
// and masked.  LDS: theta (J p), nrep histogram copies of J p cells, the level-column table, the block reduction's 16 doubles.
template <int J>
__global__ __launch_bounds__(OH_THREADS) void oh_mn_row_kernel(OhDesc ds, const int32_t* __restrict__ level_col,
                                                               const double* __restrict__ num, int64_t ldn,
                                                               const int32_t* __restrict__ codes, int64_t ldc,
                                                               const double* __restrict__ y, const double* __restrict__ theta,
                                                               int64_t n, double* __restrict__ prob, int64_t ldprob,
                                                               double* __restrict__ gpart, double* __restrict__ llpart, int nrep) {
    extern __shared__ double sm[];
    const int p = ds.p, jp = J * p;
    double* sbeta = sm;                           // J p, class-major
    double* sg = sm + jp;                         // nrep x J p (histograms of the J residuals; lanes spread over the copies)
    int* scol = reinterpret_cast<int*>(sm + (1 + nrep) * jp);       // nlev_total
    double* red = reinterpret_cast<double*>(scol + ((ds.nlev_total + 1) & ~1));
    for (int c = threadIdx.x; c < jp; c += blockDim.x) sbeta[c] = theta[c];
    for (int c = threadIdx.x; c < nrep * jp; c += blockDim.x) sg[c] = 0.0;
    double* sg_mine = sg + (threadIdx.x % nrep) * jp;
    for (int c = threadIdx.x; c < ds.nlev_total; c += blockDim.x) scol[c] = level_col[c];
    __syncthreads();
    double gd[J][OH_MAXD];
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int a = 0; a < OH_MAXD; ++a) gd[j][a] = 0.0;
    }
    double ll = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounds = (n - (int64_t)blockIdx.x * blockDim.x + stride - 1) / stride;
    const int mywave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + rd * stride;
        const bool valid = i0 < n;
        const int64_t i = valid ? i0 : n - 1;
        double d[OH_MAXD];
        oh_dense_row(ds, num, ldn, i, d);
        double eta[J];
#pragma unroll
        for (int j = 0; j < J; ++j) eta[j] = 0.0;
#pragma unroll
        for (int a = 0; a < OH_MAXD; ++a) {
            if (a < ds.D) {
                const int c = ds.dense_col[a];
#pragma unroll
                for (int j = 0; j < J; ++j) eta[j] = fma(d[a], sbeta[j * p + c], eta[j]);
            }
        }
        int cols[OH_MAXF];
#pragma unroll
        for (int t = 0; t < OH_MAXF; ++t) {
            cols[t] = -1;
            if (t < ds.f) {
                const int code = codes[i * ldc + t];
                const int nl = ds.lvl_off[t + 1] - ds.lvl_off[t];
                if (code >= 0 && code < nl) cols[t] = scol[ds.lvl_off[t] + code];      // an unknown / baseline level contributes nothing
                if (cols[t] >= 0) {
#pragma unroll
                    for (int j = 0; j < J; ++j) eta[j] += sbeta[j * p + cols[t]];
                }
            }
        }
        const double yv = y[i];
        double pr[J], r[J];
        const double term = mn_softmax_row<J>(eta, yv, pr);
        if (valid) ll += term;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            r[j] = valid ? (yv == (double)(j + 1) ? 1.0 : 0.0) - pr[j] : 0.0;
            if (prob && valid) prob[j * ldprob + i] = pr[j];
#pragma unroll
            for (int a = 0; a < OH_MAXD; ++a) gd[j][a] = fma(r[j], d[a], gd[j][a]);
        }
        if (ds.ordered) {                           // one wave at a time, in wave order: a fixed order of the LDS adds
            for (int turn = 0; turn < nwaves; ++turn) {
                if (turn == mywave && valid) {
#pragma unroll
                    for (int t = 0; t < OH_MAXF; ++t) {
                        if (t < ds.f && cols[t] >= 0) {
#pragma unroll
                            for (int j = 0; j < J; ++j) unsafeAtomicAdd(&sg_mine[j * p + cols[t]], r[j]);
                        }
                    }
                }
                __syncthreads();
            }
        } else if (valid) {
#pragma unroll
            for (int t = 0; t < OH_MAXF; ++t) {
                if (t < ds.f && cols[t] >= 0) {
#pragma unroll
                    for (int j = 0; j < J; ++j) unsafeAtomicAdd(&sg_mine[j * p + cols[t]], r[j]);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int a = 0; a < OH_MAXD; ++a) {
            const double sgd = oh_block_sum(gd[j][a], red);
            if (threadIdx.x == 0 && a < ds.D) sg[j * p + ds.dense_col[a]] += sgd;
        }
    }
    const double sll = oh_block_sum(ll, red);
    __syncthreads();
    double* gp = gpart + (int64_t)blockIdx.x * jp;
    for (int c = threadIdx.x; c < jp; c += blockDim.x) {
        double t = sg[c];
        for (int rp = 1; rp < nrep; ++rp) t += sg[rp * jp + c];      // fixed order
        gp[c] = t;
    }
    if (threadIdx.x == 0) llpart[blockIdx.x] = sll;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct OhMnLayout {
    size_t off_oh, oh_bytes, off_w, off_prob, off_y, off_cpart, off_cst, off_state, total;
    int64_t ldprob;
};

// the pass's partials: [nb][J p] and [nb], J times what onehot_workspace_bytes_impl reserves for a logit pass
static size_t oh_mn_pass_bytes(int p, int J, int64_t n) {
    const int nb = oh_logit_blocks(n);
    return align_up((size_t)nb * J * p * sizeof(double), 256) + align_up((size_t)nb * sizeof(double), 256) + 256;
}

// off_oh: the arena of the structured passes (the row pass's partials, then each Gram's: the larger of the two); w: the weights of
// the block in hand; prob: the J class rows; row_step > 1: room for the gathered responses of a strided partition; then the
// Newton state on J p coefficients
static OhMnLayout oh_mn_layout(const dlsa_onehot_plan* pl, int64_t max_rows, int J, int64_t row_step) {
    OhMnLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    const int p = onehot_plan_p(pl);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.ldprob = mn_ldprob(n);
    l.oh_bytes = align_up(std::max(onehot_workspace_bytes_impl(pl, n), oh_mn_pass_bytes(p, J, n)), 256);
    l.off_oh = take(l.oh_bytes);
    l.off_w = take(8 * (size_t)n);
    l.off_prob = take(8 * (size_t)J * l.ldprob);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_cpart = take(8 * (size_t)MN_NQ * MN_CHECK_BLOCKS);
    l.off_cst = take(8 * 16);
    l.off_state = take(newton_state_bytes(J * p));
    l.total = o;
    return l;
}

template <int J>
static void oh_mn_launch(const OhDesc& ds, const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                         const double* y, const double* theta, int64_t n, double* prob, int64_t ldprob, double* gpart, double* llpart,
                         int nb, int nrep, size_t shm, hipStream_t s) {
    hipLaunchKernelGGL(oh_mn_row_kernel<J>, dim3(nb), dim3(OH_THREADS), shm, s, ds, (const int32_t*)pl->d_level_col, num, ldn, codes, ldc,
                       y, theta, n, prob, ldprob, gpart, llpart, nrep);
}

// One partition at a fixed theta.  H (nullable; (J p) x (J p), pitch ldh) needs prob (J class rows of pitch ldprob >= n) and w (n);
// g, loglik (the sum of log p_y), prob nullable otherwise.  ws_oh: the structured passes' arena (256-aligned, oh_mn_layout's oh_bytes).
static int oh_mn_pass_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y,
                           const double* theta, int classes, int64_t n, double* H, int64_t ldh, double* g, double* loglik, double* prob,
                           int64_t ldprob, double* w, void* ws_oh, size_t ws_oh_bytes, hipStream_t s) {
    const int J = classes - 1;
    OhDesc ds = pl->desc;
    { const char* e = kernel_knob("DLSA_OH_ORDERED"); ds.ordered = e ? (atoi(e) != 0) : 1; }      // wave turn-taking unless 0
    ds.overflow = nullptr;
    const int p = ds.p, jp = J * p;
    const int nb = oh_logit_blocks(n);
    Arena ar(ws_oh, ws_oh_bytes);
    double* gpart = (double*)ar.take((size_t)nb * jp * sizeof(double));
    double* llpart = (double*)ar.take((size_t)nb * sizeof(double));
    if (!gpart || !llpart) {
        set_error("onehot multinomial pass: the pass arena of %zu bytes is too small", ws_oh_bytes);
        return DLSA_ERR_WORKSPACE;
    }
    const int nrep = oh_mn_rep(jp);
    const size_t shm = (size_t)((1 + nrep) * jp + 16) * sizeof(double) + (size_t)((ds.nlev_total + 1) & ~1) * sizeof(int);
    switch (J) {
        case 1: oh_mn_launch<1>(ds, pl, num, ldn, codes, ldc, y, theta, n, prob, ldprob, gpart, llpart, nb, nrep, shm, s); break;
        case 2: oh_mn_launch<2>(ds, pl, num, ldn, codes, ldc, y, theta, n, prob, ldprob, gpart, llpart, nb, nrep, shm, s); break;
        case 3: oh_mn_launch<3>(ds, pl, num, ldn, codes, ldc, y, theta, n, prob, ldprob, gpart, llpart, nb, nrep, shm, s); break;
        case 4: oh_mn_launch<4>(ds, pl, num, ldn, codes, ldc, y, theta, n, prob, ldprob, gpart, llpart, nb, nrep, shm, s); break;
        case 5: oh_mn_launch<5>(ds, pl, num, ldn, codes, ldc, y, theta, n, prob, ldprob, gpart, llpart, nb, nrep, shm, s); break;
        case 6: oh_mn_launch<6>(ds, pl, num, ldn, codes, ldc, y, theta, n, prob, ldprob, gpart, llpart, nb, nrep, shm, s); break;
        case 7: oh_mn_launch<7>(ds, pl, num, ldn, codes, ldc, y, theta, n, prob, ldprob, gpart, llpart, nb, nrep, shm, s); break;
        default:
            set_error("onehot multinomial pass: no row kernel for %d classes", classes);
            return DLSA_ERR_INVALID;
    }
    DLSA_HIP_CHECK(hipGetLastError());
    if (g || loglik) {
        logit_finish_launch((const double*)gpart, (const double*)llpart, nb, jp, jp, g, loglik, s, nullptr, nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    if (!H) return DLSA_OK;
    // (a Gram's partials overwrite the pass's in the same arena: the finish launch above has consumed them, in stream order)
    for (int j = 0; j < J; ++j) {
        for (int k = j; k < J; ++k) {
            int rc = mn_weight(prob + j * ldprob, prob + k * ldprob, j == k ? 1 : 0, n, w, s);
            if (rc) return rc;
            rc = onehot_gram_impl(pl, num, ldn, codes, ldc, w, n, H + (size_t)j * p * ldh + (size_t)k * p, ldh, ws_oh, ws_oh_bytes, s, false);
            if (rc) return rc;
        }
    }
    return mn_mirror(H, ldh, J, p, s);
}

}  // namespace dlsa

extern "C" {

size_t dlsa_onehot_multinomial_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int classes, int64_t row_step) {
    if (!plan || classes < 2 || classes > dlsa::MN_MAX_CLASSES || max_rows < 0 || row_step < 1) return 0;
    if ((int64_t)(classes - 1) * dlsa::onehot_plan_p(plan) > 2048) return 0;
    return dlsa::oh_mn_layout(plan, max_rows, classes - 1, row_step).total;
}

int dlsa_onehot_multinomial_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                     const double* y, const double* theta, int classes, int64_t n, double* H, int64_t ldh, double* g,
                                     double* loglik, double* prob_out, int64_t ldprob, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && theta, "onehot_multinomial_pass: null plan, y or theta");
    int rc = oh_pois_check_rows("onehot_multinomial_pass", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    const int p = onehot_plan_p(plan);
    rc = mn_coef_ok("onehot_multinomial_pass", p, classes);
    if (rc) return rc;
    const int J = classes - 1, d = J * p;
    DLSA_REQUIRE(n >= 1 && (!H || ldh >= d), "onehot_multinomial_pass: bad shape n=%lld p=%d ldh=%lld", (long long)n, p, (long long)ldh);
    DLSA_REQUIRE(!prob_out || (ldprob >= n && ldprob % 32 == 0 && ((uintptr_t)prob_out & 255) == 0),
                 "onehot_multinomial_pass: prob_out needs 256-byte aligned class rows (ldprob >= n, a multiple of 32), got ldprob=%lld",
                 (long long)ldprob);
    const OhMnLayout l = oh_mn_layout(plan, n, J, 1);
    rc = newton_check_ws("onehot_multinomial_pass", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* prob = prob_out ? prob_out : (H ? (double*)(wsc + l.off_prob) : nullptr);
    rc = oh_mn_pass_impl(plan, num, ldn, codes, ldc, y, theta, classes, n, H, ldh, g, loglik, prob, prob_out ? ldprob : l.ldprob,
                         (double*)(wsc + l.off_w), wsc + l.off_oh, l.oh_bytes, s);
    if (rc || !loglik) return rc;
    rc = mn_check(y, n, classes, (double*)(wsc + l.off_cpart), (double*)(wsc + l.off_cst), s);
    if (rc) return rc;
    return mn_ll_fix(loglik, (const double*)(wsc + l.off_cst), s);
}

int dlsa_onehot_multinomial_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                    const double* y, const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step,
                                    int K, int classes, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                                    int* n_iter_host, int* status_host, double* loglik_host, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "onehot_multinomial_fit: null argument");
    int rc = oh_pois_check_rows("onehot_multinomial_fit", plan, num, ldn, codes, ldc);
    if (rc) return rc;
    const int p = onehot_plan_p(plan);
    rc = mn_coef_ok("onehot_multinomial_fit", p, classes);
    if (rc) return rc;
    const int J = classes - 1, d = J * p;
    DLSA_REQUIRE(K > 0 && row_step >= 1, "onehot_multinomial_fit: bad shape K=%d step=%lld", K, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "onehot_multinomial_fit: bad tol/max_iter");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "onehot_multinomial_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const OhMnLayout l = oh_mn_layout(plan, max_rows, J, row_step);
    rc = newton_check_ws("onehot_multinomial_fit", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    MnFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.ybuf = (double*)(wsc + l.off_y);
    b.st = newton_state_at(wsc + l.off_state, d);
    double* wv = (double*)(wsc + l.off_w);
    double* prob = (double*)(wsc + l.off_prob);
    void* ws_oh = wsc + l.off_oh;
    const size_t oh_bytes = l.oh_bytes;
    const int64_t ldprob = l.ldprob;
    const int64_t pn = ldn * row_step, pc = ldc * row_step;   // rows first, first + step, ...: strided views, num / codes read in place
    auto eval = [=](int k, const double* yk, int64_t nk, const double* theta, double* Hk, double* g, double* ll) {
        const double* numk = num ? num + part_first_host[k] * ldn : nullptr;
        const int32_t* codesk = codes ? codes + part_first_host[k] * ldc : nullptr;
        return oh_mn_pass_impl(plan, numk, pn, codesk, pc, yk, theta, classes, nk, Hk, d, g, ll, prob, ldprob, wv, ws_oh, oh_bytes, s);
    };
    return mn_fit_core("onehot_multinomial_fit", MN_NO_CLASS, y, part_first_host, part_rows_host, row_step, K, d, classes, tol, max_iter, coef,
                       Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, b, mn_null_start(J, p, oh_pois_icpt_col(plan)), eval, s);
}

}  // extern "C"
