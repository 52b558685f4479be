// Structured Poisson map step for one-hot designs: the Poisson pass and fit of poisson.hip on the RAW representation of a
// design [intercept | standardised numerics | one-hot factor levels] (num [n, q] fp64, codes [n, f] int32) under a
// dlsa_onehot_plan -- the dense n x p matrix is never built.  Results equal the dense Poisson entries on the matrix
// dlsa_design_f64 would build (to rounding).
//
// Launches per evaluation at a fixed beta:
//   1 oh_poisson_kernel     one thread per row as oh_logit_kernel (onehot.hip): eta = d . beta_D + sum_t beta[col(t, code_t)] + o
//                           (a gather), mu = exp_full(eta) (-> w), r = y - mu, per-workgroup partials of g (dense part in
//                           registers, level part an LDS histogram with replicated copies and wave turn-taking: a fixed
//                           order of the adds, bit-reproducible) and of sum y eta - mu;
//   2 logit_finish_launch   the fixed-order column sums of those partials (logit.hip, shared);
//   3 the Gram              onehot_gram_impl(plan, num, codes, mu) with irls_weights = false: mu is unbounded, so the ordered
//                           floating-point mode (full relative accuracy at any scale, bit-reproducible), never the fixed-point one.
// Traffic per row: 8q + 4f + 8 (y) + 8 (o) + 8 (mu written) bytes for the pass, 8q + 4f + 8 for the Gram.
// The constant sum lgamma(y + 1), the data check, the gather of a strided partition's counts / offsets and the Newton loop
// are poisson.hip's (poisson_internal.h).
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "poisson_exp.h"  // exp_full

size_t onehot_workspace_bytes_impl(const dlsa_onehot_plan* pl, int64_t n);
int onehot_plan_p(const dlsa_onehot_plan* pl);
int onehot_gram_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                     const double* w, int64_t n, double* H, int64_t ldh, void* ws, size_t ws_bytes, hipStream_t s, bool irls_weights);

// The skeleton of oh_logit_kernel with the Poisson terms.  Every thread runs the same number of rounds (the ordered mode has
// barriers inside): rows past n are clamped to row n - 1 and masked.  OFF = false reads no offsets.
template <bool OFF>
__global__ __launch_bounds__(OH_THREADS) void oh_poisson_kernel(OhDesc ds, const int32_t* __restrict__ level_col,
                                                                const double* __restrict__ num, int64_t ldn,
                                                                const int32_t* __restrict__ codes, int64_t ldc,
                                                                const double* __restrict__ y, const double* __restrict__ off,
                                                                const double* __restrict__ beta, int64_t n,
                                                                double* __restrict__ w_out, double* __restrict__ gpart,
                                                                double* __restrict__ llpart, int nrep) {
    extern __shared__ double sm[];
    double* sbeta = sm;                           // p
    double* sg = sm + ds.p;                       // nrep x p histograms of residuals (lanes spread over the copies)
    int* scol = reinterpret_cast<int*>(sm + (1 + nrep) * ds.p);     // nlev_total
    double* red = reinterpret_cast<double*>(scol + ((ds.nlev_total + 1) & ~1));
    for (int j = threadIdx.x; j < ds.p; j += blockDim.x) sbeta[j] = beta[j];
    for (int j = threadIdx.x; j < nrep * ds.p; j += blockDim.x) sg[j] = 0.0;
    double* sg_mine = sg + (threadIdx.x % nrep) * ds.p;
    for (int j = threadIdx.x; j < ds.nlev_total; j += blockDim.x) scol[j] = level_col[j];
    __syncthreads();
    double gd[OH_MAXD];
#pragma unroll
    for (int a = 0; a < OH_MAXD; ++a) gd[a] = 0.0;
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
        double eta = 0.0;
#pragma unroll
        for (int a = 0; a < OH_MAXD; ++a)
            if (a < ds.D) eta = fma(d[a], sbeta[ds.dense_col[a]], eta);
        int cols[OH_MAXF];
#pragma unroll
        for (int t = 0; t < OH_MAXF; ++t) {
            cols[t] = -1;
            if (t < ds.f) {
                const int code = codes[i * ldc + t];
                const int nl = ds.lvl_off[t + 1] - ds.lvl_off[t];
                if (code >= 0 && code < nl) cols[t] = scol[ds.lvl_off[t] + code];      // an unknown / baseline level contributes nothing
                if (cols[t] >= 0) eta += sbeta[cols[t]];
            }
        }
        const double yv = y[i];
        if constexpr (OFF) eta += off[i];
        const double mu = exp_full(eta);
        if (w_out && valid) w_out[i] = mu;
        const double r = valid ? yv - mu : 0.0;
        if (valid) ll += yv * eta - mu;
#pragma unroll
        for (int a = 0; a < OH_MAXD; ++a) gd[a] = fma(r, d[a], gd[a]);
        if (ds.ordered) {                           // one wave at a time, in wave order: a fixed order of the LDS adds
            for (int turn = 0; turn < nwaves; ++turn) {
                if (turn == mywave && valid) {
#pragma unroll
                    for (int t = 0; t < OH_MAXF; ++t)
                        if (t < ds.f && cols[t] >= 0) unsafeAtomicAdd(&sg_mine[cols[t]], r);
                }
                __syncthreads();
            }
        } else if (valid) {
#pragma unroll
            for (int t = 0; t < OH_MAXF; ++t)
                if (t < ds.f && cols[t] >= 0) unsafeAtomicAdd(&sg_mine[cols[t]], r);
        }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < OH_MAXD; ++a) {
        const double sgd = oh_block_sum(gd[a], red);
        if (threadIdx.x == 0 && a < ds.D) sg[ds.dense_col[a]] += sgd;
    }
    const double sll = oh_block_sum(ll, red);
    __syncthreads();
    double* gp = gpart + (int64_t)blockIdx.x * ds.p;
    for (int j = threadIdx.x; j < ds.p; j += blockDim.x) {
        double t = sg[j];
        for (int r = 1; r < nrep; ++r) t += sg[r * ds.p + j];      // fixed order
        gp[j] = t;
    }
    if (threadIdx.x == 0) llpart[blockIdx.x] = sll;
}

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
    l.off_state = take(pois_state_bytes(onehot_plan_p(pl)));
    l.total = o;
    return l;
}

static int oh_pois_ldn_min(const dlsa_onehot_plan* pl) {       // columns of num the plan reads
    int m = 0;
    for (int a = 0; a < pl->desc.D; ++a)
        if (pl->desc.dense_kind[a] == 1) m = std::max(m, pl->desc.dense_src[a] + 1);
    return m;
}

static int oh_pois_icpt_col(const dlsa_onehot_plan* pl) {      // the plan's constant column, -1 without one
    for (int a = 0; a < pl->desc.D; ++a)
        if (pl->desc.dense_kind[a] == 0) return pl->desc.dense_col[a];
    return -1;
}

// One partition at a fixed beta.  H (nullable) needs w (mu per row: the Gram's weights); g, loglik (the sum of y eta - mu,
// without the constant) nullable.  ws_oh: the structured passes' arena (256-aligned, >= onehot_workspace_bytes_impl(pl, n)).
static int oh_pois_pass_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                             const double* y, const double* off, const double* beta, int64_t n, double* H, int64_t ldh, double* g,
                             double* loglik, double* w, void* ws_oh, size_t ws_oh_bytes, hipStream_t s) {
    OhDesc ds = pl->desc;
    { const char* e = kernel_knob("DLSA_OH_ORDERED"); ds.ordered = e ? (atoi(e) != 0) : 1; }      // wave turn-taking unless 0
    ds.overflow = nullptr;
    const int nb = oh_logit_blocks(n);
    Arena ar(ws_oh, ws_oh_bytes);
    double* gpart = (double*)ar.take((size_t)nb * ds.p * sizeof(double));
    double* llpart = (double*)ar.take((size_t)nb * sizeof(double));
    if (!gpart || !llpart) {
        set_error("onehot poisson pass: the pass arena of %zu bytes is too small", ws_oh_bytes);
        return DLSA_ERR_WORKSPACE;
    }
    const int nrep = oh_logit_rep(ds.p);
    const size_t shm = (size_t)((1 + nrep) * ds.p + 16) * sizeof(double) + (size_t)((ds.nlev_total + 1) & ~1) * sizeof(int);
    if (off)
        hipLaunchKernelGGL(oh_poisson_kernel<true>, dim3(nb), dim3(OH_THREADS), shm, s, ds, (const int32_t*)pl->d_level_col, num, ldn,
                           codes, ldc, y, off, beta, n, w, gpart, llpart, nrep);
    else
        hipLaunchKernelGGL(oh_poisson_kernel<false>, dim3(nb), dim3(OH_THREADS), shm, s, ds, (const int32_t*)pl->d_level_col, num, ldn,
                           codes, ldc, y, off, beta, n, w, gpart, llpart, nrep);
    DLSA_HIP_CHECK(hipGetLastError());
    if (g || loglik) {
        logit_finish_launch((const double*)gpart, (const double*)llpart, nb, ds.p, ds.p, g, loglik, s, nullptr, nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    if (!H) return DLSA_OK;
    // (the Gram's partials overwrite the pass's in the same arena: the finish launch above has consumed them, in stream order)
    return onehot_gram_impl(pl, num, ldn, codes, ldc, w, n, H, ldh, ws_oh, ws_oh_bytes, s, false);
}

static int oh_pois_check_rows(const char* who, const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes,
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
    if (!ws || ws_bytes < l.total || ((uintptr_t)ws & 255)) {
        set_error("onehot_poisson_pass: workspace %zu bytes needed (256-aligned), got %zu", l.total, ws_bytes);
        return DLSA_ERR_WORKSPACE;
    }
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
    if (!ws || ws_bytes < l.total || ((uintptr_t)ws & 255)) {
        set_error("onehot_poisson_fit: workspace %zu bytes needed (256-aligned), got %zu", l.total, ws_bytes);
        return DLSA_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    PoisFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.ybuf = (double*)(wsc + l.off_y); b.obuf = (double*)(wsc + l.off_o);
    b.st = pois_state_at(wsc + l.off_state, p);
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
