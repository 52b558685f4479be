// Multinomial logistic (softmax) regression map step for a response with C unordered classes, 2 <= C <= 8: one partition's
// log-likelihood, score and information at a fixed theta, and the per-partition Newton fit on top of it.  The first family whose
// parameter is a matrix: J = C - 1 non-reference classes with pe = p + intercept coefficients each.  The block a partition returns
// (coef, Sig_inv = the information at coef, Sig_inv coef) has dimension J pe and feeds the unchanged one-round combine.
//
// Layout: y holds the class codes 0 .. C - 1 as doubles; class 0 is the reference (eta_0 = 0).  theta is class-major,
// theta = [beta_1 | ... | beta_J], every beta_j with pe entries, intercept first.  g has J pe entries, H is (J pe) x (J pe) with both
// triangles; the probabilities P are stored class-major, P[(j - 1) ld + i] = p_j of row i.
//
// Algebra (one partition; D = [1 | X] with the implicit intercept, X otherwise):
//   eta_j = D beta_j,  p_j = e^eta_j / sum_k e^eta_k,  loglik = sum_i log p_{y_i},
//   g_j = D'(1[y = j] - p_j),  H_jk = D' diag(p_j (delta_jk - p_k)) D   (observed = expected information).
// The softmax of a row: M = max(0, eta_1 .. eta_J), every exponential takes a non-positive argument, the first term that attains M
// is exactly 1 and is left out of T = the sum of the others, so S = 1 + T, log S = log1p(T) and the row's term eta_y - M - log1p(T)
// keeps its relative accuracy when one class dominates.
//
// Launches per evaluation (every partial combines in a fixed order: no float atomics, no waits between workgroups):
//   1 mn_pass_kernel        one read of the rows on the dense row-pass skeleton (row_pass.h, rowdot.h: lane l holds the columns
//                           128c + 2l + {0,1}, RB rows per wave and batch, branch-free clamped non-temporal loads): J dot products
//                           per row (one merged butterfly each), the softmax on the lanes of the row, J residuals broadcast into J
//                           accumulator sets; P (when wanted), per-block partials of g, of the J intercept entries and of loglik.
//                           The coefficients sit in LDS (J p doubles <= 16 KiB, padded to the chunks) and are read once per batch.
//   J logit_finish_launch   the fixed-order column sums of the partials, one per class block (logit.hip, shared);
//   per pair j <= k         mn_weight_kernel (w = p_j (delta_jk - p_k) into ONE reused n-vector) and the Gram dispatch on (X, w)
//                           straight into H at row j pe, column k pe with the pitch J pe (gram_icpt_impl with its own border pass
//                           under an intercept): J (J + 1) / 2 Gram passes per evaluation, the model's arithmetic;
//   1 mn_mirror_kernel      the blocks (j, k), j < k, copied to (k, j): a block is symmetric in itself, so no transpose.
// Once per partition: mn_check_kernel (the C class counts -> the intercepts' start log(n_j / n_0), the exact MLE of the
// intercept-only model, and the rows whose response is no class code).
#include "common.h"
#include "poisson_internal.h"
#include "multinomial_internal.h"   // the limits, mn_softmax_row, mn_fit_core, the launchers the structured sibling shares
#include <math.h>
#include <algorithm>
#include <vector>

namespace dlsa {

#include "rowdot.h"       // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "row_pass.h"     // the batch load, loop and block reduction, count_nc, count_rb, count_blocks, COUNT_*, the dispatcher

struct MnArgs {
    const double* X;
    const double* y;
    const double* theta;   // J * pe, class-major, intercept first
    double* prob;          // [J][ldprob] (nullable)
    double* gpart;         // [nblocks][J * NC * 128]
    double* llpart;        // [nblocks]
    double* s0part;        // [J][COUNT_MAX_BLOCKS]: sums of the residuals (the intercepts' entries of g)
    int64_t ldx, n, ldprob;
    int p, icpt;
};

// The skeleton of row_pass.h with J linear predictors per row.
template <int J, int NC, int RB, bool VEC>
__global__ __launch_bounds__(COUNT_THREADS) void mn_pass_kernel(MnArgs a) {
    constexpr int W = NC * 128;                     // padded columns of one class block
    __shared__ __attribute__((aligned(16))) double sh[J * W + 1 + J];      // the coefficients, then the block reduction
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int pe = a.p + a.icpt;
    for (int i = tid; i < J * W; i += COUNT_THREADS) {
        const int j = i / W, col = i - j * W;
        sh[i] = col < a.p ? a.theta[j * pe + a.icpt + col] : 0.0;           // clamped columns meet beta = 0
    }
    double b0[J], s0[J];
    double2 g[J][NC];
    double ll = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        b0[j] = a.icpt ? a.theta[j * pe] : 0.0;
        s0[j] = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) { g[j][c].x = 0.0; g[j][c].y = 0.0; }
    }
    __syncthreads();
    const int myrow = row_of_lane<RB>(lane);
    const bool rep = (lane & rep_mask<RB>()) == 0;

    auto load_batch = [&](int64_t bt, double2 (&x)[RB][NC], double& yv) {
        yv = a.y[row_pass_load<NC, RB, VEC>(a.X, a.ldx, a.n, a.p, bt, lane, myrow, x)];
    };
    auto process = [&](int64_t bt, const double2 (&x)[RB][NC], const double yraw) {
        const int64_t r = bt * RB + myrow;
        const bool valid = r < a.n;
        double eta[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            double2 bj[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) bj[c] = *reinterpret_cast<const double2*>(sh + j * W + c * 128 + 2 * lane);
            double dot[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < NC; ++c) s = fma(x[i][c].x, bj[c].x, fma(x[i][c].y, bj[c].y, s));
                dot[i] = s;
            }
            eta[j] = merged_reduce<RB>(dot, lane) + b0[j];
        }
        double pr[J];                                                 // the softmax of the lane's row (multinomial_internal.h)
        const double term = mn_softmax_row<J>(eta, yraw, pr);
        if (valid && rep) ll += term;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const double pj = pr[j];
            const double resid = valid ? (yraw == (double)(j + 1) ? 1.0 : 0.0) - pj : 0.0;
            if (valid && rep) {
                if (a.prob) a.prob[j * a.ldprob + r] = pj;
                s0[j] += resid;
            }
            rank1_update<RB, NC, 0>(resid, x, g[j]);
        }
    };

    row_pass_stream<NC, RB, double>(a.n, wave, load_batch, process);

    __syncthreads();                                // the coefficients are no longer read: their LDS takes the block reduction
    double sc[1 + J];
    sc[0] = ll;
#pragma unroll
    for (int j = 0; j < J; ++j) sc[1 + j] = s0[j];
    row_pass_reduce(g, sc, sh, lane, wave);
    double* gp = a.gpart + (int64_t)blockIdx.x * (J * W);
    for (int col = tid; col < J * W; col += COUNT_THREADS) gp[col] = sh[col];
    if (tid == 0) a.llpart[blockIdx.x] = sh[J * W];
    if (tid < J) a.s0part[(int64_t)tid * COUNT_MAX_BLOCKS + blockIdx.x] = sh[J * W + 1 + tid];
}

// ---- once per partition: [rows of class 0 .. 7, rows whose response is not finite, not integral, < 0 or >= C] ----------
__global__ __launch_bounds__(256) void mn_check_kernel(const double* __restrict__ y, int64_t n, int classes, double* __restrict__ part) {
    __shared__ double red[4][MN_NQ];
    double acc[MN_NQ];
#pragma unroll
    for (int q = 0; q < MN_NQ; ++q) acc[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yv = y[i];
        const bool ok = yv >= 0.0 && yv < (double)classes && yv == floor(yv);      // (NaN fails yv >= 0)
#pragma unroll
        for (int q = 0; q < MN_MAX_CLASSES; ++q) acc[q] += (ok && yv == (double)q) ? 1.0 : 0.0;
        acc[MN_BAD] += ok ? 0.0 : 1.0;
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < MN_NQ; ++q) {
        const double t = wave_allreduce_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) red[wave][q] = t;
    }
    __syncthreads();
    if (threadIdx.x < MN_NQ) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) t += red[k][threadIdx.x];
        part[(int64_t)blockIdx.x * MN_NQ + threadIdx.x] = t;
    }
}

// one wave per quantity, the block partials in a fixed order (counts: exact in any order)
__global__ __launch_bounds__(64 * MN_NQ) void mn_check_finish_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int b = lane; b < nblocks; b += 64) s += part[(int64_t)b * MN_NQ + q];
    s = wave_allreduce_sum(s);
    if (lane == 0) out[q] = s;
}

// the pass entry's log-likelihood: NaN when a row is not a class code
__global__ void mn_ll_fix_kernel(double* __restrict__ ll, const double* __restrict__ cst) {
    if (threadIdx.x == 0 && cst[MN_BAD] > 0.0) ll[0] = NAN;
}

// Newton start: theta = 0, the constant column of class block j (entry j * pe + icpt_col; -1: none) at b0[j]
__global__ void mn_start_kernel(double* __restrict__ theta, int J, int pe, int icpt_col, MnStart st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < J * pe) theta[i] = (icpt_col >= 0 && i % pe == icpt_col) ? st.b0[i / pe] : 0.0;
}

// w = p_j (delta_jk - p_k): the weights of the block (j, k) of the information
__global__ void mn_weight_kernel(const double* __restrict__ pj, const double* __restrict__ pk, int same, int64_t n, double* __restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = same ? pj[i] * (1.0 - pj[i]) : -(pj[i] * pk[i]);
}

// the blocks below the block diagonal from their mirror images above it (a block is symmetric in itself)
__global__ void mn_mirror_kernel(double* __restrict__ H, int64_t ldh, int J, int pe) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (c >= J * pe) return;
    const int br = r / pe, bc = c / pe;
    if (br > bc) H[(int64_t)r * ldh + c] = H[(int64_t)(bc * pe + (r - br * pe)) * ldh + br * pe + (c - bc * pe)];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// J pe <= 2048 bounds the chunks of a class block: 16 at J = 1, 8 at J <= 3, 4 beyond.  A shape without a kernel is an error.
template <int J>
static int mn_launch(const MnArgs& a, int nc, bool vec, int blocks, hipStream_t s) {
    return row_pass_dispatch(nc, [&](auto sh) {
        constexpr int NC = decltype(sh)::NC, RB = decltype(sh)::RB;
        if constexpr (NC <= 4 || (NC == 8 && J <= 3) || (NC == 16 && J == 1)) {
            if (vec) hipLaunchKernelGGL((mn_pass_kernel<J, NC, RB, true>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
            else hipLaunchKernelGGL((mn_pass_kernel<J, NC, RB, false>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
            return (int)DLSA_OK;
        } else {
            set_error("multinomial: no row kernel for %d classes and %d column chunks", J + 1, nc);
            return (int)DLSA_ERR_INVALID;
        }
    });
}

struct MnLayout {
    size_t off_gpart, off_llpart, off_s0part, off_cpart, off_cst, off_w, off_prob, off_y, off_gram, gram_bytes, total;
    int64_t ldprob;
};

// pass scratch; row_step > 1: room for the gathered responses of a strided partition
static MnLayout mn_layout(int64_t max_rows, int p, int J, int64_t row_step) {
    MnLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.ldprob = mn_ldprob(n);
    l.off_gpart = take((size_t)COUNT_MAX_BLOCKS * J * count_nc(p) * 128 * sizeof(double));
    l.off_llpart = take(8 * (size_t)COUNT_MAX_BLOCKS);
    l.off_s0part = take(8 * (size_t)COUNT_MAX_BLOCKS * J);
    l.off_cpart = take(8 * (size_t)MN_NQ * MN_CHECK_BLOCKS);
    l.off_cst = take(8 * 16);
    l.off_w = take(8 * (size_t)n);
    l.off_prob = take(8 * (size_t)J * l.ldprob);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    // the Gram's workspace also serves the border pass of gram_icpt_impl
    l.gram_bytes = std::max(gram_workspace_bytes_impl(n, p, 8), logit_workspace_bytes_impl(n, p));
    l.off_gram = take(l.gram_bytes);
    l.total = o;
    return l;
}

// cst[0 .. 8] = the class counts and the bad rows of n responses
int mn_check(const double* y, int64_t n, int classes, double* cpart, double* cst, hipStream_t s) {
    const int blocks = (int)std::min<int64_t>(MN_CHECK_BLOCKS, std::max<int64_t>(1, (n + 255) / 256));
    hipLaunchKernelGGL(mn_check_kernel, dim3(blocks), dim3(256), 0, s, y, n, classes, cpart);
    hipLaunchKernelGGL(mn_check_finish_kernel, dim3(1), dim3(64 * MN_NQ), 0, s, (const double*)cpart, blocks, cst);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int mn_ll_fix(double* ll, const double* cst, hipStream_t s) {
    hipLaunchKernelGGL(mn_ll_fix_kernel, dim3(1), dim3(64), 0, s, ll, cst);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int mn_start(double* theta, int J, int pe, int icpt_col, const MnStart& st, hipStream_t s) {
    hipLaunchKernelGGL(mn_start_kernel, dim3((J * pe + 255) / 256), dim3(256), 0, s, theta, J, pe, icpt_col, st);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int mn_weight(const double* pj, const double* pk, int same, int64_t n, double* w, hipStream_t s) {
    hipLaunchKernelGGL(mn_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pj, pk, same, n, w);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int mn_mirror(double* H, int64_t ldh, int J, int pe, hipStream_t s) {
    if (J <= 1) return DLSA_OK;                  // one block: nothing below the block diagonal
    hipLaunchKernelGGL(mn_mirror_kernel, dim3((J * pe + 255) / 256, J * pe), dim3(256), 0, s, H, ldh, J, pe);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

// One partition at a fixed theta.  H (nullable; (J pe) x (J pe), pitch ldh) needs prob (J class rows of pitch ldprob >= n, each
// 256-byte aligned); g, loglik (the sum of log p_y), prob nullable otherwise.
static int mn_pass_impl(const double* X, int64_t ldx, const double* y, const double* theta, int classes, int64_t n, int p, int intercept,
                        double* H, int64_t ldh, double* g, double* loglik, double* prob, int64_t ldprob, char* ws, const MnLayout& l,
                        hipStream_t s) {
    const int J = classes - 1, icpt = intercept ? 1 : 0, pe = p + icpt;
    const int nc = count_nc(p), rb = count_rb(nc);
    MnArgs a{};
    a.X = X; a.y = y; a.theta = theta; a.prob = prob; a.ldx = ldx; a.n = n; a.ldprob = ldprob; a.p = p; a.icpt = icpt;
    a.gpart = (double*)(ws + l.off_gpart); a.llpart = (double*)(ws + l.off_llpart); a.s0part = (double*)(ws + l.off_s0part);
    const bool vec = row_pass_vec(X, ldx, p);
    const int blocks = count_blocks(n, rb);
    int rc;
    switch (J) {
        case 1: rc = mn_launch<1>(a, nc, vec, blocks, s); break;
        case 2: rc = mn_launch<2>(a, nc, vec, blocks, s); break;
        case 3: rc = mn_launch<3>(a, nc, vec, blocks, s); break;
        case 4: rc = mn_launch<4>(a, nc, vec, blocks, s); break;
        case 5: rc = mn_launch<5>(a, nc, vec, blocks, s); break;
        case 6: rc = mn_launch<6>(a, nc, vec, blocks, s); break;
        default: rc = mn_launch<7>(a, nc, vec, blocks, s); break;
    }
    if (rc) return rc;
    DLSA_HIP_CHECK(hipGetLastError());
    const int pitch = J * nc * 128;
    for (int j = 0; j < J && (g || (loglik && j == 0)); ++j) {
        logit_finish_launch(a.gpart + (size_t)j * nc * 128, a.llpart, blocks, pitch, p, g ? g + (size_t)j * pe + icpt : nullptr,
                            j == 0 ? loglik : nullptr, s, (g && icpt) ? a.s0part + (size_t)j * COUNT_MAX_BLOCKS : nullptr,
                            (g && icpt) ? g + (size_t)j * pe : nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    if (!H) return DLSA_OK;
    double* w = (double*)(ws + l.off_w);
    for (int j = 0; j < J; ++j) {
        for (int k = j; k < J; ++k) {
            rc = mn_weight(prob + j * ldprob, prob + k * ldprob, j == k ? 1 : 0, n, w, s);
            if (rc) return rc;
            double* Hjk = H + (size_t)j * pe * ldh + (size_t)k * pe;
            rc = icpt ? gram_icpt_impl(X, ldx, w, n, p, Hjk, ldh, ws + l.off_gram, l.gram_bytes, s)
                      : gram_impl_f64(X, ldx, w, n, p, Hjk, ldh, 0, ws + l.off_gram, l.gram_bytes, s);
            if (rc) return rc;
        }
    }
    return mn_mirror(H, ldh, J, pe, s);
}

int mn_coef_ok(const char* who, int pe, int classes) {
    DLSA_REQUIRE(classes >= 2 && classes <= MN_MAX_CLASSES, "%s: classes must lie in 2 .. %d, got %d", who, MN_MAX_CLASSES, classes);
    const int64_t d = (int64_t)(classes - 1) * pe;
    DLSA_REQUIRE(d <= 2048, "%s: (classes - 1) * (p + intercept) = %lld coefficients exceed the solver's 2048", who, (long long)d);
    return DLSA_OK;
}

static int mn_shape_ok(const char* who, int p, int intercept, int classes) {
    DLSA_REQUIRE(p > 0 || classes < 2 || classes > MN_MAX_CLASSES, "%s: bad shape p=%d", who, p);      // (the class count is judged first)
    return mn_coef_ok(who, p + (intercept ? 1 : 0), classes);
}

}  // namespace dlsa

extern "C" {

size_t dlsa_multinomial_workspace_bytes(int64_t max_rows, int p, int intercept, int classes, int64_t row_step) {
    if (p <= 0 || classes < 2 || classes > dlsa::MN_MAX_CLASSES || max_rows < 0 || row_step < 1) return 0;
    const int64_t d = (int64_t)(classes - 1) * (p + (intercept ? 1 : 0));
    if (d > 2048) return 0;
    return dlsa::align_up(dlsa::mn_layout(max_rows, p, classes - 1, row_step).total, 256) + dlsa::newton_state_bytes((int)d);
}

int dlsa_multinomial_pass_f64(const double* X, int64_t ldx, const double* y, const double* theta, int classes, int64_t n, int p,
                              int intercept, double* H, int64_t ldh, double* g, double* loglik, double* prob_out, int64_t ldprob,
                              void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && theta, "multinomial_pass: null X, y or theta");
    int rc = mn_shape_ok("multinomial_pass", p, intercept, classes);
    if (rc) return rc;
    const int J = classes - 1, d = J * (p + (intercept ? 1 : 0));
    DLSA_REQUIRE(n >= 1 && ldx >= p && (!H || ldh >= d), "multinomial_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld", (long long)n, p,
                 (long long)ldx, (long long)ldh);
    DLSA_REQUIRE(!prob_out || (ldprob >= n && ldprob % 32 == 0 && ((uintptr_t)prob_out & 255) == 0),
                 "multinomial_pass: prob_out needs 256-byte aligned class rows (ldprob >= n, a multiple of 32), got ldprob=%lld",
                 (long long)ldprob);
    const MnLayout l = mn_layout(n, p, J, 1);
    // (the pass carves l.total of it; the contract is the query, which also holds a fit's Newton state)
    rc = newton_check_ws("multinomial_pass", ws, ws_bytes, dlsa_multinomial_workspace_bytes(n, p, intercept, classes, 1));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    double* prob = prob_out ? prob_out : (H ? (double*)(wsc + l.off_prob) : nullptr);
    rc = mn_pass_impl(X, ldx, y, theta, classes, n, p, intercept, H, ldh, g, loglik, prob, prob_out ? ldprob : l.ldprob, wsc, l, s);
    if (rc || !loglik) return rc;
    rc = mn_check(y, n, classes, (double*)(wsc + l.off_cpart), (double*)(wsc + l.off_cst), s);
    if (rc) return rc;
    return mn_ll_fix(loglik, (const double*)(wsc + l.off_cst), s);
}

int dlsa_multinomial_fit_f64(const double* X, int64_t ldx, const double* y, const int64_t* part_first_host,
                             const int64_t* part_rows_host, int64_t row_step, int K, int p, int intercept, int classes, double tol,
                             int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                             double* loglik_host, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "multinomial_fit: null argument");
    int rc = mn_shape_ok("multinomial_fit", p, intercept, classes);
    if (rc) return rc;
    const int icpt = intercept ? 1 : 0, pe = p + icpt, J = classes - 1, d = J * pe;
    DLSA_REQUIRE(K > 0 && ldx >= p && row_step >= 1, "multinomial_fit: bad shape K=%d p=%d ldx=%lld step=%lld", K, p, (long long)ldx,
                 (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "multinomial_fit: bad tol/max_iter");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "multinomial_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const MnLayout l = mn_layout(max_rows, p, J, row_step);
    const size_t need = dlsa_multinomial_workspace_bytes(max_rows, p, intercept, classes, row_step);
    rc = newton_check_ws("multinomial_fit", ws, ws_bytes, need);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    MnFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.ybuf = (double*)(wsc + l.off_y);
    b.st = newton_state_at(wsc + align_up(l.total, 256), d);
    const int64_t pitch = ldx * row_step;                     // rows first, first + step, ...: a strided view, no copy of X
    auto eval = [=](int k, const double* yk, int64_t nk, const double* theta, double* Hk, double* g, double* ll) {
        return mn_pass_impl(X + part_first_host[k] * ldx, pitch, yk, theta, classes, nk, p, intercept, Hk, d, g, ll,
                            (double*)(wsc + l.off_prob), l.ldprob, wsc, l, s);
    };
    return mn_fit_core("multinomial_fit", MN_NO_CLASS, y, part_first_host, part_rows_host, row_step, K, d, classes, tol, max_iter, coef, Sig_inv,
                       Sig_invMcoef, n_iter_host, status_host, loglik_host, b, mn_null_start(J, pe, icpt ? 0 : -1), eval, s);
}

}  // extern "C"
