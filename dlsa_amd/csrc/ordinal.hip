// Ordinal (proportional-odds, cumulative logit) regression map step for a response with C ordered classes, 2 <= C <= 8: one
// partition's log-likelihood, score and observed information at a fixed theta, and the per-partition Newton fit on top of it.
// The block a partition returns (coef, Sig_inv = the information at coef, Sig_inv coef) has dimension d = J + p, J = C - 1, and feeds
// the unchanged one-round combine; the J cutpoints are the model's intercepts (include/dlsa_hip_ordinal.h holds the contract).
//
// Layout: y holds the class codes 0 .. C - 1 as doubles; theta = [alpha_1 .. alpha_J | beta_1 .. beta_p], cutpoints first.
//   logit P(y <= j) = alpha_{j+1} - x'beta,  j = 0 .. J - 1   (the sign convention of MASS::polr)
//
// Algebra (a row of class c, eta = x'beta, u = alpha_{c+1} - eta, l = alpha_c - eta, F the logistic cdf):
//   A = F(u), Abar = F(-u), B = F(l), Bbar = F(-l);  top class: A = 1, Abar = 0;  class 0: B = 0, Bbar = 1  (by select)
//   E_c = -expm1(-(alpha_{c+1} - alpha_c)) for an interior class, 1 for the two end classes: a function of theta alone
//   pi = A Bbar E (all factors positive: nothing cancels),  log pi = log A + log Bbar + log E
//   dl/deta = A + B - 1 = B - Abar,  -d2l/deta2 = w = A Abar + B Bbar >= 0
//   s_u = Abar / (Bbar E),  s_l = B / (A E),  q = s_u s_l
//   g_beta = X'(B - Abar),  g_alpha_j = sum_{y = j-1} s_u - sum_{y = j} s_l
//   N_bb = X' diag(w) X,  N_{alpha_j, beta} = X'v_j with v_j = -(1[y = j-1] A Abar + 1[y = j] B Bbar),
//   N_{alpha_j alpha_j} = sum_{y = j-1} (A Abar + q) + sum_{y = j} (B Bbar + q),  N_{alpha_j alpha_j+1} = -sum_{y = j} q.
// Cutpoints that are not strictly increasing give loglik = NaN (the launch stays harmless: the terms are selects and arithmetic).
//
// Launches per evaluation (every partial combines in a fixed order: no float atomics):
//   1 ord_pass_kernel       one read of the rows on the dense row-pass skeleton (row_pass.h, rowdot.h): one dot product per row, the
//                           terms above on the lanes of the row, the residual broadcast into the g set and -- BORDER, where the C
//                           accumulator sets of NC double2 fit (C NC <= 16) -- the row's v entries into the J border sets; w (and,
//                           without BORDER but with H, A Abar and B Bbar) per row; per-block partials of the sets, of the 3J - 1
//                           scalar sums and of loglik.
//   2 .. 3 logit_finish_launch   the fixed-order column sums: g_beta + loglik, the scalars, the border sets (logit.hip, shared);
//   without BORDER, per cutpoint: ord_mask_kernel (v_j into one reused n-vector) and xtv_impl: one more read of X each;
//   1 Gram dispatch on (X, w) straight into H at row J, column J with the pitch ldh;
//   1 ord_assemble_kernel   g_alpha, the J border rows and columns and the tridiagonal corner of H, both triangles.
// Once per partition: mn_check (the class counts -> the start alpha_j = logit of the cumulative class share, beta = 0: the exact
// MLE of the null model; and the rows whose response is no class code).
#include "common.h"
#include "poisson_internal.h"
#include "ordinal_internal.h"
#include "../../include/dlsa_hip_ordinal.h"
#include <math.h>
#include <algorithm>
#include <vector>

namespace dlsa {

#include "rowdot.h"       // merged_reduce, row_of_lane, rep_mask, rank1_update
#include "row_pass.h"     // the batch load, loop and block reduction, count_nc, count_rb, count_blocks, COUNT_*, the dispatcher

struct OrdArgs {
    const double* X;
    const double* y;
    const double* theta;   // [alpha_1 .. alpha_J | beta]
    double* w_out;         // A Abar + B Bbar per row (nullable)
    double* aa_out;        // A Abar per row (nullable; the masked vectors of the route without BORDER)
    double* bb_out;        // B Bbar per row (nullable, with aa_out)
    double* gpart;         // [nblocks][SETS * NC * 128]: the g set, then (BORDER) the J border sets
    double* llpart;        // [nblocks]
    double* scpart;        // [nblocks][ORD_SC]
    int64_t ldx, n;
    int p;
};

// The skeleton of row_pass.h with the ordinal terms and C accumulator sets.
template <int C, int NC, int RB, bool VEC, bool BORDER>
__global__ __launch_bounds__(COUNT_THREADS) void ord_pass_kernel(OrdArgs a) {
    constexpr int J = C - 1;
    constexpr int SETS = BORDER ? C : 1;
    constexpr int W = NC * 128;
    constexpr int NS = 3 * J - 1;                   // the scalar sums: g_alpha, the corner's diagonal and off-diagonal
    __shared__ double red[SETS * W + 1 + ORD_SC];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    double al[J], E[C], logE[C];
    const bool ordered = ord_cutpoints<J>(a.theta, al, E, logE);
    double sc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) sc[i] = 0.0;
    double ll = 0.0;
    double2 b[NC], g[SETS][NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 128 + 2 * lane;
        b[c].x = col < a.p ? a.theta[J + col] : 0.0;               // clamped columns meet beta = 0
        b[c].y = col + 1 < a.p ? a.theta[J + col + 1] : 0.0;
#pragma unroll
        for (int k = 0; k < SETS; ++k) { g[k][c].x = 0.0; g[k][c].y = 0.0; }
    }
    const int myrow = row_of_lane<RB>(lane);
    const bool rep = (lane & rep_mask<RB>()) == 0;

    auto load_batch = [&](int64_t bt, double2 (&x)[RB][NC], double& yv) {
        yv = a.y[row_pass_load<NC, RB, VEC>(a.X, a.ldx, a.n, a.p, bt, lane, myrow, x)];
    };
    auto process = [&](int64_t bt, const double2 (&x)[RB][NC], const double yraw) {
        double dot[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) s = fma(x[i][c].x, b[c].x, fma(x[i][c].y, b[c].y, s));
            dot[i] = s;
        }
        const int64_t r = bt * RB + myrow;
        const bool valid = r < a.n;
        const bool mine = valid && rep;
        const double eta = merged_reduce<RB>(dot, lane);
        double llt, resid, aa, bb, su, sl, q;
        ord_row_terms<J>(yraw, eta, al, E, logE, llt, resid, aa, bb, su, sl, q);
        if (mine) {
            if (a.w_out) a.w_out[r] = aa + bb;
            if (a.aa_out) { a.aa_out[r] = aa; a.bb_out[r] = bb; }
            ll += llt;
        }
#pragma unroll
        for (int j = 0; j < J; ++j) ord_cutpoint_sums<J>(j, yraw, mine, su, sl, aa, bb, q, sc);
        rank1_update<RB, NC, 0>(valid ? resid : 0.0, x, g[0]);
        if constexpr (BORDER) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double vj = -((valid && yraw == (double)j ? aa : 0.0) + (valid && yraw == (double)(j + 1) ? bb : 0.0));
                rank1_update<RB, NC, 0>(vj, x, g[1 + j]);
            }
        }
    };

    row_pass_stream<NC, RB, double>(a.n, wave, load_batch, process);

    double rs[1 + NS];                              // loglik, then the scalar sums
    rs[0] = ll;
#pragma unroll
    for (int i = 0; i < NS; ++i) rs[1 + i] = sc[i];
    row_pass_reduce(g, rs, red, lane, wave);
    double* gp = a.gpart + (int64_t)blockIdx.x * (SETS * W);
    for (int col = tid; col < SETS * W; col += COUNT_THREADS) gp[col] = red[col];
    if (tid == 0) a.llpart[blockIdx.x] = ordered ? red[SETS * W] : NAN;
    if (tid < ORD_SC) {                             // the block's row of scalars in the layout of ordinal_internal.h
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) v = ord_sc_slot<J>(i) == tid ? red[SETS * W + 1 + i] : v;
        a.scpart[(int64_t)blockIdx.x * ORD_SC + tid] = v;
    }
}

// v_j = -(1[y = j - 1] A Abar + 1[y = j] B Bbar) for cutpoint j (1-based) of the route without in-pass borders
__global__ void ord_mask_kernel(const double* __restrict__ y, const double* __restrict__ aa, const double* __restrict__ bb, int j,
                                int64_t n, double* __restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = -((y[i] == (double)(j - 1) ? aa[i] : 0.0) + (y[i] == (double)j ? bb[i] : 0.0));
}

// g_alpha (nullable; with gbeta also g_beta, copied), and of H (nullable; d x d, pitch ldh) the J border rows and columns and the
// tridiagonal corner, both triangles, from the finished sums: sc (layout of ordinal_internal.h) and the border vectors
// bd[j * ldbd + k] = (X'v_{j+1})_k.
__global__ void ord_assemble_kernel(const double* __restrict__ sc, const double* __restrict__ bd, int ldbd, int J, int p,
                                    double* __restrict__ H, int64_t ldh, double* __restrict__ g, const double* __restrict__ gbeta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (g && i < J) g[i] = sc[ORD_SC_GA + i];
    if (g && gbeta && i < p) g[J + i] = gbeta[i];
    if (!H) return;
    if (i < J * p) {
        const int j = i / p, k = i - j * p;
        const double v = bd[(int64_t)j * ldbd + k];
        H[(int64_t)j * ldh + J + k] = v;
        H[(int64_t)(J + k) * ldh + j] = v;
    }
    if (i < J * J) {
        const int r = i / J, c = i - r * J;
        const int lo = r < c ? r : c;
        H[(int64_t)r * ldh + c] = r == c ? sc[ORD_SC_DG + r] : ((r - c == 1 || c - r == 1) ? sc[ORD_SC_OF + lo] : 0.0);
    }
}

// Newton start: the cutpoints at st.a, beta = 0
__global__ void ord_start_kernel(double* __restrict__ theta, int J, int d, OrdStart st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d) theta[i] = i < J ? st.a[i] : 0.0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the launchers onehot_ordinal.hip shares (ordinal_internal.h)
int ord_mask(const double* y, const double* aa, const double* bb, int j, int64_t n, double* v, hipStream_t s) {
    hipLaunchKernelGGL(ord_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, aa, bb, j, n, v);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int ord_assemble(const double* sc, const double* bd, int ldbd, int J, int p, double* H, int64_t ldh, double* g, const double* gbeta,
                 hipStream_t s) {
    const int cells = std::max(J * p, J * J);
    hipLaunchKernelGGL(ord_assemble_kernel, dim3((cells + 255) / 256), dim3(256), 0, s, sc, bd, ldbd, J, p, H, ldh, g, gbeta);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int ord_start(double* theta, int J, int d, const OrdStart& st, hipStream_t s) {
    hipLaunchKernelGGL(ord_start_kernel, dim3((d + 255) / 256), dim3(256), 0, s, theta, J, d, st);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

// BORDER is instantiated where C NC <= ORD_BORDER_SETS (ord_border_in_pass): the caller asks for it nowhere else
template <int C>
static void ord_launch(const OrdArgs& a, int nc, bool vec, bool border, int blocks, hipStream_t s) {
    row_pass_dispatch(nc, [&](auto sh) {
        constexpr int NC = decltype(sh)::NC, RB = decltype(sh)::RB;
        if constexpr (C * NC <= ORD_BORDER_SETS) {
            if (border) {
                if (vec) hipLaunchKernelGGL((ord_pass_kernel<C, NC, RB, true, true>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
                else hipLaunchKernelGGL((ord_pass_kernel<C, NC, RB, false, true>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
                return;
            }
        }
        if (vec) hipLaunchKernelGGL((ord_pass_kernel<C, NC, RB, true, false>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
        else hipLaunchKernelGGL((ord_pass_kernel<C, NC, RB, false, false>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
    });
}

struct OrdLayout {
    size_t off_gpart, off_llpart, off_scpart, off_cpart, off_cst, off_sc, off_bd, off_w, off_aa, off_bb, off_v, off_y, off_gram,
        gram_bytes, total;
};

// pass scratch; row_step > 1: room for the gathered responses of a strided partition
static OrdLayout ord_layout(int64_t max_rows, int p, int classes, int64_t row_step) {
    OrdLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    const int J = classes - 1, nc = count_nc(p);
    const bool border = ord_border_in_pass(classes, nc);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.off_gpart = take((size_t)COUNT_MAX_BLOCKS * (border ? classes : 1) * nc * 128 * sizeof(double));
    l.off_llpart = take(8 * (size_t)COUNT_MAX_BLOCKS);
    l.off_scpart = take(8 * (size_t)COUNT_MAX_BLOCKS * ORD_SC);
    l.off_cpart = take(8 * (size_t)MN_NQ * MN_CHECK_BLOCKS);
    l.off_cst = take(8 * 16);
    l.off_sc = take(8 * ORD_SC);
    l.off_bd = take(8 * (size_t)J * nc * 128);
    l.off_w = take(8 * (size_t)n);
    l.off_aa = take(border ? 0 : 8 * (size_t)n);
    l.off_bb = take(border ? 0 : 8 * (size_t)n);
    l.off_v = take(border ? 0 : 8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    // the Gram's workspace also serves xtv_impl on the route without in-pass borders
    l.gram_bytes = std::max(gram_workspace_bytes_impl(n, p, 8), logit_workspace_bytes_impl(n, p));
    l.off_gram = take(l.gram_bytes);
    l.total = o;
    return l;
}

// One partition at a fixed theta.  H (nullable; d x d, pitch ldh), g, loglik, w_out nullable.
static int ord_pass_impl(const double* X, int64_t ldx, const double* y, const double* theta, int classes, int64_t n, int p, double* H,
                         int64_t ldh, double* g, double* loglik, double* w_out, char* ws, const OrdLayout& l, hipStream_t s) {
    const int J = classes - 1;
    const int nc = count_nc(p), rb = count_rb(nc), W = nc * 128;
    const bool border = H && ord_border_in_pass(classes, nc);
    const bool masked = H && !border;
    OrdArgs a{};
    a.X = X; a.y = y; a.theta = theta; a.ldx = ldx; a.n = n; a.p = p;
    a.w_out = w_out ? w_out : (H ? (double*)(ws + l.off_w) : nullptr);
    a.aa_out = masked ? (double*)(ws + l.off_aa) : nullptr;
    a.bb_out = masked ? (double*)(ws + l.off_bb) : nullptr;
    a.gpart = (double*)(ws + l.off_gpart); a.llpart = (double*)(ws + l.off_llpart); a.scpart = (double*)(ws + l.off_scpart);
    const bool vec = row_pass_vec(X, ldx, p);
    const int blocks = count_blocks(n, rb);
    switch (classes) {
        case 2: ord_launch<2>(a, nc, vec, border, blocks, s); break;
        case 3: ord_launch<3>(a, nc, vec, border, blocks, s); break;
        case 4: ord_launch<4>(a, nc, vec, border, blocks, s); break;
        case 5: ord_launch<5>(a, nc, vec, border, blocks, s); break;
        case 6: ord_launch<6>(a, nc, vec, border, blocks, s); break;
        case 7: ord_launch<7>(a, nc, vec, border, blocks, s); break;
        default: ord_launch<8>(a, nc, vec, border, blocks, s); break;
    }
    DLSA_HIP_CHECK(hipGetLastError());
    const int pitch = (border ? classes : 1) * W;
    double* sc = (double*)(ws + l.off_sc);
    double* bd = (double*)(ws + l.off_bd);
    if (g || loglik) {
        logit_finish_launch(a.gpart, a.llpart, blocks, pitch, p, g ? g + J : nullptr, loglik, s, nullptr, nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    if (!g && !H) return DLSA_OK;
    logit_finish_launch(a.scpart, nullptr, blocks, ORD_SC, ORD_SC, sc, nullptr, s, nullptr, nullptr);
    DLSA_HIP_CHECK(hipGetLastError());
    if (border) {
        logit_finish_launch(a.gpart + W, nullptr, blocks, pitch, J * W, bd, nullptr, s, nullptr, nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    if (masked) {
        double* v = (double*)(ws + l.off_v);
        for (int j = 1; j <= J; ++j) {
            int rc = ord_mask(y, a.aa_out, a.bb_out, j, n, v, s);
            if (rc) return rc;
            rc = xtv_impl(X, ldx, v, n, p, bd + (size_t)(j - 1) * W, nullptr, nullptr, ws + l.off_gram, l.gram_bytes, s);
            if (rc) return rc;
        }
    }
    if (H) {
        const int rc = gram_impl_f64(X, ldx, a.w_out, n, p, H + (size_t)J * ldh + J, ldh, 0, ws + l.off_gram, l.gram_bytes, s);
        if (rc) return rc;
    }
    return ord_assemble(sc, bd, W, J, p, H, ldh, g, nullptr, s);
}

static int ord_shape_ok(const char* who, int p, int classes) {
    DLSA_REQUIRE(classes >= 2 && classes <= ORD_MAX_CLASSES, "%s: classes must lie in 2 .. %d, got %d", who, ORD_MAX_CLASSES, classes);
    DLSA_REQUIRE(p > 0, "%s: bad shape p=%d", who, p);
    const int64_t d = (int64_t)(classes - 1) + p;
    DLSA_REQUIRE(d <= 2048, "%s: d = (classes - 1) + p = %lld coefficients exceed the solver's 2048", who, (long long)d);
    return DLSA_OK;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_ordinal_workspace_bytes(int64_t max_rows, int p, int classes, int64_t row_step) {
    if (p <= 0 || classes < 2 || classes > dlsa::ORD_MAX_CLASSES || max_rows < 0 || row_step < 1) return 0;
    const int64_t d = (int64_t)(classes - 1) + p;
    if (d > 2048) return 0;
    return dlsa::align_up(dlsa::ord_layout(max_rows, p, classes, row_step).total, 256) + dlsa::newton_state_bytes((int)d);
}

int dlsa_ordinal_pass_f64(const double* X, int64_t ldx, const double* y, const double* theta, int classes, int64_t n, int p, double* H,
                          int64_t ldh, double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && theta, "ordinal_pass: null X, y or theta");
    int rc = ord_shape_ok("ordinal_pass", p, classes);
    if (rc) return rc;
    const int d = classes - 1 + p;
    DLSA_REQUIRE(n >= 1 && ldx >= p && (!H || ldh >= d), "ordinal_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld", (long long)n, p,
                 (long long)ldx, (long long)ldh);
    const OrdLayout l = ord_layout(n, p, classes, 1);
    // (the pass carves l.total of it; the contract is the query, which also holds a fit's Newton state)
    rc = newton_check_ws("ordinal_pass", ws, ws_bytes, dlsa_ordinal_workspace_bytes(n, p, classes, 1));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    rc = ord_pass_impl(X, ldx, y, theta, classes, n, p, H, ldh, g, loglik, w_out, wsc, l, s);
    if (rc || !loglik) return rc;
    rc = mn_check(y, n, classes, (double*)(wsc + l.off_cpart), (double*)(wsc + l.off_cst), s);
    if (rc) return rc;
    return mn_ll_fix(loglik, (const double*)(wsc + l.off_cst), s);
}

// The per-partition driver is mn_fit_core (multinomial_internal.h, shared with the multinomial fits): the data check of EVERY
// partition first, then per partition the null model's start, newton_fit_loop with the policy NEWTON_POISSON on d coefficients and
// newton_fit_finish.
int dlsa_ordinal_fit_f64(const double* X, int64_t ldx, const double* y, const int64_t* part_first_host, const int64_t* part_rows_host,
                         int64_t row_step, int K, int p, int classes, double tol, int max_iter, double* coef, double* Sig_inv,
                         double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, void* ws, size_t ws_bytes,
                         void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef,
                 "ordinal_fit: null argument (X, y, the partitions, coef, Sig_inv and Sig_invMcoef are required)");
    int rc = ord_shape_ok("ordinal_fit", p, classes);
    if (rc) return rc;
    const int d = classes - 1 + p;
    DLSA_REQUIRE(K > 0 && ldx >= p && row_step >= 1, "ordinal_fit: bad shape K=%d p=%d ldx=%lld step=%lld", K, p, (long long)ldx,
                 (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "ordinal_fit: bad tol/max_iter");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "ordinal_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const OrdLayout l = ord_layout(max_rows, p, classes, row_step);
    rc = newton_check_ws("ordinal_fit", ws, ws_bytes, dlsa_ordinal_workspace_bytes(max_rows, p, classes, row_step));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    MnFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.ybuf = (double*)(wsc + l.off_y);
    b.st = newton_state_at(wsc + align_up(l.total, 256), d);
    const int64_t pitch = ldx * row_step;                     // rows first, first + step, ...: a strided view, no copy of X
    auto eval = [=](int k, const double* yk, int64_t nk, const double* theta, double* Hk, double* g, double* ll) {
        return ord_pass_impl(X + part_first_host[k] * ldx, pitch, yk, theta, classes, nk, p, Hk, d, g, ll, nullptr, wsc, l, s);
    };
    return mn_fit_core("ordinal_fit", ORD_NO_CLASS, y, part_first_host, part_rows_host, row_step, K, d, classes, tol, max_iter, coef, Sig_inv,
                       Sig_invMcoef, n_iter_host, status_host, loglik_host, b, ord_null_start(classes - 1, d), eval, s);
}

}  // extern "C"
