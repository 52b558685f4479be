// Structured ordinal (proportional-odds) map step for one-hot designs: the pass and fit of ordinal.hip on the RAW representation of a
// design [standardised numerics | one-hot factor levels] (num [n, q] fp64, codes [n, f] int32) under a dlsa_onehot_plan -- the dense
// n x p matrix is never built.  Results equal the dense ordinal entries on the matrix dlsa_design_f64 would build (to rounding).
// The plan has NO constant column: the J cutpoints are the intercepts (include/dlsa_hip_onehot_ordinal.h holds the contract).
//
// Layout: as ordinal.hip with p = the plan's p: y holds the class codes 0 .. C - 1 as doubles, J = C - 1, theta = [alpha_1 ..
// alpha_J | beta] (beta in the plan's column order), g has d = J + p entries, H is d x d with both triangles.
//
// Launches per evaluation at a fixed theta:
//   1 oh_ord_row_kernel<J, BORDER>   one thread per row on the skeleton of oh_mn_row_kernel (onehot_multinomial.hip): ONE gather
//                           eta = d . beta_D + sum_t beta[col(t, code_t)] from beta in LDS, the row's terms by ord_row_terms
//                           (ordinal_internal.h, shared with the dense kernel), r = B - Abar into the g set; BORDER: a row of
//                           class c adds -A Abar into border set c + 1 (c < J) and -B Bbar into border set c (c >= 1) -- two sets
//                           per row whatever C is.  Level columns are LDS adds into the thread's copy of a `cells`-cell histogram
//                           (wave turn-taking: a fixed order of the adds, bit-reproducible); the dense columns of all C sets sit in
//                           registers and are fed by selects (the register table of profiles/onehot_ordinal_stats.txt: no
//                           instantiation spills, and a dense column is the one address every lane of a wave would add to).  The
//                           3J - 1 scalar sums are per-thread accumulators fed by selects, as in ord_pass_kernel.  w = A Abar +
//                           B Bbar per row (and, without BORDER but with H, A Abar and B Bbar).
//   2 logit_finish_launch   the fixed-order column sums over all `cells` columns at once ([g_beta | J border vectors], contiguous)
//                           and over the blocks' rows of ORD_SC scalars (logit.hip, shared);
//   without BORDER, per cutpoint: ord_mask (v_j into one reused n-vector) and one structured X'v_j through oh_row_kernel
//                           (onehot_pass.h) with the row model OhXtvRow of this unit;
//   1 onehot_gram_impl(plan, num, codes, w) straight into H at row J, column J with the pitch of H: ordered floating point;
//   1 ord_assemble          g (g_alpha and the copy of g_beta), the J border rows and columns and the tridiagonal corner of H.
// LDS of the row kernel: beta and the cutpoints (p + J doubles), nrep histogram copies of `cells` doubles (cells = C p with BORDER,
// p without), the level-column table, the block reduction's 16 doubles.  oh_ord_border / oh_ord_rep below hold the rule.
// Traffic per row: 8q + 4f + 8 (y) + 8 (w written) bytes for the pass, 8q + 4f + 8 for the Gram.
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include "ordinal_internal.h"
#include "../../include/dlsa_hip_onehot_ordinal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "onehot_pass.h"  // oh_row_kernel, oh_row_pass (the masked border route)

constexpr size_t OH_ORD_LDS_BUDGET = 32 * 1024;      // oh_logit_rep's budget

// the borders are taken in the pass where one copy of the C p-cell histogram fits the budget beside beta and the cutpoints
static bool oh_ord_border(int p, int classes) {
    return (size_t)(p + (classes - 1) + classes * p) * sizeof(double) <= OH_ORD_LDS_BUDGET;
}
// histogram copies: the largest of 8, 4, 2, 1 that keeps beta, the cutpoints and the copies within the budget
static int oh_ord_rep(int p, int J, int cells) {
    int r = OH_LOGIT_REP;
    while (r > 1 && (size_t)(p + J + r * cells) * sizeof(double) > OH_ORD_LDS_BUDGET) r /= 2;
    return r;
}

struct OhOrdArgs {
    const double* num; const int32_t* codes; const double* y; const double* theta;
    int64_t ldn, ldc, n;
    double* w_out;         // A Abar + B Bbar per row (nullable)
    double* aa_out;        // A Abar per row (nullable; the masked vectors of the route without BORDER)
    double* bb_out;        // B Bbar per row (nullable, with aa_out)
    double* gpart;         // [nblocks][cells]: the g set, then (BORDER) the J border sets of p cells each
    double* llpart;        // [nblocks]
    double* scpart;        // [nblocks][ORD_SC]
    int nrep;
};

// One thread per row; every thread runs the same number of rounds (the ordered mode has barriers inside): rows past n are clamped
// and masked.  Nothing is indexed by y: the class of a row is a sum of compare results (0 for a value that is no class code).
template <int J, bool BORDER>
__global__ __launch_bounds__(OH_THREADS) void oh_ord_row_kernel(OhDesc ds, const int32_t* __restrict__ level_col, OhOrdArgs a) {
    constexpr int C = J + 1;
    constexpr int SETS = BORDER ? C : 1;
    constexpr int NS = 3 * J - 1;                 // the scalar sums: g_alpha, the corner's diagonal and off-diagonal
    extern __shared__ double sm[];
    const int p = ds.p, cells = SETS * p, nrep = a.nrep;
    double* sbeta = sm;                           // p, then the J cutpoints
    double* sg = sm + p + J;                      // nrep x cells (lanes spread over the copies)
    int* scol = reinterpret_cast<int*>(sg + nrep * cells);          // nlev_total
    double* red = reinterpret_cast<double*>(scol + ((ds.nlev_total + 1) & ~1));
    for (int c = threadIdx.x; c < p + J; c += blockDim.x) sbeta[c] = c < p ? a.theta[J + c] : a.theta[c - p];
    for (int c = threadIdx.x; c < nrep * cells; c += blockDim.x) sg[c] = 0.0;
    double* sg_mine = sg + (threadIdx.x % nrep) * cells;
    for (int c = threadIdx.x; c < ds.nlev_total; c += blockDim.x) scol[c] = level_col[c];
    __syncthreads();
    double al[J], E[C], logE[C];                  // once per launch
    const bool ordered = ord_cutpoints<J>(sbeta + p, al, E, logE);
    double gd[SETS][OH_MAXD];                     // the dense columns of the g set and of the border sets
#pragma unroll
    for (int k = 0; k < SETS; ++k) {
#pragma unroll
        for (int c = 0; c < OH_MAXD; ++c) gd[k][c] = 0.0;
    }
    double sc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) sc[i] = 0.0;
    double ll = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounds = (a.n - (int64_t)blockIdx.x * blockDim.x + stride - 1) / stride;
    const int mywave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + rd * stride;
        const bool valid = i0 < a.n;
        const int64_t i = valid ? i0 : a.n - 1;
        double d[OH_MAXD];
        oh_dense_row(ds, a.num, a.ldn, i, d);
        double eta = 0.0;
#pragma unroll
        for (int c = 0; c < OH_MAXD; ++c)
            if (c < ds.D) eta = fma(d[c], sbeta[ds.dense_col[c]], eta);
        int cols[OH_MAXF];
#pragma unroll
        for (int t = 0; t < OH_MAXF; ++t) {
            cols[t] = -1;
            if (t < ds.f) {
                const int code = a.codes[i * a.ldc + t];
                const int nl = ds.lvl_off[t + 1] - ds.lvl_off[t];
                if (code >= 0 && code < nl) cols[t] = scol[ds.lvl_off[t] + code];      // an unknown / baseline level contributes nothing
                if (cols[t] >= 0) eta += sbeta[cols[t]];
            }
        }
        const double yv = a.y[i];
        double llt, resid, aa, bb, su, sl, q;
        ord_row_terms<J>(yv, eta, al, E, logE, llt, resid, aa, bb, su, sl, q);
        if (valid) {
            if (a.w_out) a.w_out[i] = aa + bb;
            if (a.aa_out) { a.aa_out[i] = aa; a.bb_out[i] = bb; }
            ll += llt;
        }
        const double r = valid ? resid : 0.0;
        int cls = 0;                               // 0 .. J: bounded whatever y holds
        bool isclass = yv == 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            ord_cutpoint_sums<J>(j, yv, valid, su, sl, aa, bb, q, sc);
            cls += yv == (double)(j + 1) ? j + 1 : 0;
            isclass = isclass || yv == (double)(j + 1);
        }
#pragma unroll
        for (int c = 0; c < OH_MAXD; ++c) gd[0][c] = fma(r, d[c], gd[0][c]);
        if constexpr (BORDER) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double vj = -((valid && yv == (double)j ? aa : 0.0) + (valid && yv == (double)(j + 1) ? bb : 0.0));
#pragma unroll
                for (int c = 0; c < OH_MAXD; ++c) gd[1 + j][c] = fma(vj, d[c], gd[1 + j][c]);
            }
        }
        // border set 1 + j holds X'v_{j+1}: class c feeds set c + 1 with -A Abar (c < J) and set c with -B Bbar (c >= 1)
        const bool has_up = BORDER && isclass && cls < J, has_lo = BORDER && cls >= 1;
        double* sg_up = sg_mine + (has_up ? cls + 1 : 0) * p;
        double* sg_lo = sg_mine + (has_lo ? cls : 0) * p;
        auto level_adds = [&]() {
#pragma unroll
            for (int t = 0; t < OH_MAXF; ++t) {
                if (t < ds.f && cols[t] >= 0) {
                    unsafeAtomicAdd(&sg_mine[cols[t]], r);
                    if constexpr (BORDER) {
                        if (has_up) unsafeAtomicAdd(&sg_up[cols[t]], -aa);
                        if (has_lo) unsafeAtomicAdd(&sg_lo[cols[t]], -bb);
                    }
                }
            }
        };
        if (ds.ordered) {                           // one wave at a time, in wave order: a fixed order of the LDS adds
            for (int turn = 0; turn < nwaves; ++turn) {
                if (turn == mywave && valid) level_adds();
                __syncthreads();
            }
        } else if (valid) {
            level_adds();
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SETS; ++k) {
#pragma unroll
        for (int c = 0; c < OH_MAXD; ++c) {
            if (c < ds.D) {                         // (uniform: every thread meets the same barriers)
                const double sgd = oh_block_sum(gd[k][c], red);
                if (threadIdx.x == 0) sg[k * p + ds.dense_col[c]] += sgd;
            }
        }
    }
    // the block's row of scalars in the layout of ordinal_internal.h: [g_alpha | diagonal | off-diagonal], 7 slots each
    double* scrow = a.scpart + (int64_t)blockIdx.x * ORD_SC;
    if (threadIdx.x < ORD_SC) {                     // the slots no sum goes to
        bool used = false;
#pragma unroll
        for (int i = 0; i < NS; ++i) used = used || ord_sc_slot<J>(i) == (int)threadIdx.x;
        if (!used) scrow[threadIdx.x] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double s = oh_block_sum(sc[i], red);
        if (threadIdx.x == 0) scrow[ord_sc_slot<J>(i)] = s;
    }
    const double sll = oh_block_sum(ll, red);
    __syncthreads();
    double* gp = a.gpart + (int64_t)blockIdx.x * cells;
    for (int c = threadIdx.x; c < cells; c += blockDim.x) {
        double t = sg[c];
        for (int rp = 1; rp < nrep; ++rp) t += sg[rp * cells + c];   // fixed order
        gp[c] = t;
    }
    if (threadIdx.x == 0) a.llpart[blockIdx.x] = ordered ? sll : NAN;
}

// The row model of one structured X'v through oh_row_kernel: mean keeps v[i], resid returns it, no weight, term 0.
struct OhXtvRow {
    static constexpr bool STORES_MU = false;
    const double* v;
    double vi;
    __device__ __forceinline__ double mean(int64_t i, double&) { vi = v[i]; return 0.0; }
    __device__ __forceinline__ double resid(double, double, double) const { return vi; }
    __device__ __forceinline__ double weight(double) const { return 0.0; }
    __device__ __forceinline__ double term(double, double, double) const { return 0.0; }
};

// ---- host side ---------------------------------------------------------------------------------------------------------
struct OhOrdLayout {
    size_t off_oh, oh_bytes, off_fin, off_sc, off_w, off_aa, off_bb, off_v, off_y, off_cpart, off_cst, off_state, total;
};

// the row pass's partials in the arena: [nb][cells], [nb] and [nb][ORD_SC]
static size_t oh_ord_pass_bytes(int p, int classes, int64_t n) {
    const int nb = oh_logit_blocks(n);
    const int cells = (oh_ord_border(p, classes) ? classes : 1) * p;
    return align_up((size_t)nb * cells * sizeof(double), 256) + align_up((size_t)nb * sizeof(double), 256) +
           align_up((size_t)nb * ORD_SC * sizeof(double), 256) + 256;
}

// off_oh: the arena of the structured passes (the row pass's partials, then the masked route's and the Gram's: the largest);
// fin: the finished [g_beta | J border vectors]; sc: the finished scalars; w, and on the masked route A Abar, B Bbar and v_j per
// row; row_step > 1: room for the gathered responses of a strided partition; then the Newton state on d coefficients
static OhOrdLayout oh_ord_layout(const dlsa_onehot_plan* pl, int64_t max_rows, int classes, int64_t row_step) {
    OhOrdLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    const int p = onehot_plan_p(pl), J = classes - 1;
    const bool border = oh_ord_border(p, classes);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.oh_bytes = align_up(std::max(onehot_workspace_bytes_impl(pl, n), oh_ord_pass_bytes(p, classes, n)), 256);
    l.off_oh = take(l.oh_bytes);
    l.off_fin = take(8 * (size_t)classes * p);
    l.off_sc = take(8 * ORD_SC);
    l.off_w = take(8 * (size_t)n);
    l.off_aa = take(border ? 0 : 8 * (size_t)n);
    l.off_bb = take(border ? 0 : 8 * (size_t)n);
    l.off_v = take(border ? 0 : 8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_cpart = take(8 * (size_t)MN_NQ * MN_CHECK_BLOCKS);
    l.off_cst = take(8 * 16);
    l.off_state = take(newton_state_bytes(J + p));
    l.total = o;
    return l;
}

template <int J>
static void oh_ord_launch(const OhDesc& ds, const dlsa_onehot_plan* pl, const OhOrdArgs& a, bool border, int nb, size_t shm,
                          hipStream_t s) {
    if (border) hipLaunchKernelGGL((oh_ord_row_kernel<J, true>), dim3(nb), dim3(OH_THREADS), shm, s, ds, (const int32_t*)pl->d_level_col, a);
    else hipLaunchKernelGGL((oh_ord_row_kernel<J, false>), dim3(nb), dim3(OH_THREADS), shm, s, ds, (const int32_t*)pl->d_level_col, a);
}

// One partition at a fixed theta.  H (nullable; d x d, pitch ldh), g, loglik, w_out nullable.  Never synchronises the stream.
static int oh_ord_pass_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y,
                            const double* theta, int classes, int64_t n, double* H, int64_t ldh, double* g, double* loglik,
                            double* w_out, char* ws, const OhOrdLayout& l, hipStream_t s) {
    const int J = classes - 1;
    OhDesc ds = pl->desc;
    { const char* e = kernel_knob("DLSA_OH_ORDERED"); ds.ordered = e ? (atoi(e) != 0) : 1; }      // wave turn-taking unless 0
    ds.overflow = nullptr;
    const int p = ds.p;
    const bool border = H && oh_ord_border(p, classes);
    const bool masked = H && !border;
    const int cells = (border ? classes : 1) * p;
    const int nb = oh_logit_blocks(n);
    void* ws_oh = ws + l.off_oh;
    Arena ar(ws_oh, l.oh_bytes);
    OhOrdArgs a{};
    a.num = num; a.codes = codes; a.y = y; a.theta = theta; a.ldn = ldn; a.ldc = ldc; a.n = n;
    a.w_out = w_out ? w_out : (H ? (double*)(ws + l.off_w) : nullptr);
    a.aa_out = masked ? (double*)(ws + l.off_aa) : nullptr;
    a.bb_out = masked ? (double*)(ws + l.off_bb) : nullptr;
    a.gpart = (double*)ar.take((size_t)nb * cells * sizeof(double));
    a.llpart = (double*)ar.take((size_t)nb * sizeof(double));
    a.scpart = (double*)ar.take((size_t)nb * ORD_SC * sizeof(double));
    if (!a.gpart || !a.llpart || !a.scpart) {
        set_error("onehot ordinal pass: the pass arena of %zu bytes is too small", l.oh_bytes);
        return DLSA_ERR_WORKSPACE;
    }
    a.nrep = oh_ord_rep(p, J, cells);
    const size_t shm = (size_t)(p + J + a.nrep * cells + 16) * sizeof(double) + (size_t)((ds.nlev_total + 1) & ~1) * sizeof(int);
    switch (J) {
        case 1: oh_ord_launch<1>(ds, pl, a, border, nb, shm, s); break;
        case 2: oh_ord_launch<2>(ds, pl, a, border, nb, shm, s); break;
        case 3: oh_ord_launch<3>(ds, pl, a, border, nb, shm, s); break;
        case 4: oh_ord_launch<4>(ds, pl, a, border, nb, shm, s); break;
        case 5: oh_ord_launch<5>(ds, pl, a, border, nb, shm, s); break;
        case 6: oh_ord_launch<6>(ds, pl, a, border, nb, shm, s); break;
        case 7: oh_ord_launch<7>(ds, pl, a, border, nb, shm, s); break;
        default:
            set_error("onehot ordinal pass: no row kernel for %d classes", classes);
            return DLSA_ERR_INVALID;
    }
    DLSA_HIP_CHECK(hipGetLastError());
    double* fin = (double*)(ws + l.off_fin);      // [g_beta (p) | border vector 1 .. J (p each)]
    double* bd = fin + p;
    double* sc = (double*)(ws + l.off_sc);
    const bool sums = g || H;
    if (sums || loglik) {
        logit_finish_launch(a.gpart, a.llpart, nb, cells, cells, sums ? fin : nullptr, loglik, s, nullptr, nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    if (!sums) return DLSA_OK;
    logit_finish_launch(a.scpart, nullptr, nb, ORD_SC, ORD_SC, sc, nullptr, s, nullptr, nullptr);
    DLSA_HIP_CHECK(hipGetLastError());
    // (the masked route's and the Gram's partials overwrite the pass's in the same arena: the finish launches above have consumed
    //  them, in stream order)
    if (masked) {
        double* v = (double*)(ws + l.off_v);
        for (int j = 1; j <= J; ++j) {
            int rc = ord_mask(y, a.aa_out, a.bb_out, j, n, v, s);
            if (rc) return rc;
            rc = oh_row_pass("onehot ordinal border pass", OhXtvRow{v, 0.0}, pl, num, ldn, codes, ldc, v, theta + J, n, nullptr, nullptr,
                             bd + (size_t)(j - 1) * p, nullptr, ws_oh, l.oh_bytes, s);
            if (rc) return rc;
        }
    }
    if (H) {
        const int rc = onehot_gram_impl(pl, num, ldn, codes, ldc, a.w_out, n, H + (size_t)J * ldh + J, ldh, ws_oh, l.oh_bytes, s, false);
        if (rc) return rc;
    }
    return ord_assemble(sc, bd, p, J, p, H, ldh, g, fin, s);
}

// what both entries refuse about the plan, the rows and the shape; `who` prefixes the message
static int oh_ord_args_ok(const char* who, const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                          int classes) {
    DLSA_REQUIRE(oh_pois_icpt_col(pl) < 0,
                 "%s: the plan has a constant column (column %d); the cutpoints are the intercepts of an ordinal model, so the plan "
                 "must have none", who, oh_pois_icpt_col(pl));
    const int rc = oh_pois_check_rows(who, pl, num, ldn, codes, ldc);
    if (rc) return rc;
    DLSA_REQUIRE(classes >= 2 && classes <= ORD_MAX_CLASSES, "%s: classes must lie in 2 .. %d, got %d", who, ORD_MAX_CLASSES, classes);
    const int64_t d = (int64_t)(classes - 1) + onehot_plan_p(pl);
    DLSA_REQUIRE(d <= 2048, "%s: d = (classes - 1) + p = %lld coefficients exceed the solver's 2048", who, (long long)d);
    return DLSA_OK;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_onehot_ordinal_workspace_bytes(const dlsa_onehot_plan* plan, int64_t max_rows, int classes, int64_t row_step) {
    if (!plan || classes < 2 || classes > dlsa::ORD_MAX_CLASSES || max_rows < 0 || row_step < 1) return 0;
    if (dlsa::oh_pois_icpt_col(plan) >= 0) return 0;
    if ((int64_t)(classes - 1) + dlsa::onehot_plan_p(plan) > 2048) return 0;
    return dlsa::oh_ord_layout(plan, max_rows, classes, row_step).total;
}

int dlsa_onehot_ordinal_pass_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                 const double* y, const double* theta, int classes, int64_t n, double* H, int64_t ldh, double* g,
                                 double* loglik, double* w_out, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && theta, "onehot_ordinal_pass: null plan, y or theta");
    int rc = oh_ord_args_ok("onehot_ordinal_pass", plan, num, ldn, codes, ldc, classes);
    if (rc) return rc;
    const int p = onehot_plan_p(plan), d = classes - 1 + p;
    DLSA_REQUIRE(n >= 1 && (!H || ldh >= d), "onehot_ordinal_pass: bad shape n=%lld p=%d ldh=%lld", (long long)n, p, (long long)ldh);
    const OhOrdLayout l = oh_ord_layout(plan, n, classes, 1);
    rc = newton_check_ws("onehot_ordinal_pass", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    rc = oh_ord_pass_impl(plan, num, ldn, codes, ldc, y, theta, classes, n, H, ldh, g, loglik, w_out, wsc, l, s);
    if (rc || !loglik) return rc;
    rc = mn_check(y, n, classes, (double*)(wsc + l.off_cpart), (double*)(wsc + l.off_cst), s);
    if (rc) return rc;
    return mn_ll_fix(loglik, (const double*)(wsc + l.off_cst), s);
}

int dlsa_onehot_ordinal_fit_f64(const dlsa_onehot_plan* plan, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                                const double* y, const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step, int K,
                                int classes, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                                int* n_iter_host, int* status_host, double* loglik_host, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(plan && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef,
                 "onehot_ordinal_fit: null argument (plan, y, the partitions, coef, Sig_inv and Sig_invMcoef are required)");
    int rc = oh_ord_args_ok("onehot_ordinal_fit", plan, num, ldn, codes, ldc, classes);
    if (rc) return rc;
    const int p = onehot_plan_p(plan), d = classes - 1 + p;
    DLSA_REQUIRE(K > 0 && row_step >= 1, "onehot_ordinal_fit: bad shape K=%d step=%lld", K, (long long)row_step);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "onehot_ordinal_fit: bad tol/max_iter");
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "onehot_ordinal_fit: negative partition shape (partition %d)", k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    const OhOrdLayout l = oh_ord_layout(plan, max_rows, classes, row_step);
    rc = newton_check_ws("onehot_ordinal_fit", ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    MnFitBufs b{};
    b.cpart = (double*)(wsc + l.off_cpart); b.cst = (double*)(wsc + l.off_cst);
    b.ybuf = (double*)(wsc + l.off_y);
    b.st = newton_state_at(wsc + l.off_state, d);
    const int64_t pn = ldn * row_step, pc = ldc * row_step;   // rows first, first + step, ...: strided views, num / codes read in place
    auto eval = [=](int k, const double* yk, int64_t nk, const double* theta, double* Hk, double* g, double* ll) {
        const double* numk = num ? num + part_first_host[k] * ldn : nullptr;
        const int32_t* codesk = codes ? codes + part_first_host[k] * ldc : nullptr;
        return oh_ord_pass_impl(plan, numk, pn, codesk, pc, yk, theta, classes, nk, Hk, d, g, ll, nullptr, wsc, l, s);
    };
    return mn_fit_core("onehot_ordinal_fit", ORD_NO_CLASS, y, part_first_host, part_rows_host, row_step, K, d, classes, tol, max_iter, coef, Sig_inv,
                       Sig_invMcoef, n_iter_host, status_host, loglik_host, b, ord_null_start(classes - 1, d), eval, s);
}

}  // extern "C"
