// The dense row pass of the count models with a log link (Poisson: poisson.hip, NB2: negbin.hip): one kernel, its launch
// ladder and the pass driver, as templates on the ROW MODEL M -- a struct of the model's parameters with
//   static constexpr bool STORES_MU    the pass also writes mu per row (a.mu_out) next to the Gram's weight
//   void terms(y, eta, mu, wgt, rs, llt)   the Gram weight, the unmasked residual and the log-likelihood term of one row
// The model is a compile-time type: an instantiation holds its own terms only, and nothing here asks which model it serves.
// Included inside namespace dlsa after rowdot.h (merged_reduce, row_of_lane, rep_mask, rank1_update) and poisson_exp.h
// (exp_full), with poisson_internal.h above it; the library is built without relocatable device code, so the kernel is
// instantiated in the file that launches it.
#include "row_pass.h"     // the batch load, the batch loop, the block reduction, the shapes and the dispatcher

template <class M>
struct CountArgs {
    const double* X;
    const double* y;
    const double* off;     // nullable (OFF = false)
    const double* beta;    // the p coefficients of X's columns
    const double* beta0;   // the intercept's coefficient (nullable: no intercept)
    double* w_out;         // the Gram's weight per row (nullable)
    double* mu_out;        // mu per row (nullable; M::STORES_MU only)
    double* gpart;         // [nblocks][NC*128]
    double* llpart;        // [nblocks]: sum of the log-likelihood terms
    double* s0part;        // [nblocks]: sum of the residuals (the intercept's entry of g)
    double* hpart;         // BORDER: [nblocks][NC*128] X'w
    double* swpart;        // BORDER: [nblocks] sum w
    int64_t ldx;
    int64_t n;
    int p;
    M m;
};

struct CountRowIn { double y, off; };      // the lane's own row's count and offset: they travel with the batch

// The skeleton of row_pass.h with the model's terms.  Accumulator sets: g, then (BORDER) h = X'w; scalars: ll, s0, then sw.
template <class M, int NC, int RB, bool VEC, bool OFF, bool BORDER>
__global__ __launch_bounds__(COUNT_THREADS) void count_pass_kernel(CountArgs<M> a) {
    constexpr int SETS = BORDER ? 2 : 1, W = NC * 128;
    __shared__ double red[SETS * W + 2 + (BORDER ? 1 : 0)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const double b0 = a.beta0 ? *a.beta0 : 0.0;
    const M m = a.m;
    double s0 = 0.0, sw = 0.0, ll = 0.0;
    double2 b[NC], g[SETS][NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 128 + 2 * lane;
        b[c].x = col < a.p ? a.beta[col] : 0.0;
        b[c].y = col + 1 < a.p ? a.beta[col + 1] : 0.0;
#pragma unroll
        for (int k = 0; k < SETS; ++k) { g[k][c].x = 0.0; g[k][c].y = 0.0; }
    }
    const int myrow = row_of_lane<RB>(lane);
    const bool rep = (lane & rep_mask<RB>()) == 0;

    auto load_batch = [&](int64_t bt, double2 (&x)[RB][NC], CountRowIn& in) {
        const int64_t ry = row_pass_load<NC, RB, VEC>(a.X, a.ldx, a.n, a.p, bt, lane, myrow, x);
        in.y = a.y[ry];
        in.off = OFF ? a.off[ry] : 0.0;
    };
    auto process = [&](int64_t bt, const double2 (&x)[RB][NC], const CountRowIn& in) {
        const int64_t row0 = bt * RB;
        double dot[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) s = fma(x[i][c].x, b[c].x, fma(x[i][c].y, b[c].y, s));
            dot[i] = s;
        }
        const int64_t r = row0 + myrow;
        const bool valid = r < a.n;
        const double yv = valid ? in.y : 0.0;
        const double eta = merged_reduce<RB>(dot, lane) + b0 + (OFF ? in.off : 0.0);
        const double mu = exp_full(eta);
        double wgt, rs, llt;
        m.terms(yv, eta, mu, wgt, rs, llt);
        const double resid = valid ? rs : 0.0;
        if (valid && rep) {
            if (a.w_out) a.w_out[r] = wgt;
            if constexpr (M::STORES_MU) { if (a.mu_out) a.mu_out[r] = mu; }
            ll += llt;
            s0 += resid;
        }
        rank1_update<RB, NC, 0>(resid, x, g[0]);
        if constexpr (BORDER) {                 // X'w and sum w of the same rows (a clamped row past n weighs nothing)
            const double wv = valid ? wgt : 0.0;
            if (rep) sw += wv;
            rank1_update<RB, NC, 0>(wv, x, g[1]);
        }
    };

    // The batch loop of row_pass_stream (row_pass.h), kept as this kernel's own text: on the shared template the NC = 1 instantiations
    // without BORDER take 2 VGPRs more (one 64-bit value moves out of the SGPRs), and <TweedieRow, 1, 8, true, true, false>
    // loses its fourth wave over them (130 VGPRs for 128).
    const int64_t nbatch = (a.n + RB - 1) / RB;
    const int64_t stride = (int64_t)gridDim.x * COUNT_WAVES;
    int64_t bt = (int64_t)blockIdx.x * COUNT_WAVES + wave;
    if constexpr (NC == 1) {
        double2 xa[RB][NC], xb[RB][NC];
        CountRowIn ia{}, ib{};
        if (a.n > 0) {
            load_batch(bt, xa, ia);
            for (; bt < nbatch; bt += 2 * stride) {
                const int64_t b1 = bt + stride, b2 = bt + 2 * stride;
                load_batch(b1, xb, ib);
                process(bt, xa, ia);
                load_batch(b2, xa, ia);
                if (b1 < nbatch) process(b1, xb, ib);
            }
        }
    } else {
        for (; bt < nbatch; bt += stride) {
            double2 x[RB][NC];
            CountRowIn in;
            load_batch(bt, x, in);
            process(bt, x, in);
        }
    }

    double sc[2 + (BORDER ? 1 : 0)];
    sc[0] = ll; sc[1] = s0;
    if constexpr (BORDER) sc[2] = sw;
    row_pass_reduce(g, sc, red, lane, wave);
    double* gp = a.gpart + (int64_t)blockIdx.x * W;
    for (int col = tid; col < W; col += COUNT_THREADS) gp[col] = red[col];
    if (tid == 0) { a.llpart[blockIdx.x] = red[SETS * W]; a.s0part[blockIdx.x] = red[SETS * W + 1]; }
    if constexpr (BORDER) {
        double* hp = a.hpart + (int64_t)blockIdx.x * W;
        for (int col = tid; col < W; col += COUNT_THREADS) hp[col] = red[W + col];
        if (tid == 0) a.swpart[blockIdx.x] = red[SETS * W + 2];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The pass's scratch: the per-block partials and the Hessian's border.  A workspace layout takes the six through
// count_scratch_take (one order, one alignment) and hands the pass the pointers of count_scratch_at.
template <class T>
struct CountScratchOf { T gpart, llpart, s0part, hpart, swpart, border; };
using CountScratchOff = CountScratchOf<size_t>;
using CountScratch = CountScratchOf<double*>;

template <class Take>
static CountScratchOff count_scratch_take(Take& take, int p) {
    const size_t gp = (size_t)COUNT_MAX_BLOCKS * count_nc(p) * 128 * sizeof(double);
    CountScratchOff o{};
    o.gpart = take(gp);
    o.llpart = take(8 * (size_t)COUNT_MAX_BLOCKS);
    o.s0part = take(8 * (size_t)COUNT_MAX_BLOCKS);
    o.hpart = take(gp);
    o.swpart = take(8 * (size_t)COUNT_MAX_BLOCKS);
    o.border = take(8 * (size_t)(p + 1));
    return o;
}

static CountScratch count_scratch_at(char* ws, const CountScratchOff& o) {
    return {(double*)(ws + o.gpart), (double*)(ws + o.llpart), (double*)(ws + o.s0part), (double*)(ws + o.hpart),
            (double*)(ws + o.swpart), (double*)(ws + o.border)};
}

template <class M, int NC, int RB, bool VEC, bool OFF>
static void count_launch_b(const CountArgs<M>& a, bool border, int blocks, hipStream_t s) {
    if (border) hipLaunchKernelGGL((count_pass_kernel<M, NC, RB, VEC, OFF, true>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
    else hipLaunchKernelGGL((count_pass_kernel<M, NC, RB, VEC, OFF, false>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
}
template <class M, int NC, int RB>
static void count_launch(const CountArgs<M>& a, bool vec, bool border, int blocks, hipStream_t s) {
    if (vec) {
        if (a.off) count_launch_b<M, NC, RB, true, true>(a, border, blocks, s);
        else count_launch_b<M, NC, RB, true, false>(a, border, blocks, s);
    } else {
        if (a.off) count_launch_b<M, NC, RB, false, true>(a, border, blocks, s);
        else count_launch_b<M, NC, RB, false, false>(a, border, blocks, s);
    }
}

// One partition at fixed coefficients beta (pe = p + intercept entries, intercept first) and model parameters m.  H (nullable)
// needs w (the Gram's weights); g, loglik (the sum of the model's log-likelihood terms, without its beta-free part), w, mu
// nullable otherwise.  gws: the Gram's workspace.
template <class M>
static int count_pass(const M& m, const double* X, int64_t ldx, const double* y, const double* off, const double* beta, int64_t n,
                      int p, int intercept, double* H, int64_t ldh, double* g, double* loglik, double* w, double* mu,
                      const CountScratch& sc, void* gws, size_t gws_bytes, hipStream_t s) {
    const int nc = count_nc(p), rb = count_rb(nc);
    const bool border = H && intercept;
    CountArgs<M> a{};
    a.X = X; a.y = y; a.off = off; a.beta = intercept ? beta + 1 : beta; a.beta0 = intercept ? beta : nullptr;
    a.w_out = w; a.mu_out = mu; a.ldx = ldx; a.n = n; a.p = p; a.m = m;
    a.gpart = sc.gpart; a.llpart = sc.llpart; a.s0part = sc.s0part; a.hpart = sc.hpart; a.swpart = sc.swpart;
    const bool vec = row_pass_vec(X, ldx, p);
    const int blocks = count_blocks(n, rb);
    row_pass_dispatch(nc, [&](auto sh) { count_launch<M, decltype(sh)::NC, decltype(sh)::RB>(a, vec, border, blocks, s); });
    DLSA_HIP_CHECK(hipGetLastError());
    if (g || loglik) {
        logit_finish_launch(a.gpart, a.llpart, blocks, nc * 128, p, (g && intercept) ? g + 1 : g, loglik, s,
                            (g && intercept) ? a.s0part : nullptr, (g && intercept) ? g : nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    if (!H) return DLSA_OK;
    if (!intercept) return gram_impl_f64(X, ldx, w, n, p, H, ldh, 0, gws, gws_bytes, s);
    double* bd = sc.border;                             // [sum w | X'w]: row 0 of [1 | X]' diag(w) [1 | X]
    logit_finish_launch(a.hpart, a.swpart, blocks, nc * 128, p, bd + 1, bd, s, nullptr, nullptr);
    DLSA_HIP_CHECK(hipGetLastError());
    return gram_icpt_impl(X, ldx, w, n, p, H, ldh, gws, gws_bytes, s, bd);
}
