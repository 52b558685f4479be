// The dense row pass of the count models with a log link (Poisson: poisson.hip, NB2: negbin.hip): one kernel, its launch
// ladder and the pass driver, as templates on the ROW MODEL M -- a struct of the model's parameters with
//   static constexpr bool STORES_MU    the pass also writes mu per row (a.mu_out) next to the Gram's weight
//   void terms(y, eta, mu, wgt, rs, llt)   the Gram weight, the unmasked residual and the log-likelihood term of one row
// The model is a compile-time type: an instantiation holds its own terms only, and nothing here asks which model it serves.
// Included inside namespace dlsa after rowdot.h (merged_reduce, row_of_lane, rep_mask, rank1_update) and poisson_exp.h
// (exp_full), with poisson_internal.h above it; the library is built without relocatable device code, so the kernel is
// instantiated in the file that launches it.

typedef double count_d2v __attribute__((ext_vector_type(2)));

constexpr int COUNT_THREADS = 256;
constexpr int COUNT_WAVES = COUNT_THREADS / 64;
constexpr int COUNT_MAX_BLOCKS = 2048;

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

static __device__ __forceinline__ double2 count_ld2(const double* ptr) {
    const count_d2v t = __builtin_nontemporal_load(reinterpret_cast<const count_d2v*>(ptr));
    double2 r; r.x = t.x; r.y = t.y; return r;
}

// The logit pass's skeleton (logit.hip logit_kernel) with the model's terms: branch-free clamped loads, the lane's own row's
// count and offset travel with the batch, a second register set prefetches the next batch at NC = 1.
template <class M, int NC, int RB, bool VEC, bool OFF, bool BORDER>
__global__ __launch_bounds__(COUNT_THREADS) void count_pass_kernel(CountArgs<M> a) {
    __shared__ double red[NC * 128 + 2];
    __shared__ double redh[BORDER ? NC * 128 + 1 : 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const double b0 = a.beta0 ? *a.beta0 : 0.0;
    const M m = a.m;
    double s0 = 0.0, sw = 0.0, ll = 0.0;
    double2 b[NC], g[NC], h[BORDER ? NC : 1];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 128 + 2 * lane;
        b[c].x = col < a.p ? a.beta[col] : 0.0;
        b[c].y = col + 1 < a.p ? a.beta[col + 1] : 0.0;
        g[c].x = 0.0; g[c].y = 0.0;
        if constexpr (BORDER) { h[c].x = 0.0; h[c].y = 0.0; }
    }
    const int myrow = row_of_lane<RB>(lane);
    const bool rep = (lane & rep_mask<RB>()) == 0;
    const int64_t nbatch = (a.n + RB - 1) / RB;
    const int64_t stride = (int64_t)gridDim.x * COUNT_WAVES;

    auto load_batch = [&](int64_t bt, double2 (&x)[RB][NC], double& yv, double& ov) {
        const int64_t row0 = bt * RB;
        const int64_t ry = min(row0 + myrow, a.n - 1);
        const double ytmp = a.y[ry];
        const double otmp = OFF ? a.off[ry] : 0.0;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int64_t r = min(row0 + i, a.n - 1);
            const double* rowp = a.X + r * a.ldx;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int col = c * 128 + 2 * lane;
                const int c0 = col < a.p ? col : 0;                   // clamped columns meet beta = 0
                if (VEC) {                                            // VEC implies p even: a pair never straddles p
                    x[i][c] = count_ld2(rowp + c0);
                } else {
                    x[i][c].x = __builtin_nontemporal_load(rowp + c0);
                    x[i][c].y = __builtin_nontemporal_load(rowp + (col + 1 < a.p ? col + 1 : 0));
                }
            }
        }
        yv = ytmp;
        ov = otmp;
    };
    auto process = [&](int64_t bt, const double2 (&x)[RB][NC], const double yraw, const double oraw) {
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
        const double yv = valid ? yraw : 0.0;
        const double eta = merged_reduce<RB>(dot, lane) + b0 + (OFF ? oraw : 0.0);
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
        rank1_update<RB, NC, 0>(resid, x, g);
        if constexpr (BORDER) {                 // X'w and sum w of the same rows (a clamped row past n weighs nothing)
            const double wv = valid ? wgt : 0.0;
            if (rep) sw += wv;
            rank1_update<RB, NC, 0>(wv, x, h);
        }
    };

    int64_t bt = (int64_t)blockIdx.x * COUNT_WAVES + wave;
    if constexpr (NC == 1) {
        double2 xa[RB][NC], xb[RB][NC];
        double ya = 0.0, yb = 0.0, oa = 0.0, ob = 0.0;
        if (a.n > 0) {
            load_batch(bt, xa, ya, oa);
            for (; bt < nbatch; bt += 2 * stride) {
                const int64_t b1 = bt + stride, b2 = bt + 2 * stride;
                load_batch(b1, xb, yb, ob);
                process(bt, xa, ya, oa);
                load_batch(b2, xa, ya, oa);
                if (b1 < nbatch) process(b1, xb, yb, ob);
            }
        }
    } else {
        for (; bt < nbatch; bt += stride) {
            double2 x[RB][NC];
            double yv, ov;
            load_batch(bt, x, yv, ov);
            process(bt, x, yv, ov);
        }
    }

    // block reduction: waves add into LDS one after another (fixed order)
    ll = wave_allreduce_sum(ll);
    s0 = wave_allreduce_sum(s0);
    if constexpr (BORDER) sw = wave_allreduce_sum(sw);
    for (int wv = 0; wv < COUNT_WAVES; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double* dst = red + c * 128 + 2 * lane;
                if (wv == 0) { dst[0] = g[c].x; dst[1] = g[c].y; }
                else { dst[0] += g[c].x; dst[1] += g[c].y; }
                if constexpr (BORDER) {
                    double* dh = redh + c * 128 + 2 * lane;
                    if (wv == 0) { dh[0] = h[c].x; dh[1] = h[c].y; }
                    else { dh[0] += h[c].x; dh[1] += h[c].y; }
                }
            }
            if (lane == 0) {
                if (wv == 0) { red[NC * 128] = ll; red[NC * 128 + 1] = s0; }
                else { red[NC * 128] += ll; red[NC * 128 + 1] += s0; }
                if constexpr (BORDER) { if (wv == 0) redh[NC * 128] = sw; else redh[NC * 128] += sw; }
            }
        }
        __syncthreads();
    }
    double* gp = a.gpart + (int64_t)blockIdx.x * (NC * 128);
    for (int col = tid; col < NC * 128; col += COUNT_THREADS) gp[col] = red[col];
    if (tid == 0) { a.llpart[blockIdx.x] = red[NC * 128]; a.s0part[blockIdx.x] = red[NC * 128 + 1]; }
    if constexpr (BORDER) {
        double* hp = a.hpart + (int64_t)blockIdx.x * (NC * 128);
        for (int col = tid; col < NC * 128; col += COUNT_THREADS) hp[col] = redh[col];
        if (tid == 0) a.swpart[blockIdx.x] = redh[NC * 128];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int count_nc(int p) {
    const int chunks = (p + 127) / 128;
    int nc = 1;
    while (nc < chunks) nc *= 2;
    return nc;
}

static int count_rb(int nc) { return nc <= 2 ? 8 : nc == 4 ? 4 : nc == 8 ? 2 : 1; }

static int count_blocks(int64_t n, int rb) {
    const int64_t nbatch = (n + rb - 1) / rb;
    int64_t blocks = (nbatch + COUNT_WAVES * 4 - 1) / (COUNT_WAVES * 4);   // >= 4 batches per wave
    return (int)std::min<int64_t>(std::max<int64_t>(blocks, 1), COUNT_MAX_BLOCKS);
}

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
    const bool vec = (ldx % 2 == 0) && (p % 2 == 0) && (((uintptr_t)X & 15) == 0);
    const int blocks = count_blocks(n, rb);
    switch (nc) {
        case 1: count_launch<M, 1, 8>(a, vec, border, blocks, s); break;
        case 2: count_launch<M, 2, 8>(a, vec, border, blocks, s); break;
        case 4: count_launch<M, 4, 4>(a, vec, border, blocks, s); break;
        case 8: count_launch<M, 8, 2>(a, vec, border, blocks, s); break;
        default: count_launch<M, 16, 1>(a, vec, border, blocks, s); break;
    }
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
