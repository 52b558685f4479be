// The row pass of the structured one-hot models (logistic: onehot.hip, Poisson: onehot_poisson.hip, NB2: onehot_negbin.hip): one
// kernel and its launch driver, as templates on the ROW MODEL M -- a struct of the model's per-row inputs (and what it keeps of
// the row in hand) with
//   static constexpr bool STORES_MU   the pass also writes mu per row (mu_out, nullable) next to the Gram's weight
//   double mean(i, eta)          row i's offset added to eta (if the model has one); returns mu
//   double resid(y, eta, mu)     the row's residual, the multiplier of its columns in g (y - mu, or the model's own)
//   double weight(mu)            the Gram's weight of the row (computed only where it is stored)
//   double term(y, eta, mu)      the row's log-likelihood term (computed only for rows below n)
// called in this order on a copy of the model per row.
// The model is a compile-time type: an instantiation holds its own terms only, and nothing here asks which model it serves.
// Included inside namespace dlsa after onehot_plan.h; the library is built without relocatable device code, so the kernel is
// instantiated in the file that launches it.

// One thread per row: eta = d . beta_D + sum_t beta[col(t, code_t)] is a gather, r = the model's residual; per-workgroup partials
// of g (dense part in registers, level part an LDS histogram) and of the log-likelihood terms; w per row to w_out (nullable), mu
// per row to mu_out (nullable; M::STORES_MU only).
template <class M>
__global__ __launch_bounds__(OH_THREADS) void oh_row_kernel(OhDesc ds, const int32_t* __restrict__ level_col,
                                                            const double* __restrict__ num, int64_t ldn,
                                                            const int32_t* __restrict__ codes, int64_t ldc,
                                                            const double* __restrict__ y, const double* __restrict__ beta,
                                                            int64_t n, double* __restrict__ w_out, double* __restrict__ mu_out,
                                                            double* __restrict__ gpart, double* __restrict__ llpart, int nrep, M m) {
    extern __shared__ double sm[];
    double* sbeta = sm;                           // p
    double* sg = sm + ds.p;                       // nrep x p (histograms of residuals; lanes spread over the copies,
                                                  // so the lanes of a wave that share a hot level do not serialise on one address)
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
    // every thread runs the same number of rounds (the ordered mode has barriers inside): rows past n are clamped and masked
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
        M row = m;                                  // the model's inputs and this row's own state
        const double mu = row.mean(i, eta);
        const double rs = row.resid(yv, eta, mu);
        if (w_out && valid) w_out[i] = row.weight(mu);
        if constexpr (M::STORES_MU) { if (mu_out && valid) mu_out[i] = mu; }
        const double r = valid ? rs : 0.0;
        if (valid) ll += row.term(yv, eta, mu);
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

// One partition at a fixed beta: w and (M::STORES_MU) mu per row (nullable), g and loglik (the sum of the model's terms;
// nullable) through the fixed-order column sums of the per-workgroup partials.  ws: the structured passes' arena (256-aligned, at least
// onehot_workspace_bytes_impl(pl, n)); `who` prefixes the message.
template <class M>
static int oh_row_pass(const char* who, const M& m, const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes,
                       int64_t ldc, const double* y, const double* beta, int64_t n, double* w_out, double* mu_out, double* g,
                       double* loglik, void* ws, size_t ws_bytes, hipStream_t s) {
    OhDesc ds = pl->desc;
    { const char* e = kernel_knob("DLSA_OH_ORDERED"); ds.ordered = e ? (atoi(e) != 0) : 1; }      // wave turn-taking unless 0
    ds.overflow = nullptr;
    const int nb = oh_logit_blocks(n);
    Arena ar(ws, ws_bytes);
    double* gpart = (double*)ar.take((size_t)nb * ds.p * sizeof(double));
    double* llpart = (double*)ar.take((size_t)nb * sizeof(double));
    if (!gpart || !llpart) {
        set_error("%s: the pass arena of %zu bytes is too small", who, ws_bytes);
        return DLSA_ERR_WORKSPACE;
    }
    const int nrep = oh_logit_rep(ds.p);
    const size_t shm = (size_t)((1 + nrep) * ds.p + 16) * sizeof(double) + (size_t)((ds.nlev_total + 1) & ~1) * sizeof(int);
    hipLaunchKernelGGL(oh_row_kernel<M>, dim3(nb), dim3(OH_THREADS), shm, s, ds, (const int32_t*)pl->d_level_col, num, ldn, codes,
                       ldc, y, beta, n, w_out, mu_out, gpart, llpart, nrep, m);
    DLSA_HIP_CHECK(hipGetLastError());
    if (g || loglik) {
        logit_finish_launch((const double*)gpart, (const double*)llpart, nb, ds.p, ds.p, g, loglik, s, nullptr, nullptr);
        DLSA_HIP_CHECK(hipGetLastError());
    }
    return DLSA_OK;
}
