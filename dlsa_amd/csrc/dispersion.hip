// The driver of the log-link families with a scalar dispersion (dispersion_internal.h: Gamma and Tweedie, dense rows and the raw
// representation of a one-hot design): the H / g scaling, the pass entries' epilogue, the
// per-partition fit, the two workspace layouts and the bodies of the eight C entries.  What a family computes it brings as its
// record; what reads the rows comes as a callable from the unit that instantiates the row kernel.  The Newton iteration is
// newton_fit.h's with the policy of the Poisson fit, the gather of a strided partition's responses and offsets and the start
// launcher poisson_internal.h's.
#include "common.h"
#include "onehot_plan.h"
#include "poisson_internal.h"
#include "dispersion_internal.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

#include "rowdot.h"
#include "poisson_exp.h"
#include "count_pass.h"   // CountScratch, count_scratch_take, count_scratch_at (no kernel of it is instantiated here)

// H (pe x pe, pitch ldh) and g (pe) times nu; either may be null
__global__ void disp_scale_kernel(double* __restrict__ H, int64_t ldh, int pe, double* __restrict__ g, double nu) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (H && i < (int64_t)pe * pe) H[(i / pe) * ldh + i % pe] *= nu;
    if (g && i < pe) g[i] *= nu;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int disp_sum_blocks(int64_t n) { return (int)std::min<int64_t>(DISP_SUM_BLOCKS, std::max<int64_t>(1, (n + 255) / 256)); }

int disp_scale(double* H, int64_t ldh, int pe, double* g, double nu, hipStream_t s) {
    if (!H && !g) return DLSA_OK;
    const int64_t items = H ? (int64_t)pe * pe : pe;
    hipLaunchKernelGGL(disp_scale_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, H, ldh, pe, g, nu);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

// device scratch of a pass entry and of the fit loop
struct DispFitBufs {
    double* cpart;     // nc * DISP_SUM_BLOCKS
    double* cst;       // 4
    double* dpart;     // DISP_ND * DISP_SUM_BLOCKS
    double* dst;       // 4
    double* w;         // max_rows: the Gram's weights
    double* mu;        // max_rows: mu of the last evaluation, what the dispersion sums read
    double* ybuf;      // max_rows when row_step > 1: the gathered responses
    double* obuf;      // max_rows when row_step > 1 and offsets are given
    NewtonState st;
};

// "evaluate (H, g, the row sum of the family's term, mu) at beta and unit dispersion for partition k": yk / ok (nullable) are the
// partition's nk > 0 responses and offsets, contiguous (gathered when the partition is strided); H is pe x pe (ldh = pe, both
// triangles), g pe, ll one device double, mu nk
using DispEval = std::function<int(int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* H, double* g,
                                   double* ll, double* mu)>;

// One workspace, two orders of carving it: the dense entries' (the count pass's partials first, the Gram's workspace last) and the
// structured entries' (the arena of the structured passes first).  row_step > 1: room for the gathered responses and offsets of a
// strided partition.  total is what the queries return; the Newton state is the last region of both.
struct DispLayout {
    size_t off_cpart, off_cst, off_dpart, off_dst, off_w, off_mu, off_y, off_o, off_state, total;
    CountScratchOff sc;       // dense
    size_t off_gram;          // dense: the Gram's workspace, up to off_state
    size_t off_oh, oh_bytes;  // structured: the pass's partials, then the Gram's (onehot_workspace_bytes_impl sizes both)
};

template <class Take>
static void disp_take_sums(DispLayout& l, Take& take, int nc) {
    l.off_cpart = take(8 * (size_t)nc * DISP_SUM_BLOCKS);
    l.off_cst = take(8 * 4);
    l.off_dpart = take(8 * (size_t)DISP_ND * DISP_SUM_BLOCKS);
    l.off_dst = take(8 * 4);
}
template <class Take>
static void disp_take_rows(DispLayout& l, Take& take, int64_t n, int64_t row_step) {
    l.off_w = take(8 * (size_t)n);
    l.off_mu = take(8 * (size_t)n);
    l.off_y = take(row_step > 1 ? 8 * (size_t)n : 0);
    l.off_o = take(row_step > 1 ? 8 * (size_t)n : 0);
}

static DispLayout disp_layout(int nc, int64_t max_rows, int p, int pe, int64_t row_step) {
    DispLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.sc = count_scratch_take(take, p);
    disp_take_sums(l, take, nc);
    disp_take_rows(l, take, n, row_step);
    l.off_gram = take(gram_workspace_bytes_impl(n, p, 8));
    l.off_state = take(newton_state_bytes(pe));
    l.total = o;
    return l;
}

static DispLayout disp_onehot_layout(int nc, const dlsa_onehot_plan* pl, int64_t max_rows, int64_t row_step) {
    DispLayout l{};
    const int64_t n = std::max<int64_t>(max_rows, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    l.oh_bytes = align_up(onehot_workspace_bytes_impl(pl, n), 256);
    l.off_oh = take(l.oh_bytes);
    disp_take_rows(l, take, n, row_step);
    disp_take_sums(l, take, nc);
    l.off_state = take(newton_state_bytes(onehot_plan_p(pl)));
    l.total = o;
    return l;
}

static DispFitBufs disp_bufs_at(char* ws, const DispLayout& l, int pe) {
    DispFitBufs b{};
    b.cpart = (double*)(ws + l.off_cpart); b.cst = (double*)(ws + l.off_cst);
    b.dpart = (double*)(ws + l.off_dpart); b.dst = (double*)(ws + l.off_dst);
    b.w = (double*)(ws + l.off_w); b.mu = (double*)(ws + l.off_mu);
    b.ybuf = (double*)(ws + l.off_y); b.obuf = (double*)(ws + l.off_o);
    b.st = newton_state_at(ws + l.off_state, pe);
    return b;
}

// The epilogue of the pass entries, after the row pass at unit dispersion has left H, g, the row sum of the family's term in
// loglik and (stats_out wanted) mu: [P, Dev] into stats_out, H and g times nu = 1 / dispersion, loglik the family's
// log-likelihood at that dispersion (NaN when a row is not a valid response).  H, g, loglik, stats_out nullable.
static int disp_pass_finish(const DispFamily& f, const double* y, const double* off, const double* mu, int64_t n, int pe,
                            double dispersion, double* H, int64_t ldh, double* g, double* loglik, double* stats_out,
                            const DispFitBufs& b, hipStream_t s) {
    const double nu = 1.0 / dispersion;
    int rc = DLSA_OK;
    if (stats_out) {
        rc = f.disp_sums(f, y, mu, n, b.dpart, stats_out, s);
        if (rc) return rc;
    }
    if (nu != 1.0) {
        rc = disp_scale(H, ldh, pe, g, nu, s);
        if (rc) return rc;
    }
    if (!loglik) return DLSA_OK;
    rc = f.const_sums(f, y, off, n, b.cpart, b.cst, s);
    if (rc) return rc;
    return f.ll_fix(loglik, b.cst, nu, n, s);
}

// The per-partition driver (dispersion_internal.h: disp_fit_entry): `eval` is the only part that knows the representation of
// the design; the iteration is newton_fit_loop (newton_fit.h).  icpt_col: the entry of beta that is the intercept (-1: none).
static int disp_fit_core(const char* who, const DispFamily& f, const double* y, const double* offset, const int64_t* part_first_host,
                         const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double dispersion_fixed,
                         double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host,
                         int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host, double* deviance_host,
                         const DispFitBufs& b, const DispEval& eval, hipStream_t s) {
    const bool fixed = dispersion_fixed > 0;
    if (!fixed) {
        for (int k = 0; k < K; ++k) {
            if (part_rows_host[k] > 0 && part_rows_host[k] <= pe) {
                set_error("%s: partition %d has %lld rows for %d coefficients: the estimated dispersion has no degrees of freedom",
                          who, k, (long long)part_rows_host[k], pe);
                return DLSA_ERR_INVALID;
            }
        }
    }
    int overall = DLSA_OK;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_rows_host[k];
        double* Hk = Sig_inv + (size_t)k * pe * pe;
        double* ck = coef + (size_t)k * pe;
        double* sk = Sig_invMcoef + (size_t)k * pe;
        int st_k = DLSA_PART_EMPTY, iters = 0;
        double ll = 0.0, phi = 0.0, d[DISP_ND] = {0.0, 0.0};
        if (nk > 0) {
            const double *yk, *ok;
            int rc = pois_gather_rows(y, offset, part_first_host[k], row_step, nk, b.ybuf, b.obuf, yk, ok, s);
            if (rc) return rc;
            rc = f.const_sums(f, yk, ok, nk, b.cpart, b.cst, s);
            if (rc) return rc;
            double cst[4];
            DLSA_HIP_CHECK(hipMemcpyAsync(cst, b.cst, 8 * (size_t)f.nc, hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            rc = f.check(who, k, cst);
            if (rc) return rc;
            // the intercept starts at the log of the intercept-only model's mean, that model's exact MLE
            const double m0 = f.start_mean(cst, nk);
            const double b0 = (icpt_col >= 0 && m0 > 0.0 && isfinite(m0)) ? log(m0) : 0.0;
            rc = pois_start(b.st.beta, pe, icpt_col, b0, s);
            if (rc) return rc;
            const NewtonDevice dev{b.st, Hk, pe, s};
            NewtonOutcome o;
            rc = newton_fit_loop(NEWTON_POISSON, tol, max_iter + 1,
                                 [&](bool&) { return eval(k, yk, ok, nk, b.st.beta, Hk, b.st.g, b.st.stats + 3, b.mu); }, dev,
                                 newton_no_hook, o);
            if (rc) return rc;
            st_k = o.status; iters = o.n_iter;
            // the dispersion of the point H was evaluated at: b.mu is that evaluation's
            rc = f.disp_sums(f, yk, b.mu, nk, b.dpart, b.dst, s);
            if (rc) return rc;
            DLSA_HIP_CHECK(hipMemcpyAsync(d, b.dst, sizeof(d), hipMemcpyDeviceToHost, s));
            DLSA_HIP_CHECK(hipStreamSynchronize(s));
            phi = fixed ? dispersion_fixed : d[DISP_PEARSON] / (double)(nk - pe);
            ll = o.ll;
            if (phi > 0.0 && isfinite(phi)) {              // (else: Sig_inv and loglik stay those of unit dispersion)
                const double nu = 1.0 / phi;
                rc = disp_scale(Hk, pe, pe, nullptr, nu, s);
                if (rc) return rc;
                ll = f.loglik(nu, o.ll, cst, nk);
            }
        }
        const int rcf = newton_fit_finish(st_k, iters, ll, b.st.beta, pe, Hk, ck, sk, k, n_iter_host, status_host, loglik_host, overall, s);
        if (rcf) return rcf;
        if (dispersion_host) dispersion_host[k] = phi;
        if (pearson_host) pearson_host[k] = d[DISP_PEARSON];
        if (deviance_host) deviance_host[k] = d[DISP_DEV];
    }
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    return overall;
}

// what the two fit entries check after their shapes, in the order the refusals fire; max_rows = the longest partition
static int disp_fit_args(const char* who, const DispFamily& f, double dispersion_fixed, double tol, int max_iter,
                         const int64_t* part_first_host, const int64_t* part_rows_host, int K, int64_t& max_rows) {
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "%s: bad tol/max_iter", who);
    DLSA_REQUIRE(!f.bad_param, "%s: %s", who, f.bad_param);
    DLSA_REQUIRE(!(dispersion_fixed > 0) || isfinite(dispersion_fixed), "%s: a fixed dispersion must be finite", who);
    max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_rows_host[k] >= 0 && part_first_host[k] >= 0, "%s: negative partition shape (partition %d)", who, k);
        max_rows = std::max(max_rows, part_rows_host[k]);
    }
    return DLSA_OK;
}

// ---- the dense entries ---------------------------------------------------------------------------------------------------
size_t disp_workspace_bytes(int nc, int64_t max_rows, int p, int intercept, int64_t row_step) {
    const int pe = p + (intercept ? 1 : 0);
    if (p <= 0 || pe > 2048 || max_rows < 0 || row_step < 1) return 0;
    return disp_layout(nc, max_rows, p, pe, row_step).total;
}

int disp_pass_entry(const char* who, const DispFamily& f, const DispDenseRows& rows, const double* X, int64_t ldx, const double* y,
                    const double* offset, const double* beta, double dispersion, int64_t n, int p, int intercept, double* H, int64_t ldh,
                    double* g, double* loglik, double* w_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    DLSA_REQUIRE(X && y && beta, "%s: null X, y or beta", who);
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(n >= 1 && p > 0 && pe <= 2048 && ldx >= p && (!H || ldh >= pe), "%s: bad shape n=%lld p=%d ldx=%lld ldh=%lld", who,
                 (long long)n, p, (long long)ldx, (long long)ldh);
    DLSA_REQUIRE(!f.bad_param, "%s: %s", who, f.bad_param);
    DLSA_REQUIRE(dispersion > 0 && isfinite(dispersion), "%s: the dispersion must be positive and finite", who);
    const DispLayout l = disp_layout(f.nc, n, p, pe, 1);
    // (the pass carves up to off_state of it; the contract is the query, which also holds a fit's Newton state)
    int rc = newton_check_ws(who, ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    const DispFitBufs b = disp_bufs_at(wsc, l, pe);
    double* w = w_out ? w_out : (H ? b.w : nullptr);
    double* mu = stats_out ? b.mu : nullptr;
    rc = rows(X, ldx, y, offset, beta, n, p, intercept, H, ldh, g, loglik, w, mu, count_scratch_at(wsc, l.sc), wsc + l.off_gram,
              l.off_state - l.off_gram, s);
    if (rc) return rc;
    return disp_pass_finish(f, y, offset, mu, n, pe, dispersion, H, ldh, g, loglik, stats_out, b, s);
}

int disp_fit_entry(const char* who, const DispFamily& f, const DispDenseRows& rows, const double* X, int64_t ldx, const double* y,
                   const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step, int K, int p,
                   int intercept, double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv,
                   double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host,
                   double* pearson_host, double* deviance_host, void* ws, size_t ws_bytes, void* stream) {
    DLSA_REQUIRE(X && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "%s: null argument", who);
    const int pe = p + (intercept ? 1 : 0);
    DLSA_REQUIRE(K > 0 && p > 0 && pe <= 2048 && ldx >= p && row_step >= 1, "%s: bad shape K=%d p=%d ldx=%lld step=%lld", who, K, p,
                 (long long)ldx, (long long)row_step);
    int64_t max_rows;
    int rc = disp_fit_args(who, f, dispersion_fixed, tol, max_iter, part_first_host, part_rows_host, K, max_rows);
    if (rc) return rc;
    const DispLayout l = disp_layout(f.nc, max_rows, p, pe, row_step);
    rc = newton_check_ws(who, ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    const DispFitBufs b = disp_bufs_at(wsc, l, pe);
    const int64_t pitch = ldx * row_step;                     // rows first, first + step, ...: a strided view, no copy of X
    const DispEval eval = [&](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* Hk, double* g,
                              double* ll, double* mu) {
        return rows(X + part_first_host[k] * ldx, pitch, yk, ok, beta, nk, p, intercept, Hk, pe, g, ll, b.w, mu,
                    count_scratch_at(wsc, l.sc), wsc + l.off_gram, l.off_state - l.off_gram, s);
    };
    return disp_fit_core(who, f, y, offset, part_first_host, part_rows_host, row_step, K, pe, intercept ? 0 : -1, dispersion_fixed, tol,
                         max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, dispersion_host, pearson_host,
                         deviance_host, b, eval, s);
}

// ---- the structured one-hot entries (the row checks of num / codes and the plan's constant column: poisson_internal.h) ---------
size_t disp_onehot_workspace_bytes(int nc, const dlsa_onehot_plan* plan, int64_t max_rows, int64_t row_step) {
    if (!plan || max_rows < 0 || row_step < 1) return 0;
    return disp_onehot_layout(nc, plan, max_rows, row_step).total;
}

int disp_onehot_pass_entry(const char* who, const DispFamily& f, const DispOnehotRows& rows, const dlsa_onehot_plan* plan,
                           const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y, const double* offset,
                           const double* beta, double dispersion, int64_t n, double* H, int64_t ldh, double* g, double* loglik,
                           double* w_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    DLSA_REQUIRE(plan && y && beta, "%s: null plan, y or beta", who);
    int rc = oh_pois_check_rows(who, plan, num, ldn, codes, ldc);
    if (rc) return rc;
    const int p = onehot_plan_p(plan);
    DLSA_REQUIRE(n >= 1 && (!H || ldh >= p), "%s: bad shape n=%lld p=%d ldh=%lld", who, (long long)n, p, (long long)ldh);
    DLSA_REQUIRE(!f.bad_param, "%s: %s", who, f.bad_param);
    DLSA_REQUIRE(dispersion > 0 && isfinite(dispersion), "%s: the dispersion must be positive and finite", who);
    const DispLayout l = disp_onehot_layout(f.nc, plan, n, 1);
    rc = newton_check_ws(who, ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    const DispFitBufs b = disp_bufs_at(wsc, l, p);
    double* w = w_out ? w_out : (H ? b.w : nullptr);
    double* mu = stats_out ? b.mu : nullptr;
    rc = rows(plan, num, ldn, codes, ldc, y, offset, beta, n, H, ldh, g, loglik, w, mu, wsc + l.off_oh, l.oh_bytes, s);
    if (rc) return rc;
    return disp_pass_finish(f, y, offset, mu, n, p, dispersion, H, ldh, g, loglik, stats_out, b, s);
}

int disp_onehot_fit_entry(const char* who, const DispFamily& f, const DispOnehotRows& rows, const dlsa_onehot_plan* plan,
                          const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y, const double* offset,
                          const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step, int K,
                          double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                          int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host,
                          double* deviance_host, void* ws, size_t ws_bytes, void* stream) {
    DLSA_REQUIRE(plan && y && part_first_host && part_rows_host && coef && Sig_inv && Sig_invMcoef, "%s: null argument", who);
    int rc = oh_pois_check_rows(who, plan, num, ldn, codes, ldc);
    if (rc) return rc;
    DLSA_REQUIRE(K > 0 && row_step >= 1, "%s: bad shape K=%d step=%lld", who, K, (long long)row_step);
    int64_t max_rows;
    rc = disp_fit_args(who, f, dispersion_fixed, tol, max_iter, part_first_host, part_rows_host, K, max_rows);
    if (rc) return rc;
    const int p = onehot_plan_p(plan);
    const DispLayout l = disp_onehot_layout(f.nc, plan, max_rows, row_step);
    rc = newton_check_ws(who, ws, ws_bytes, l.total);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* wsc = (char*)ws;
    const DispFitBufs b = disp_bufs_at(wsc, l, p);
    const int64_t pn = ldn * row_step, pc = ldc * row_step;   // rows first, first + step, ...: strided views, num / codes read in place
    const DispEval eval = [&](int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* Hk, double* g,
                              double* ll, double* mu) {
        const double* numk = num ? num + part_first_host[k] * ldn : nullptr;
        const int32_t* codesk = codes ? codes + part_first_host[k] * ldc : nullptr;
        return rows(plan, numk, pn, codesk, pc, yk, ok, beta, nk, Hk, p, g, ll, b.w, mu, wsc + l.off_oh, l.oh_bytes, s);
    };
    return disp_fit_core(who, f, y, offset, part_first_host, part_rows_host, row_step, K, p, oh_pois_icpt_col(plan), dispersion_fixed,
                         tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter_host, status_host, loglik_host, dispersion_host,
                         pearson_host, deviance_host, b, eval, s);
}

}  // namespace dlsa
