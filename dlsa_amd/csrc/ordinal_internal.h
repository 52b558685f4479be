// What the ordinal (proportional-odds) family's two translation units (ordinal.hip: the dense rows, onehot_ordinal.hip: the raw
// representation of a one-hot design) share: the limits, the layout of the per-block scalar partials, the terms of one row, the
// host launchers of the mask, assemble and start kernels (ordinal.hip's) and the per-partition fit driver that takes the
// evaluation as a callable.  The class check, the gather of a strided partition's responses and the Newton state, loop and
// epilogue are the multinomial family's, poisson_internal.h's and newton_fit.h's.
#pragma once
#include "common.h"
#include "multinomial_internal.h"   // MN_MAX_CLASSES, mn_check, mn_ll_fix, exp_full (poisson_exp.h)

namespace dlsa {

constexpr int ORD_MAX_CLASSES = MN_MAX_CLASSES;
constexpr int ORD_MAX_J = ORD_MAX_CLASSES - 1;
// the scalar sums of a pass, one row of ORD_SC doubles per block: g_alpha (J), the corner's diagonal (J), its off-diagonal (J - 1)
constexpr int ORD_SC = 32;
constexpr int ORD_SC_GA = 0, ORD_SC_DG = ORD_MAX_J, ORD_SC_OF = 2 * ORD_MAX_J;
// in-pass borders where the C accumulator sets of NC double2 fit the lane's registers
constexpr int ORD_BORDER_SETS = 16;
static inline bool ord_border_in_pass(int classes, int nc) { return classes * nc <= ORD_BORDER_SETS; }

struct OrdStart { double a[ORD_MAX_J]; };

// ---- ordinal.hip: the host launchers of its kernels (the library has no relocatable device code, so the structured sibling
// onehot_ordinal.hip reaches them through these) ---------------------------------------------------------------------------
// v[i] = -(1[y = j - 1] A Abar + 1[y = j] B Bbar) of n rows for cutpoint j (1-based): the route without in-pass borders
int ord_mask(const double* y, const double* aa, const double* bb, int j, int64_t n, double* v, hipStream_t s);
// g (nullable, d entries): g_alpha from sc and, with gbeta (nullable, p values), g_beta copied from it; of H (nullable; d x d,
// pitch ldh) the J border rows and columns and the tridiagonal corner, both triangles, from sc (the layout above) and the border
// vectors bd[j * ldbd + k] = (X'v_{j+1})_k
int ord_assemble(const double* sc, const double* bd, int ldbd, int J, int p, double* H, int64_t ldh, double* g, const double* gbeta,
                 hipStream_t s);
// the Newton start: theta = [st.a | 0], d = J + p entries
int ord_start(double* theta, int J, int d, const OrdStart& st, hipStream_t s);

// device scratch of the fit loop
struct OrdFitBufs {
    double* cpart;     // MN_NQ * MN_CHECK_BLOCKS
    double* cst;       // MN_NQ
    double* ybuf;      // max_rows when row_step > 1: the gathered responses
    NewtonState st;
};

// The per-partition driver of the ordinal fits, in the shape of mn_fit_core (multinomial_internal.h): the data check of EVERY
// partition first (a partition that lacks a class merges two cutpoints, and the blocks of different partitions must mean the same
// parameter), then per partition the null model's start (alpha_j = the logit of the cumulative class share, beta = 0),
// newton_fit_loop with the policy NEWTON_POISSON on d = J + p coefficients and newton_fit_finish.  eval(k, yk, nk, theta, H, g, ll)
// is the only part that knows the representation of the design; `who` prefixes messages.
template <class Eval>
static int ord_fit_core(const char* who, const double* y, const int64_t* part_first_host, const int64_t* part_rows_host, int64_t row_step,
                        int K, int p, int classes, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                        int* n_iter_host, int* status_host, double* loglik_host, const OrdFitBufs& b, Eval&& eval, hipStream_t s) {
    const int J = classes - 1, d = J + p;
    std::vector<double> counts((size_t)K * MN_NQ, 0.0);
    const double* yk = nullptr;
    const double* none = nullptr;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_rows_host[k];
        if (nk <= 0) continue;
        int rc = pois_gather_rows(y, nullptr, part_first_host[k], row_step, nk, b.ybuf, nullptr, yk, none, s);
        if (rc) return rc;
        rc = mn_check(yk, nk, classes, b.cpart, b.cst, s);
        if (rc) return rc;
        double* cst = counts.data() + (size_t)k * MN_NQ;
        DLSA_HIP_CHECK(hipMemcpyAsync(cst, b.cst, MN_NQ * sizeof(double), hipMemcpyDeviceToHost, s));
        DLSA_HIP_CHECK(hipStreamSynchronize(s));
        if (cst[MN_BAD] > 0.0) {
            set_error("%s: partition %d has %.0f rows whose response is not a class code 0 .. %d", who, k, cst[MN_BAD], classes - 1);
            return DLSA_ERR_INVALID;
        }
        for (int c = 0; c < classes; ++c) {
            if (!(cst[c] > 0.0)) {
                set_error("%s: partition %d has no row of class %d: its maximum-likelihood fit merges two cutpoints", who, k, c);
                return DLSA_ERR_INVALID;
            }
        }
    }
    int overall = DLSA_OK;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_rows_host[k];
        double* Hk = Sig_inv + (size_t)k * d * d;
        double* ck = coef + (size_t)k * d;
        double* sk = Sig_invMcoef + (size_t)k * d;
        int st_k = DLSA_PART_EMPTY, iters = 0;
        double ll = 0.0;
        if (nk > 0) {
            int rc = pois_gather_rows(y, nullptr, part_first_host[k], row_step, nk, b.ybuf, nullptr, yk, none, s);
            if (rc) return rc;
            const double* cst = counts.data() + (size_t)k * MN_NQ;
            OrdStart start{};
            double cum = 0.0;
            for (int j = 0; j < J; ++j) {
                cum += cst[j];
                start.a[j] = log(cum / ((double)nk - cum));           // the logit of the cumulative class share
            }
            rc = ord_start(b.st.beta, J, d, start, s);
            if (rc) return rc;
            const NewtonDevice dev{b.st, Hk, d, s};
            NewtonOutcome o;
            rc = newton_fit_loop(NEWTON_POISSON, tol, max_iter + 1, [&](bool&) { return eval(k, yk, nk, b.st.beta, Hk, b.st.g, b.st.stats + 3); },
                                 dev, newton_no_hook, o);
            if (rc) return rc;
            st_k = o.status; iters = o.n_iter; ll = o.ll;
        }
        const int rcf = newton_fit_finish(st_k, iters, ll, b.st.beta, d, Hk, ck, sk, k, n_iter_host, status_host, loglik_host, overall, s);
        if (rcf) return rcf;
    }
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    return overall;
}

#if defined(__HIPCC__)
// F(t) and F(-t) of the logistic cdf and log F(t), each from e^{-|t|}: no cancellation on either side
static __device__ __forceinline__ void ord_logistic(double t, double& F, double& Fbar, double& logF) {
    const double e = exp_full(-fabs(t));
    const double big = 1.0 / (1.0 + e), small = e * big;
    const bool pos = t >= 0.0;
    F = pos ? big : small;
    Fbar = pos ? small : big;
    logF = (pos ? 0.0 : t) - log1p(e);
}

// One row of class c (the class code as a double; a value that is no class code reads as class 0) at eta = x'beta.
// al[j] = alpha_{j+1}, E[c] / logE[c] the class factors (1 / 0 for the two end classes).  Out: the log-likelihood term, resid =
// dl/deta = B - Abar (what multiplies x in g_beta), w = A Abar + B Bbar, aa = A Abar, bb = B Bbar, su, sl, q.  The end classes
// take A = 1, Abar = 0 (top) and B = 0, Bbar = 1 (class 0) by select: no infinity enters the arithmetic, nothing is indexed by y.
template <int J>
static __device__ __forceinline__ void ord_row_terms(double yraw, double eta, const double (&al)[J], const double (&E)[J + 1],
                                                     const double (&logE)[J + 1], double& llt, double& resid, double& aa, double& bb,
                                                     double& su, double& sl, double& q) {
    double au = al[0], alo = al[0], Ec = E[0], lEc = logE[0];
#pragma unroll
    for (int c = 1; c <= J; ++c) {
        const bool is = yraw == (double)c;
        au = (is && c < J) ? al[c < J ? c : J - 1] : au;
        alo = is ? al[c - 1] : alo;
        Ec = is ? E[c] : Ec;
        lEc = is ? logE[c] : lEc;
    }
    const bool top = yraw == (double)J, bot = !(yraw >= 1.0 && yraw <= (double)J);
    double A, Ab, lA, Bb, B, lBb;
    ord_logistic(au - eta, A, Ab, lA);
    ord_logistic(eta - alo, Bb, B, lBb);            // Bbar = F(-l), B = F(l), log Bbar
    A = top ? 1.0 : A; Ab = top ? 0.0 : Ab; lA = top ? 0.0 : lA;
    B = bot ? 0.0 : B; Bb = bot ? 1.0 : Bb; lBb = bot ? 0.0 : lBb;
    llt = lA + lBb + lEc;
    resid = B - Ab;
    aa = A * Ab;
    bb = B * Bb;
    su = Ab / (Bb * Ec);
    sl = B / (A * Ec);
    q = su * sl;
}
#endif

}  // namespace dlsa
