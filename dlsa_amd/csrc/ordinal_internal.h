// What the ordinal (proportional-odds) family's two translation units (ordinal.hip: the dense rows, onehot_ordinal.hip: the raw
// representation of a one-hot design) share: the limits, the layout of the per-block scalar partials, the terms of one row, the
// host launchers of the mask, assemble and start kernels (ordinal.hip's), the fits' start and, device side, the cutpoint preamble
// and the scalar sums of both row kernels.  The class check and the fit driver (mn_fit_core) are multinomial_internal.h's, the
// gather of a strided partition's responses poisson_internal.h's, the Newton state, loop and epilogue newton_fit.h's.
#pragma once
#include "common.h"
#include "multinomial_internal.h"   // MN_MAX_CLASSES, mn_check, mn_ll_fix, mn_fit_core, MnFitBufs, exp_full (poisson_exp.h)

namespace dlsa {

constexpr int ORD_MAX_CLASSES = MN_MAX_CLASSES;
constexpr int ORD_MAX_J = ORD_MAX_CLASSES - 1;
// the scalar sums of a pass, one row of ORD_SC doubles per block: g_alpha (J), the corner's diagonal (J), its off-diagonal (J - 1)
constexpr int ORD_SC = 32;
constexpr int ORD_SC_GA = 0, ORD_SC_DG = ORD_MAX_J, ORD_SC_OF = 2 * ORD_MAX_J;
// the slot of the row that sum i of a kernel's 3J - 1 goes to; the slots no sum goes to hold 0
template <int J>
constexpr int ord_sc_slot(int i) { return i < J ? ORD_SC_GA + i : i < 2 * J ? ORD_SC_DG + (i - J) : ORD_SC_OF + (i - 2 * J); }
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

constexpr char ORD_NO_CLASS[] = "merges two cutpoints";           // what a partition without a row of some class does to the fit

// the ordinal fits' start for mn_fit_core (multinomial_internal.h): alpha_j = the logit of the cumulative class share, beta = 0,
// the exact MLE of the null model on d = J + p coefficients
static inline auto ord_null_start(int J, int d) {
    return [=](const double* cst, int64_t nk, double* theta, hipStream_t s) {
        OrdStart start{};
        double cum = 0.0;
        for (int j = 0; j < J; ++j) {
            cum += cst[j];
            start.a[j] = log(cum / ((double)nk - cum));
        }
        return ord_start(theta, J, d, start, s);
    };
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

// The cutpoints al[j] = alpha[j] = alpha_{j+1} and the class factors E_c = -expm1(-(alpha_{c+1} - alpha_c)) of the interior classes
// (1 for the two end classes) with their logarithms: functions of theta alone, the same in every lane.  Returns whether the
// cutpoints increase strictly (a NaN cutpoint fails too).
template <int J>
static __device__ __forceinline__ bool ord_cutpoints(const double* alpha, double (&al)[J], double (&E)[J + 1], double (&logE)[J + 1]) {
#pragma unroll
    for (int j = 0; j < J; ++j) al[j] = alpha[j];
    bool ordered = true;
    E[0] = 1.0; logE[0] = 0.0; E[J] = 1.0; logE[J] = 0.0;
#pragma unroll
    for (int c = 1; c < J; ++c) {
        const double gap = al[c] - al[c - 1];
        ordered = ordered && gap > 0.0;
        E[c] = -expm1(-gap);
        logE[c] = log(E[c]);
    }
    return ordered;
}

// One row's share of the scalar sums sc = [g_alpha (J) | the corner's diagonal (J) | its off-diagonal (J - 1)] that belong to
// cutpoint j + 1, the upper one of class j and the lower one of class j + 1; a kernel calls it for j = 0 .. J - 1.  Selects, no
// branch on y; a row that is not `valid` adds 0.  (Per cutpoint, the loop in the kernel: with the loop in here
// oh_ord_row_kernel<2, true> takes 169 VGPRs for 167 and loses a wave.)
template <int J>
static __device__ __forceinline__ void ord_cutpoint_sums(int j, double y, bool valid, double su, double sl, double aa, double bb, double q,
                                                         double (&sc)[3 * J - 1]) {
    const bool up = valid && y == (double)j, lo = valid && y == (double)(j + 1);
    sc[j] += (up ? su : 0.0) - (lo ? sl : 0.0);
    sc[J + j] += (up ? aa + q : 0.0) + (lo ? bb + q : 0.0);
    if (j < J - 1) sc[2 * J + j] -= lo ? q : 0.0;
}
#endif

}  // namespace dlsa
