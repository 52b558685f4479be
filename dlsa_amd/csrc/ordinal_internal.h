// What the ordinal (proportional-odds) family keeps apart from its translation unit ordinal.hip: the limits, the layout of the
// per-block scalar partials and the terms of one row.  The class check, the gather of a strided partition's responses and the
// Newton state, loop and epilogue are the multinomial family's, poisson_internal.h's and newton_fit.h's.
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
