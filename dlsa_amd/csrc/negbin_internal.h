// What is NB2's among the things the negative-binomial translation units (negbin.hip: the dense rows, onehot_negbin.hip: the raw
// representation of a one-hot design) share: the row's terms, the host launchers of the dispersion step and the log-likelihood
// fix, and the per-partition fit driver that takes the model-specific steps as callables.  The kernels are negbin.hip's: the
// library is built without relocatable device code, so the other unit reaches them through these host functions.
#pragma once
#include "common.h"
#include "poisson_internal.h"
#include <math.h>
#include <functional>

namespace dlsa {

// the NB2 row at theta = 1 / alpha: weight mu q, residual (y - mu) q, term y eta - (y + theta) L
struct NbRow {
    static constexpr bool STORES_MU = true;
    double alpha;          // >= 0 (0: the Poisson limit, used by the fit at its start)
    double theta;          // 1 / alpha
    double log_alpha;
    __device__ __forceinline__ void terms(double yv, double eta, double mu, double& wgt, double& rs, double& llt) const {
        const double amu = alpha * mu;
        // one reciprocal: q = 1 / (1 + alpha mu), w = mu q; where alpha mu overflowed (or is NaN) the limits w = 1 / alpha, q = 0
        const bool big = !(amu <= 1e300);
        const double q = big ? 0.0 : 1.0 / (1.0 + amu);
        wgt = big ? theta : mu * q;
        const double L = amu < 9007199254740992.0 ? log1p(amu) : (mu < INFINITY ? eta + log_alpha : INFINITY);
        rs = big ? -theta : (yv - mu) * q;
        llt = yv * eta - (alpha > 0.0 ? (yv + theta) * L : mu);      // (y + theta) L -> mu as alpha -> 0
    }
};

constexpr int NB_THETA_BLOCKS = 2048;
// theta-step sums: c (without lgamma(y+1)), s, i, Pearson, sum (y-mu)^2 - y, bad rows, sum (y-mu)^2 - mu, sum mu^2, sum lgamma(y+1),
// sum (y + theta) L (the alpha-dependent part of the row log-likelihood: lets the driver move it from one alpha to the next)
constexpr int NB_NQ = 10;
enum { NB_C = 0, NB_S = 1, NB_I = 2, NB_PEARSON = 3, NB_D0 = 4, NB_BAD = 5, NB_M1 = 6, NB_M2 = 7, NB_LG = 8, NB_YL = 9 };

// the NB_NQ sums over (y, mu) at theta = 1 / alpha (alpha = 0: no special functions) into tst (device, 16 doubles); tpart:
// NB_NQ * NB_THETA_BLOCKS doubles of scratch; off (nullable) is read for the data check only; want_lg: also sum lgamma(y + 1)
int nb_theta_launch(const double* y, const double* mu, const double* off, int64_t n, double alpha, int want_lg, double* tpart,
                    double* tst, hipStream_t s);
// ll[0] = tst[NB_BAD] > 0 ? NaN : ll[0] + tst[NB_C] - tst[NB_LG]: the pass entries' full log-likelihood
int nb_ll_fix(double* ll, const double* tst, hipStream_t s);

// device scratch of the fit loop
struct NbFitBufs {
    double* ybuf;      // max_rows when row_step > 1: the gathered counts
    double* obuf;      // max_rows when row_step > 1 and offsets are given
    double* w;         // max_rows: the Gram's weights
    double* mu;        // max_rows: what the dispersion step reads
    double* tpart;     // NB_NQ * NB_THETA_BLOCKS
    double* tst;       // 16
    NewtonState st;
};

// "fit the Poisson block of partition k into (ck, Hk, sk)": iters (nullable), st_k and ll as the Poisson fit entries report them
// for that one partition; returns their code (an invalid partition: DLSA_ERR_INVALID)
using NbPoisFit = std::function<int(int k, double* ck, double* Hk, double* sk, int* iters, int* st_k, double* ll)>;
// "evaluate (H, g, the row log-likelihood, w, mu) at (beta, alpha) for partition k": yk / ok (nullable) are the partition's nk > 0
// counts and offsets, contiguous (gathered when the partition is strided); alpha = 0 is the Poisson limit (then only mu is asked
// for); H is pe x pe (ldh = pe, both triangles); H, g, ll, w nullable
using NbEval = std::function<int(int k, const double* yk, const double* ok, int64_t nk, const double* beta, double alpha, double* H,
                                 double* g, double* ll, double* w, double* mu)>;

// The per-partition driver of the NB2 fits: the Poisson start (the data check, the EMPTY block, the answer where alpha = 0), the
// look at the Poisson MLE at alpha = 0, the moment start, the theta solve, newton_fit_loop with the policy NEWTON_NB2 and the theta
// hook, the "fell back to Poisson" branches and the epilogue.  alpha_fixed > 0: no theta steps.  `who` prefixes messages.
int nb_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host, const int64_t* part_rows_host,
                int64_t row_step, int K, int pe, double alpha_fixed, double tol, int max_iter, double* coef, double* Sig_inv,
                double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, double* alpha_host,
                double* alpha_info_host, double* pearson_host, const NbFitBufs& b, const NbPoisFit& pois, const NbEval& eval,
                hipStream_t s);

}  // namespace dlsa
