// What is the Gamma family's among the things its two translation units (gamma.hip: the dense rows, onehot_gamma.hip: the raw
// representation of a one-hot design) share: the host launchers of the once-per-partition sums, the dispersion sums and the
// dispersion scaling, the epilogue of a pass entry, and the per-partition fit driver that takes the evaluation as a callable.
// The kernels are gamma.hip's: the library is built without relocatable device code, so the other unit reaches them through
// these host functions.  The gather of a strided partition's responses and offsets is poisson_internal.h's.
#pragma once
#include "common.h"
#include "poisson_internal.h"
#include <functional>

namespace dlsa {

constexpr int GAMMA_SUM_BLOCKS = 1024;
// once per partition: [sum log y, sum y e^-o, rows with y <= 0 or a non-finite y / o]
constexpr int GAMMA_NC = 3;
enum { GAMMA_LOGY = 0, GAMMA_YEO = 1, GAMMA_BAD = 2 };
// the dispersion sums over (y, mu): [Pearson sum (r - 1)^2, deviance 2 sum (r - 1 - log r)], r = y / mu
constexpr int GAMMA_ND = 2;
enum { GAMMA_PEARSON = 0, GAMMA_DEV = 1 };

// cst[0..2] = the GAMMA_NC sums of n rows (off nullable); cpart: GAMMA_NC * GAMMA_SUM_BLOCKS doubles of scratch
int gamma_const(const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s);
// dst[0..1] = the GAMMA_ND sums of n rows; dpart: GAMMA_ND * GAMMA_SUM_BLOCKS doubles of scratch.  Fixed-order: bit-reproducible
int gamma_disp(const double* y, const double* mu, int64_t n, double* dpart, double* dst, hipStream_t s);
// out[j] = the sum over b < nblocks of part[b * nq + j], j < nq <= 4, in a fixed order: the finish of gamma_const / gamma_disp and
// of the Tweedie family's per-block sums (tweedie.hip)
int gamma_sum_finish(const double* part, int nblocks, int nq, double* out, hipStream_t s);
// the blocks of a per-block sum kernel over n rows: at most GAMMA_SUM_BLOCKS workgroups of 256 threads
int gamma_sum_blocks(int64_t n);
// H (pe x pe, pitch ldh; nullable) and g (pe; nullable) times nu: the unit-dispersion quantities taken to dispersion 1 / nu
int gamma_scale(double* H, int64_t ldh, int pe, double* g, double nu, hipStream_t s);
// n (nu log nu - lgamma nu): the beta-free part of the log-likelihood that does not depend on y
double gamma_ll_const(double nu, int64_t n);

// The epilogue the two pass entries share, after the row pass at unit dispersion has left H, g, the row sum of -(r + eta) in
// loglik and (stats_out wanted) mu: [P, Dev] into stats_out, H and g times nu = 1 / dispersion, loglik the full log-likelihood
// at that dispersion (NaN when a row is not a valid response).  H, g, loglik, stats_out nullable.
int gamma_pass_finish(const double* y, const double* off, const double* mu, int64_t n, int pe, double dispersion, double* H,
                      int64_t ldh, double* g, double* loglik, double* stats_out, double* cpart, double* cst, double* dpart,
                      hipStream_t s);

// device scratch of the fit loop
struct GammaFitBufs {
    double* cpart;     // GAMMA_NC * GAMMA_SUM_BLOCKS
    double* cst;       // 4
    double* dpart;     // GAMMA_ND * GAMMA_SUM_BLOCKS
    double* dst;       // 4
    double* ybuf;      // max_rows when row_step > 1: the gathered responses
    double* obuf;      // max_rows when row_step > 1 and offsets are given
    double* mu;        // max_rows: mu of the last evaluation, what the dispersion sums read
    NewtonState st;
};

// "evaluate (H, g, sum -(r + eta), mu) at beta and unit dispersion for partition k": yk / ok (nullable) are the partition's
// nk > 0 responses and offsets, contiguous (gathered when the partition is strided); H is pe x pe (ldh = pe, both triangles),
// g pe, ll one device double, mu nk
using GammaEval = std::function<int(int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* H, double* g,
                                    double* ll, double* mu)>;

// The per-partition driver of the Gamma fits: the refusal of a partition without degrees of freedom (estimated dispersion, 0 < n
// <= pe), data check and sums, start at beta = 0 with entry icpt_col (-1: none) at log(sum y e^-o / n), newton_fit_loop with the
// policy NEWTON_POISSON at unit dispersion (the iteration does not depend on it), then the dispersion from the mu of the evaluation
// that left H, Sig_inv = H / dispersion, and newton_fit_finish.  dispersion_fixed > 0: every block uses it.  `who` prefixes messages.
int gamma_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host,
                   const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double dispersion_fixed, double tol,
                   int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                   double* loglik_host, double* dispersion_host, double* pearson_host, double* deviance_host, const GammaFitBufs& b,
                   const GammaEval& eval, hipStream_t s);

}  // namespace dlsa
