// What is the Tweedie family's among the things its two translation units (tweedie.hip: the dense rows, onehot_tweedie.hip: the
// raw representation of a one-hot design) share: the host launchers of the once-per-partition sums and of the dispersion sums, the
// epilogue of a pass entry, the per-partition fit driver that takes the evaluation as a callable, and the arithmetic of a row that the
// two row models share.  The kernels are tweedie.hip's: the library is built without relocatable device code, so the other unit
// reaches them through these host functions.  The sum finish and the dispersion scaling are gamma.hip's (gamma_internal.h), the gather of a strided partition's
// responses and offsets and the start launcher poisson_internal.h's.
#pragma once
#include "common.h"
#include "poisson_internal.h"
#include "gamma_internal.h"
#include <functional>

namespace dlsa {

// once per partition: [sum y e^((1 - xi) o), sum e^((2 - xi) o), rows with y < 0 or a non-finite y / o, rows with y > 0]
constexpr int TWEEDIE_NC = 4;
enum { TWEEDIE_YEO = 0, TWEEDIE_EO = 1, TWEEDIE_BAD = 2, TWEEDIE_POS = 3 };
// the dispersion sums over (y, mu): [Pearson sum (y - mu)^2 mu^-xi, the deviance] -- the order of GAMMA_PEARSON / GAMMA_DEV
constexpr int TWEEDIE_ND = GAMMA_ND;

// 1 < power < 2 (a NaN fails both comparisons)
static inline bool tweedie_power_ok(double power) { return power > 1.0 && power < 2.0; }

#include "poisson_exp.h"  // exp_full

// exp(c x) without the rounding of the product c x: the product's low part enters as the factor 1 + lo (|lo| <= ulp(c x) / 2)
static __device__ __forceinline__ double tweedie_exp_prod(double c, double x) {
    const double hi = c * x, lo = fma(c, x, -hi);
    const double e = exp_full(hi);
    return fma(e, lo, e);
}

// what both row models compute of a row at unit dispersion, with a = mu^(1 - xi): y a, b = mu a and the weight (xi - 1) y a + (2 - xi) b.
// The residual is ya - b, the term ya / (1 - xi) - b / (2 - xi).
static __device__ __forceinline__ void tweedie_row(double one_m_xi, double two_m_xi, double y, double eta, double mu, double& ya,
                                                   double& b, double& w) {
    const double a = tweedie_exp_prod(one_m_xi, eta);
    b = mu * a;
    ya = y * a;
    w = fma(-one_m_xi, ya, two_m_xi * b);
}

// cst[0..3] = the TWEEDIE_NC sums of n rows (off nullable); cpart: TWEEDIE_NC * GAMMA_SUM_BLOCKS doubles of scratch
int tweedie_const(const double* y, const double* off, int64_t n, double power, double* cpart, double* cst, hipStream_t s);
// dst[0..1] = [P, Dev] of n rows; dpart: TWEEDIE_ND * GAMMA_SUM_BLOCKS doubles of scratch.  Fixed-order: bit-reproducible
int tweedie_disp(const double* y, const double* mu, int64_t n, double power, double* dpart, double* dst, hipStream_t s);

// The epilogue the two pass entries share, after the row pass at unit dispersion has left H, g, the row sum of q in loglik and
// (stats_out wanted) mu: [P, Dev] into stats_out, H and g times nu = 1 / dispersion, loglik = nu sum q, the quasi-log-likelihood
// (NaN when a row is not a valid response).  H, g, loglik, stats_out nullable.
int tweedie_pass_finish(const double* y, const double* off, const double* mu, int64_t n, int pe, double power, double dispersion,
                        double* H, int64_t ldh, double* g, double* loglik, double* stats_out, double* cpart, double* cst,
                        double* dpart, hipStream_t s);

// device scratch of the fit loop
struct TweedieFitBufs {
    double* cpart;     // TWEEDIE_NC * GAMMA_SUM_BLOCKS
    double* cst;       // 4
    double* dpart;     // TWEEDIE_ND * GAMMA_SUM_BLOCKS
    double* dst;       // 4
    double* ybuf;      // max_rows when row_step > 1: the gathered responses
    double* obuf;      // max_rows when row_step > 1 and offsets are given
    double* mu;        // max_rows: mu of the last evaluation, what the dispersion sums read
    NewtonState st;
};

// "evaluate (H, g, sum q, mu) at beta and unit dispersion for partition k", at the power the callable carries: yk / ok (nullable)
// are the partition's nk > 0 responses and offsets, contiguous (gathered when the partition is strided); H is pe x pe (ldh = pe,
// both triangles), g pe, ll one device double, mu nk
using TweedieEval = std::function<int(int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* H, double* g,
                                      double* ll, double* mu)>;

// The per-partition driver of the Tweedie fits: the refusal of a partition without degrees of freedom (estimated dispersion, 0 < n
// <= pe), data check (an invalid response or offset, no positive response) and sums, start at beta = 0 with entry icpt_col (-1:
// none) at log(sum y e^((1 - xi) o) / sum e^((2 - xi) o)), newton_fit_loop with the policy NEWTON_POISSON at unit dispersion (the
// iteration does not depend on it), then the dispersion from the mu of the evaluation that left H, Sig_inv = H / dispersion,
// loglik = sum q / dispersion, and newton_fit_finish.  dispersion_fixed > 0: every block uses it.  `who` prefixes messages.
int tweedie_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host,
                     const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double power,
                     double dispersion_fixed, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef,
                     int* n_iter_host, int* status_host, double* loglik_host, double* dispersion_host, double* pearson_host,
                     double* deviance_host, const TweedieFitBufs& b, const TweedieEval& eval, hipStream_t s);

}  // namespace dlsa
