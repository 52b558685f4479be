// What is the multinomial family's among the things its two translation units (multinomial.hip: the dense rows,
// onehot_multinomial.hip: the raw representation of a one-hot design) share: the limits, the softmax of one row, the host launchers
// of the once-per-partition check and of the weight, mirror, start and log-likelihood-fix kernels, and the per-partition fit driver
// of every family whose response is a class code (the ordinal family's too), which takes the start and the evaluation as callables.  The kernels are multinomial.hip's: the library is built without relocatable device code,
// so the other unit reaches them through these host functions.  The gather of a strided partition's responses is
// poisson_internal.h's, the Newton state, loop and epilogue newton_fit.h's.
#pragma once
#include "common.h"
#include "poisson_internal.h"
#include <math.h>
#include <algorithm>
#include <vector>

namespace dlsa {

constexpr int MN_MAX_CLASSES = 8;
constexpr int MN_NQ = MN_MAX_CLASSES + 1;       // the check's sums: the rows of class 0 .. 7, then the bad rows
constexpr int MN_BAD = MN_MAX_CLASSES;
constexpr int MN_CHECK_BLOCKS = 512;

#include "poisson_exp.h"  // exp_full

// The softmax of one row with the reference class at eta_0 = 0: p[j] = the probability of class j + 1, returns the row's
// log-likelihood term log p_y (y = the class code as a double; a value that is no class code reads as the reference class).
// M = max(0, eta_1 .. eta_J), every exponential takes a non-positive argument, the first term that attains M is exactly 1 and is
// left out of T = the sum of the others, so S = 1 + T, log S = log1p(T) and the term eta_y - M - log1p(T) keeps its relative
// accuracy when one class dominates.  Compare-and-select chains: nothing is indexed by y.
template <int J>
static __device__ __forceinline__ double mn_softmax_row(const double (&eta)[J], double yraw, double (&p)[J]) {
    double M = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) M = eta[j] > M ? eta[j] : M;
    bool found = M == 0.0;                                        // the reference class attains it
    double T = found ? 0.0 : exp_full(-M);
    double e[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        e[j] = exp_full(eta[j] - M);
        const bool hit = !found && eta[j] == M;
        T += hit ? 0.0 : e[j];
        found = found || hit;
    }
    const double inv = 1.0 / (1.0 + T);
    double eta_y = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) eta_y = yraw == (double)(j + 1) ? eta[j] : eta_y;
#pragma unroll
    for (int j = 0; j < J; ++j) p[j] = e[j] * inv;      // (before the log1p: computed after it, <1,2,8,true> of the dense pass loses a wave)
    return eta_y - M - log1p(T);
}

struct MnStart { double b0[MN_MAX_CLASSES - 1]; };

// the pitch of the class rows of P for n rows: 256-byte class rows
static inline int64_t mn_ldprob(int64_t n) { return (int64_t)align_up((size_t)std::max<int64_t>(n, 1), 32); }

// ---- multinomial.hip ---------------------------------------------------------------------------------------------------
// cst[0 .. 8] = the class counts and the bad rows of n responses; cpart: MN_NQ * MN_CHECK_BLOCKS doubles of scratch
int mn_check(const double* y, int64_t n, int classes, double* cpart, double* cst, hipStream_t s);
// ll[0] = NaN when cst[MN_BAD] > 0: the pass entries' log-likelihood when a row is not a class code
int mn_ll_fix(double* ll, const double* cst, hipStream_t s);
// the Newton start: theta = 0, entry icpt_col (-1: none) of class block j (pe entries each) at st.b0[j]
int mn_start(double* theta, int J, int pe, int icpt_col, const MnStart& st, hipStream_t s);
// w[i] = p_j (delta_jk - p_k) of n rows (same = (j == k)): the weights of the block (j, k) of the information
int mn_weight(const double* pj, const double* pk, int same, int64_t n, double* w, hipStream_t s);
// the blocks (k, j), j < k, of H ((J pe) x (J pe), pitch ldh) from their mirror images above the block diagonal
int mn_mirror(double* H, int64_t ldh, int J, int pe, hipStream_t s);
// 2 <= classes <= MN_MAX_CLASSES and (classes - 1) pe <= 2048 coefficients, pe > 0 per class block; `who` prefixes the message
int mn_coef_ok(const char* who, int pe, int classes);

// device scratch of the fit loop
struct MnFitBufs {
    double* cpart;     // MN_NQ * MN_CHECK_BLOCKS
    double* cst;       // MN_NQ
    double* ybuf;      // max_rows when row_step > 1: the gathered responses
    NewtonState st;
};

// The per-partition fit driver of the families whose response is a class code (multinomial, ordinal; dense and structured), beside
// pois_fit_core: the data check of EVERY partition first (a partition that lacks a class has no finite MLE -- `no_class` ends the
// refusal in the family's words -- and the blocks of different partitions must mean the same parameter), then per partition the
// family's start, newton_fit_loop with the policy NEWTON_POISSON on d coefficients and newton_fit_finish.
//   start(cst, nk, theta, s)                   theta = the null model's MLE from the class counts cst[0 .. classes - 1] of the nk rows
//   eval(k, yk, nk, theta, H, g, ll)           the only part that knows the representation of the design
template <class Start, class Eval>
static int mn_fit_core(const char* who, const char* no_class, const double* y, const int64_t* part_first_host, const int64_t* part_rows_host,
                       int64_t row_step, int K, int d, int classes, double tol, int max_iter, double* coef, double* Sig_inv,
                       double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, const MnFitBufs& b, Start&& start,
                       Eval&& eval, hipStream_t s) {
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
                set_error("%s: partition %d has no row of class %d: its maximum-likelihood fit %s", who, k, c, no_class);
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
            rc = start(counts.data() + (size_t)k * MN_NQ, nk, b.st.beta, s);
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

constexpr char MN_NO_CLASS[] = "runs off to eta = -inf";       // what a partition without a row of some class does to the fit

// the multinomial fits' start: theta = 0 with entry icpt_col (-1: none) of class block j (pe entries each) at log(n_j / n_0), the
// exact MLE of the intercept-only model
static inline auto mn_null_start(int J, int pe, int icpt_col) {
    return [=](const double* cst, int64_t, double* theta, hipStream_t s) {
        MnStart start{};
        for (int j = 0; j < J; ++j) start.b0[j] = log(cst[j + 1] / cst[0]);
        return mn_start(theta, J, pe, icpt_col, start, s);
    };
}

}  // namespace dlsa
