// What poisson.hip shares with the other Poisson translation units (onehot_poisson.hip).  The library is built without
// relocatable device code, so a kernel is launched by the file that defines it: these are HOST functions of poisson.hip.
#pragma once
#include "common.h"
#include <functional>

namespace dlsa {

constexpr int POIS_CONST_BLOCKS = 512;

// cst[0..3] = [sum lgamma(y + 1), sum y, sum e^o, rows with y < 0 or a non-finite y / o] of n rows (off nullable);
// cpart: 4 * POIS_CONST_BLOCKS doubles of scratch
int pois_const(const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s);
// ll[0] = cst[3] > 0 ? NaN : ll[0] - cst[0]: the pass entries' full log-likelihood
int pois_ll_fix(double* ll, const double* cst, hipStream_t s);

// device scratch of the fit loop
struct PoisFitBufs {
    double* cpart;     // 4 * POIS_CONST_BLOCKS
    double* cst;       // 4
    double* ybuf;      // max_rows when row_step > 1: the gathered counts
    double* obuf;      // max_rows when row_step > 1 and offsets are given
    double* state;     // 4 * pe + 8: stats[8], beta, prev, delta, g
    double* Lf;        // pe * pe: the Cholesky factor
};
static inline size_t pois_state_bytes(int pe) {                 // state, then the Cholesky factor
    return align_up(8 * (size_t)(4 * pe + 8), 256) + align_up(8 * (size_t)pe * pe, 256);
}

// "evaluate (H, g, sum y eta - mu) at beta for partition k": yk / ok (nullable) are the partition's nk > 0 counts and offsets,
// contiguous (gathered when the partition is strided); H is pe x pe (ldh = pe, both triangles), g pe, ll one device double
using PoisEval = std::function<int(int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* H,
                                   double* g, double* ll)>;

// The per-partition Newton loop of the Poisson fits: data check and constant term, start at beta = 0 with entry icpt_col
// (-1: none) at log(sum y / sum e^o), Cholesky solve, step halving (<= 30) while the likelihood drops or is not finite, the
// IRLS stopping rule, Sig_inv = H at the returned coef, EMPTY + zero block without rows or events.  `who` prefixes messages.
int pois_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host,
                  const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double tol, int max_iter,
                  double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                  const PoisFitBufs& b, const PoisEval& eval, hipStream_t s);

}  // namespace dlsa
