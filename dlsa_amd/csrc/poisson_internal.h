// What the count-model translation units (poisson.hip, onehot_poisson.hip, negbin.hip) share: the host functions of poisson.hip
// the others call, the Newton state's carving, and the one declaration of what they all use from the rest of the library.  The
// library is built without relocatable device code, so a kernel is launched by the file that defines it: these are HOST functions.
#pragma once
#include "common.h"
#include <functional>

namespace dlsa {

// gram.hip, logit.hip, chol.hip, dense.hip
int gram_impl_f64(const double* X, int64_t ldx, const double* w, int64_t n, int p, double* H, int64_t ldh,
                  int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);
size_t gram_workspace_bytes_impl(int64_t n, int p, int elem_bytes);
int gram_icpt_impl(const double* X, int64_t ldx, const double* w, int64_t n, int p, double* H, int64_t ldh,
                   void* ws, size_t ws_bytes, hipStream_t s, const double* border);
void logit_finish_launch(const double* gpart, const double* llpart, int nblocks, int pitch, int p, double* g,
                         double* loglik, hipStream_t stream, const double* s0part, double* s0);
int launch_chol_solve(const double* A, int64_t lda, int64_t strideA, const double* rhs, int64_t stride_rhs,
                      const double* ref, int64_t stride_ref, int p, int nsys, double* Lws, double* xout,
                      int64_t stride_x, double* stats, int64_t stride_stats, hipStream_t s, int reuse_factor);
int launch_matvec(const double* A, int64_t lda, const double* x, int p, double* y, hipStream_t s);
int launch_axpby(const double* a, const double* b, double sc, int n, double* out, hipStream_t s);
int launch_advance(double* prev, double* beta, const double* delta, int n, hipStream_t s);

constexpr int POIS_CONST_BLOCKS = 512;

// cst[0..3] = [sum lgamma(y + 1), sum y, sum e^o, rows with y < 0 or a non-finite y / o] of n rows (off nullable);
// cpart: 4 * POIS_CONST_BLOCKS doubles of scratch
int pois_const(const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s);
// ll[0] = cst[3] > 0 ? NaN : ll[0] - cst[0]: the pass entries' full log-likelihood
int pois_ll_fix(double* ll, const double* cst, hipStream_t s);
// out[j] = v[first + j * step], j < n: a strided partition's counts or offsets, gathered once (8 bytes per row)
int pois_gather(const double* v, int64_t first, int64_t step, int64_t n, double* out, hipStream_t s);

// The Newton state of a fit: stats[8] ([0] |delta|_inf, [1] |beta|_inf, [2] factor status, [3] the row log-likelihood), beta,
// prev, delta, g (pe each), then the pe x pe Cholesky factor -- one block of pois_state_bytes(pe), carved by pois_state_at
struct PoisState { double *stats, *beta, *prev, *delta, *g, *Lf; };
static inline size_t pois_state_bytes(int pe) {
    return align_up(8 * (size_t)(4 * pe + 8), 256) + align_up(8 * (size_t)pe * pe, 256);
}
static inline PoisState pois_state_at(void* block, int pe) {
    double* st = (double*)block;
    return {st, st + 8, st + 8 + pe, st + 8 + 2 * pe, st + 8 + 3 * pe, (double*)((char*)block + align_up(8 * (size_t)(4 * pe + 8), 256))};
}

// device scratch of the fit loop
struct PoisFitBufs {
    double* cpart;     // 4 * POIS_CONST_BLOCKS
    double* cst;       // 4
    double* ybuf;      // max_rows when row_step > 1: the gathered counts
    double* obuf;      // max_rows when row_step > 1 and offsets are given
    PoisState st;
};

// a partition's status folded into the fit's return code: the first soft failure stands
static inline void pois_fold_status(int st_k, int& overall) {
    if (overall != DLSA_OK) return;
    if (st_k == DLSA_PART_NOT_CONVERGED) overall = DLSA_ERR_NOT_CONVERGED;
    if (st_k == DLSA_PART_NOT_SPD) overall = DLSA_ERR_NOT_SPD;
    if (st_k == DLSA_PART_NAN) overall = DLSA_ERR_NAN;
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
