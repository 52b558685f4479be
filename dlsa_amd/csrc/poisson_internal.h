// What is Poisson's among the things the log-link translation units (poisson.hip, onehot_poisson.hip, negbin.hip,
// onehot_negbin.hip, gamma.hip, onehot_gamma.hip) share: the constant-term, log-likelihood-fix, start and gather launchers of
// poisson.hip, the fit driver that takes the evaluation as a callable, and the structured pass and plan helpers of onehot_poisson.hip.  The Newton state, loop and epilogue are newton_fit.h; the prototypes of the rest of the library are host_calls.h.
#pragma once
#include "common.h"
#include "newton_fit.h"
#include <functional>

namespace dlsa {

constexpr int POIS_CONST_BLOCKS = 512;

// cst[0..3] = [sum lgamma(y + 1), sum y, sum e^o, rows with y < 0 or a non-finite y / o] of n rows (off nullable);
// cpart: 4 * POIS_CONST_BLOCKS doubles of scratch
int pois_const(const double* y, const double* off, int64_t n, double* cpart, double* cst, hipStream_t s);
// ll[0] = cst[3] > 0 ? NaN : ll[0] - cst[0]: the pass entries' full log-likelihood
int pois_ll_fix(double* ll, const double* cst, hipStream_t s);
// out[j] = v[first + j * step], j < n: a strided partition's counts or offsets, gathered once (8 bytes per row)
int pois_gather(const double* v, int64_t first, int64_t step, int64_t n, double* out, hipStream_t s);
// the Newton start of the log-link fits: beta = 0, entry icpt_col (-1: none) at b0
int pois_start(double* beta, int pe, int icpt_col, double b0, hipStream_t s);
// yk / ok = the n > 0 responses and offsets (nullable) of the partition rows first, first + step, ...: in place when step == 1,
// else gathered into ybuf / obuf
static inline int pois_gather_rows(const double* y, const double* offset, int64_t first, int64_t step, int64_t n, double* ybuf,
                                   double* obuf, const double*& yk, const double*& ok, hipStream_t s) {
    yk = y + first;
    ok = offset ? offset + first : nullptr;
    if (step <= 1) return DLSA_OK;
    int rc = pois_gather(y, first, step, n, ybuf, s);
    if (rc) return rc;
    yk = ybuf;
    if (offset) {
        rc = pois_gather(offset, first, step, n, obuf, s);
        if (rc) return rc;
        ok = obuf;
    }
    return DLSA_OK;
}

// device scratch of the fit loop
struct PoisFitBufs {
    double* cpart;     // 4 * POIS_CONST_BLOCKS
    double* cst;       // 4
    double* ybuf;      // max_rows when row_step > 1: the gathered counts
    double* obuf;      // max_rows when row_step > 1 and offsets are given
    NewtonState st;
};

// "evaluate (H, g, sum y eta - mu) at beta for partition k": yk / ok (nullable) are the partition's nk > 0 counts and offsets,
// contiguous (gathered when the partition is strided); H is pe x pe (ldh = pe, both triangles), g pe, ll one device double
using PoisEval = std::function<int(int k, const double* yk, const double* ok, int64_t nk, const double* beta, double* H,
                                   double* g, double* ll)>;

// The per-partition driver of the Poisson fits: data check and constant term, start at beta = 0 with entry icpt_col (-1: none)
// at log(sum y / sum e^o), then newton_fit_loop with the policy NEWTON_POISSON and newton_fit_finish (Sig_inv = H at the returned
// coef, EMPTY + zero block without rows or events).  `who` prefixes messages.
int pois_fit_core(const char* who, const double* y, const double* offset, const int64_t* part_first_host,
                  const int64_t* part_rows_host, int64_t row_step, int K, int pe, int icpt_col, double tol, int max_iter,
                  double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                  const PoisFitBufs& b, const PoisEval& eval, hipStream_t s);

// ---- onehot_poisson.hip ------------------------------------------------------------------------------------------------
// One partition at a fixed beta on the raw representation: H (nullable) needs w (mu per row); g, loglik (the sum of y eta - mu)
// nullable.  ws_oh: the structured passes' arena (256-aligned, >= onehot_workspace_bytes_impl(pl, n)).
int oh_pois_pass_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc, const double* y,
                      const double* off, const double* beta, int64_t n, double* H, int64_t ldh, double* g, double* loglik, double* w,
                      void* ws_oh, size_t ws_oh_bytes, hipStream_t s);
// num / codes against what the plan reads (null pointers, ldn, ldc); `who` prefixes the message
int oh_pois_check_rows(const char* who, const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc);
// the plan's constant column (where the intercept's start value goes), -1 without one
int oh_pois_icpt_col(const dlsa_onehot_plan* pl);

}  // namespace dlsa
