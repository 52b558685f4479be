// Arguments and workspace of the LARS path kernels (lars.hip: R^{-1} form, one workgroup or a grid; lars_q.hip: carried
// Cholesky rows, one workgroup).  Reference: lars_lsa, dlsa/lsa.py:90-212.
#pragma once
#include "common.h"
#include <mutex>

namespace dlsa {

struct LarsArgs {
    const double* Sigma0;   // p x p
    const double* b0;       // p
    int64_t lds0;
    int p, intercept, type, max_steps;   // intercept: 1 when exactly ONE leading coefficient is unpenalised (the scalar Schur complement), else 0
    int unpen;        // u, the number of leading unpenalised coefficients (m = p - u); u >= 2: the kernels subtract V'V instead
    const double* V;  // u >= 2: u x ld, L^{-1} Sigma0[:u, u:] with L the Cholesky factor of Sigma0[:u,:u] (lars_unpen.hip; pad column zero)
    double n, eps;
    // workspace
    double* S;        // m x ld scaled Sigma (ld = m rounded up to even; the pad column is zero)
    double* Rinv;     // m x ld upper triangular inverse factor (active order), rows
    double* RinvT;    // m x ld its transpose, rows
    double* vec;      // 12 vectors of length m (see kernel)
    int* ivec;        // 4 int vectors of length m
    // outputs
    double* beta_path; double* beta0; double* aic; double* bic;
    int* n_steps;     // device scalar; u >= 2: n_steps[1] is the prepare kernel's flag (0, or 1 + the index of the bad pivot of A11)
    // multi-workgroup kernel only
    double* rbuf;     // m: r = R^{-T} x of the current append, gathered from the row owners
    double* wbuf;     // m: equiangular weights, gathered from the row owners
    double* upart;    // G x ld: per-workgroup partial sums of Sigma[:,active] w
    unsigned* bar;    // grid barrier: [0] arrival counter, [1] abort word (both zero at launch)
    long long bar_timeout;   // ticks of the 100 MHz wall clock a workgroup waits at a grid barrier before it aborts the launch
    int nwg;          // lars_q.hip: workgroups sharing the rows of the fused pass (1: none)
};

extern std::mutex g_lars_grid_mu;      // lars.hip: serialises this process's multi-workgroup path launches (launch .. completion)

// In the functions below `intercept` is the COUNT u of leading unpenalised coefficients and m = p - u.  Which kernel takes a width
// is decided by m; lars.hip's own choices (workgroups, 512 / 1024 threads) are keyed as before u >= 2 existed, by m + (u ? 1 : 0).
inline int lars_keyed_p(int p, int intercept) { return p - intercept + (intercept ? 1 : 0); }

// lars_unpen.hip: u >= 2.  prepare: one workgroup, writes a.V and the flag a.n_steps[1] (and zeroes a.n_steps[0]); the path kernels
// leave at once when the flag is set.  finish: a.beta0[k][r] for k <= *a.n_steps from a.beta_path (nothing when *a.n_steps < 0).
int lars_unpen_prepare(const LarsArgs& a, hipStream_t s);
int lars_unpen_finish(const LarsArgs& a, int rows, hipStream_t s);
#if defined(__HIPCC__)
// The term the prologues subtract from Sigma0[u + i][u + j] when u >= 2: (V'V)[i][j] = sum_r V[r][i] V[r][j], in the fixed order
// r = 0 .. u - 1.  The path kernels read rows of S for columns, so S must be symmetric TO THE BIT: a product commutes, also inside an
// fma, so (i, j) and (j, i) give the same bits -- which A12' (A11^-1 A12) would not.  V is read from global memory (u m doubles,
// L2-resident; m^2 u loads once per call).
__device__ __forceinline__ double lars_unpen_term(const double* __restrict__ V, int ld, int u, int i, int j) {
    double s = 0.0;
    for (int r = 0; r < u; ++r) s = fma(V[(int64_t)r * ld + i], V[(int64_t)r * ld + j], s);
    return s;
}
#endif

// lars_q.hip: the path kernel for narrow problems (m = p - intercept <= LARS_Q_MAX_M)
constexpr int LARS_Q_MAX_M = 1020;
bool lars_q_eligible(int p, int intercept);
// returns DLSA_OK with *aborted = 1 when a clustered launch gave up at its barrier (nothing usable was written: run again with max_wgs = 1)
int lars_q_run(LarsArgs& a, int p, int intercept, hipStream_t s, int max_wgs, int* wgs_used);

// lars_c.hip (round 6): the same carried rows for WIDE problems (LARS_C_MIN_M < m <= LARS_C_MAX_M), the fused pass split by COLUMNS over
// up to LARS_C_MAX_WGS workgroups that meet at one bounded grid barrier per append; *n_steps = -1 when a barrier gave up (the caller
// reruns the path on lars.hip's single-workgroup kernel)
constexpr int LARS_C_MAX_M = 2044, LARS_C_MAX_WGS = 64;
constexpr int LARS_C_MIN_M = 448;                   // narrower problems: lars_q.hip (same box, lasso paths, lars_q.hip / lars_c.hip: p = 400 3.70 / 3.59 ms, 500 5.10 / 4.61,
                                                    // 640 9.31 / 6.26, 1020 20.8 / 12.1: profiles/r06_lars_column_split.txt)
bool lars_c_eligible(int p, int intercept);
int lars_c_run(LarsArgs& a, int p, int intercept, hipStream_t s, int* wgs_used);

}  // namespace dlsa
