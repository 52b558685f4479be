// LARS path with u >= 2 leading unpenalised coefficients (dlsa_lars_lsa_f64, `intercept` = u): the two small kernels round the path
// kernel.  The reference removes ONE unpenalised coefficient by a scalar Schur complement (lars_lsa(intercept=True), dlsa/lsa.py:98-104,
// and beta0 at :203-205); this is the same elimination for a block.  With A11 = Sigma0[:u,:u] = L L', A12 = Sigma0[:u,u:] and
// V = L^{-1} A12:
//   reduced matrix   A22 - A12' A11^{-1} A12 = A22 - V'V     (the path kernels' prologues subtract V'V: lars.h, lars_unpen_term)
//   beta0_k          A11^{-1} A12 (b - beta_k) = L^{-T} (V (b - beta_k))
// prepare: one workgroup; L in LDS (u <= 32: 8 KB), every thread solves whole columns of V in registers.
// finish:  up to 256 workgroups, each refactors A11 (the same instructions on the same numbers: the same L) and takes the path rows
//          k = blockIdx.x, + gridDim.x, ...: u dot products of length m (one wave each, fixed order), then one back substitution.
#include "common.h"
#include "lars.h"
#include <math.h>

namespace dlsa {
namespace {

constexpr int UMAX = DLSA_LARS_MAX_UNPENALIZED;
constexpr int UT = 256;                       // threads of both kernels
static_assert(UMAX == 32, "the column solve below is unrolled for 32 rows");

// Lower Cholesky factor of A (u x u, lower triangle read) into L (LDS, row pitch UMAX), right-looking.  Returns -1, or the index of
// the first pivot that is not positive: at most u 2^-50 times its diagonal entry -- a pivot of a singular block is a sum of at most u
// products bounded by that entry, so it carries up to ~u 2^-53 of it in rounding error, of either sign; eight times that is taken
// for zero -- or not finite.  The same value in every thread.
__device__ int chol_lower_lds(const double* __restrict__ A, int64_t lda, int u, double* L) {
    const int tid = threadIdx.x;
    for (int e = tid; e < u * u; e += UT) {
        const int r = e / u, c = e - r * u;
        L[r * UMAX + c] = c <= r ? A[(int64_t)r * lda + c] : 0.0;
    }
    __syncthreads();
    const double tol = (double)u * 0x1p-50;
    for (int k = 0; k < u; ++k) {
        const double d = L[k * UMAX + k], akk = A[(int64_t)k * lda + k];
        if (!(d > tol * akk) || !isfinite(d)) return k;
        __syncthreads();
        const double rk = sqrt(d);
        if (tid == 0) L[k * UMAX + k] = rk;
        for (int r = k + 1 + tid; r < u; r += UT) L[r * UMAX + k] /= rk;
        __syncthreads();
        const int w = u - k - 1;              // trailing block (k, u) x (k, u), lower part
        for (int e = tid; e < w * w; e += UT) {
            const int r = k + 1 + e / w, c = k + 1 + e % w;
            if (c <= r) L[r * UMAX + c] = fma(-L[r * UMAX + k], L[c * UMAX + k], L[r * UMAX + c]);
        }
        __syncthreads();
    }
    return -1;
}

__global__ __launch_bounds__(UT) void lars_unpen_prepare_kernel(LarsArgs a) {
    __shared__ double L[UMAX * UMAX];
    const int tid = threadIdx.x;
    const int u = a.unpen, m = a.p - u, ld = (m + 1) & ~1;
    const int bad = chol_lower_lds(a.Sigma0, a.lds0, u, L);
    if (tid == 0) { a.n_steps[0] = 0; a.n_steps[1] = bad + 1; }
    if (bad >= 0) return;
    double* __restrict__ V = const_cast<double*>(a.V);
    for (int j = tid; j < ld; j += UT) {      // column j of V = L^{-1} A12 by forward substitution; the pad column is zero
        double v[UMAX];
#pragma unroll
        for (int r = 0; r < UMAX; ++r) {
            if (r < u) {
                double s = j < m ? a.Sigma0[(int64_t)r * a.lds0 + u + j] : 0.0;
#pragma unroll
                for (int q = 0; q < r; ++q) s = fma(-L[r * UMAX + q], v[q], s);
                v[r] = s / L[r * UMAX + r];
                V[(int64_t)r * ld + j] = v[r];
            }
        }
    }
}

__global__ __launch_bounds__(UT) void lars_unpen_finish_kernel(LarsArgs a, int rows) {
    __shared__ double L[UMAX * UMAX];
    __shared__ double t[UMAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int u = a.unpen, m = a.p - u, ld = (m + 1) & ~1;
    if (chol_lower_lds(a.Sigma0, a.lds0, u, L) >= 0) return;      // (the prepare kernel passed: not taken)
    for (int k = blockIdx.x; k < rows; k += gridDim.x) {
        const double* __restrict__ bk = a.beta_path + (int64_t)k * m;
        for (int r = wave; r < u; r += UT / 64) {
            const double* __restrict__ vr = a.V + (int64_t)r * ld;
            double s = 0.0;
            for (int j = lane; j < m; j += 64) s = fma(vr[j], a.b0[u + j] - bk[j], s);
            s = wave_allreduce_sum(s);
            if (lane == 0) t[r] = s;
        }
        __syncthreads();
        if (tid == 0) {                       // L' x = t, in place
            for (int r = u - 1; r >= 0; --r) {
                double x = t[r];
                for (int q = r + 1; q < u; ++q) x = fma(-L[q * UMAX + r], t[q], x);
                x /= L[r * UMAX + r];
                t[r] = x;
                a.beta0[(int64_t)k * u + r] = x;
            }
        }
        __syncthreads();
    }
}

}  // namespace

int lars_unpen_prepare(const LarsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(lars_unpen_prepare_kernel, dim3(1), dim3(UT), 0, s, a);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int lars_unpen_finish(const LarsArgs& a, int rows, hipStream_t s) {
    if (rows <= 0) return DLSA_OK;
    hipLaunchKernelGGL(lars_unpen_finish_kernel, dim3(rows < 256 ? rows : 256), dim3(UT), 0, s, a, rows);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

}  // namespace dlsa
