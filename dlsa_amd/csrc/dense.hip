// Small dense fp64 pieces that sit between the big passes: the Sig_inv . coef product
// (dlsa/models.py:131), the local block sum that feeds the one-round all-reduce (dlsa/dlsa.py:30-34)
// and the C entry of the WLS combine (dlsa.py:48-49; the blocked Cholesky itself is chol.hip).
#include "common.h"
#include "host_calls.h"

namespace dlsa {

// y = A x   (A p x p row-major, one wave per row)
__global__ void matvec_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ x,
                              int p, double* __restrict__ y) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= p) return;
    double s = 0.0;
    for (int k = lane; k < p; k += 64) s = fma(A[(int64_t)row * lda + k], x[k], s);
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) y[row] = s;
}

// out = a + s * b
__global__ void axpby_kernel(const double* a, const double* b, double s,
                             int n, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + s * b[i];
}

// the end of a Newton iteration in one launch: prev = beta, beta = beta + delta
__global__ void advance_kernel(double* __restrict__ prev, double* __restrict__ beta, const double* __restrict__ delta, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const double b = beta[i]; prev[i] = b; beta[i] = b + 1.0 * delta[i]; }
}

// out[e] = sum over included k of in[k*stride + e]   (fixed order)
__global__ void sum_blocks_kernel(const double* __restrict__ in, int64_t stride, int K,
                                  const int* __restrict__ mask, int64_t count, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    double s = 0.0;
    for (int k = 0; k < K; ++k)
        if (!mask || mask[k] == 0) s += in[k * stride + e];
    out[e] = s;
}

// y = alpha * A x + beta * z   (A p x p row-major, one wave per row; z nullable; y may be z)
__global__ void matvec_axpy_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ x, int p, double alpha,
                                   const double* z, double beta, double* y) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= p) return;
    double s0 = 0.0, s1 = 0.0;
    const double* a = A + (int64_t)row * lda;
    int k = lane;
    for (; k + 64 < p; k += 128) { s0 = fma(a[k], x[k], s0); s1 = fma(a[k + 64], x[k + 64], s1); }
    if (k < p) s0 = fma(a[k], x[k], s0);
    double s = s0 + s1;
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) y[row] = z ? fma(alpha, s, beta * z[row]) : alpha * s;
}

// stats[0] = |delta|_inf, stats[1] = |ref|_inf, stats[2] = 2 when delta holds a non-finite value, else 0 (the step statistics the
// Cholesky solve kernels leave, for steps that come from elsewhere)
__global__ __launch_bounds__(1024) void step_stats_kernel(const double* __restrict__ delta, const double* __restrict__ ref, int p,
                                                          double* __restrict__ stats) {
    __shared__ double red[3][16];
    double mx = 0.0, mr = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < p; i += blockDim.x) {
        const double v = delta[i];
        mx = fmax(mx, fabs(v));
        if (!isfinite(v)) bad = 1.0;
        mr = fmax(mr, fabs(ref[i]));
    }
    for (int m = 32; m >= 1; m >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, m, 64));
        mr = fmax(mr, __shfl_xor(mr, m, 64));
        bad = fmax(bad, __shfl_xor(bad, m, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mx; red[1][threadIdx.x >> 6] = mr; red[2][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { a = fmax(a, red[0][k]); b = fmax(b, red[1][k]); c = fmax(c, red[2][k]); }
        stats[0] = a; stats[1] = b; stats[2] = c != 0.0 ? 2.0 : 0.0;
    }
}

int launch_matvec(const double* A, int64_t lda, const double* x, int p, double* y, hipStream_t s) {
    hipLaunchKernelGGL(matvec_kernel, dim3((p + 3) / 4), dim3(256), 0, s, A, lda, x, p, y);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int launch_matvec_axpy(const double* A, int64_t lda, const double* x, int p, double alpha, const double* z, double beta, double* y, hipStream_t s) {
    hipLaunchKernelGGL(matvec_axpy_kernel, dim3((p + 3) / 4), dim3(256), 0, s, A, lda, x, p, alpha, z, beta, y);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int launch_step_stats(const double* delta, const double* ref, int p, double* stats, hipStream_t s) {
    hipLaunchKernelGGL(step_stats_kernel, dim3(1), dim3(1024), 0, s, delta, ref, p, stats);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int launch_advance(double* prev, double* beta, const double* delta, int n, hipStream_t s) {
    hipLaunchKernelGGL(advance_kernel, dim3((n + 255) / 256), dim3(256), 0, s, prev, beta, delta, n);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

int launch_axpby(const double* a, const double* b, double sc, int n, double* out, hipStream_t s) {
    hipLaunchKernelGGL(axpby_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, b, sc, n, out);
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_solve_workspace_bytes(int p) {
    if (p <= 0) return 0;
    return dlsa::align_up((size_t)p * p * sizeof(double), 256) + 256 + 256;
}

int dlsa_spd_solve_f64(const double* S, int64_t lds, const double* v, int p, double* theta,
                       void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(S && v && theta, "spd_solve: null argument");
    DLSA_REQUIRE(p > 0 && lds >= p, "spd_solve: bad shape p=%d lds=%lld", p, (long long)lds);
    if (!ws || ws_bytes < dlsa_solve_workspace_bytes(p) || ((uintptr_t)ws & 255)) {
        set_error("spd_solve: workspace %zu bytes needed (256-aligned), got %zu", dlsa_solve_workspace_bytes(p), ws_bytes);
        return DLSA_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    Arena ar(ws, ws_bytes);
    double* L = (double*)ar.take((size_t)p * p * sizeof(double));
    double* stats = (double*)ar.take(4 * sizeof(double));
    int rc = launch_chol_solve(S, lds, 0, v, 0, nullptr, 0, p, 1, L, theta, 0, stats, 0, s, 0);
    if (rc) return rc;
    double h[3];
    DLSA_HIP_CHECK(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, s));
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    if (h[2] == 1.0) { set_error("spd_solve: matrix is not positive definite"); return DLSA_ERR_NOT_SPD; }
    if (h[2] == 2.0) { set_error("spd_solve: NaN/Inf in the system"); return DLSA_ERR_NAN; }
    return DLSA_OK;
}

int dlsa_sum_blocks_f64(const double* coef, const double* Sig_inv, const double* Sig_invMcoef, int K, int p,
                        const int* mask_host, double* out, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(coef && Sig_inv && Sig_invMcoef && out, "sum_blocks: null argument");
    DLSA_REQUIRE(K > 0 && p > 0, "sum_blocks: bad K=%d p=%d", K, p);
    hipStream_t s = (hipStream_t)stream;
    int* dmask = nullptr;
    if (mask_host) {
        bool any = false;
        for (int k = 0; k < K; ++k) any |= (mask_host[k] != 0);
        if (any) {
            // the mask rides in the tail of `out`'s own message?  no: keep it simple and exact --
            // a K-int scratch is allocated stream-ordered and released before return.
            DLSA_HIP_CHECK(hipMallocAsync((void**)&dmask, (size_t)K * sizeof(int), s));
            DLSA_HIP_CHECK(hipMemcpyAsync(dmask, mask_host, (size_t)K * sizeof(int), hipMemcpyHostToDevice, s));
        }
    }
    const int64_t pp = (int64_t)p * p;
    hipLaunchKernelGGL(sum_blocks_kernel, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, s, Sig_inv, pp, K, dmask, pp, out);
    hipLaunchKernelGGL(sum_blocks_kernel, dim3((p + 255) / 256), dim3(256), 0, s, Sig_invMcoef, (int64_t)p, K, dmask, (int64_t)p, out + pp);
    hipLaunchKernelGGL(sum_blocks_kernel, dim3((p + 255) / 256), dim3(256), 0, s, coef, (int64_t)p, K, dmask, (int64_t)p, out + pp + p);
    DLSA_HIP_CHECK(hipGetLastError());
    if (dmask) {
        DLSA_HIP_CHECK(hipStreamSynchronize(s));   // mask_host must stay valid until the copy is done
        DLSA_HIP_CHECK(hipFreeAsync(dmask, s));
    }
    return DLSA_OK;
}

}  // extern "C"
