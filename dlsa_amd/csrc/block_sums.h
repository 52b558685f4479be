// The per-block sums of the log-link families (Poisson's constant sums, the once-per-partition and dispersion sums of Gamma and
// Tweedie): the tail every such sum kernel ends in and the fixed-order finish of its block partials.  A header of its own, not
// common.h: common.h is one of the Gram sources whose hash ties profiles/pmc_latest.json to the tree, and nothing here concerns
// the Gram.
#pragma once
#include "common.h"

namespace dlsa {

#if defined(__HIPCC__)
// The tail of a sum kernel of 256 threads that holds NQ running sums per thread: part[block * NQ + j] = the block's sum of acc[j],
// each wave's all-reduce first, then the four wave sums added in the order 0..3 -- a fixed order, bit-reproducible.
template <int NQ>
__device__ __forceinline__ void block_partials_store(const double (&acc)[NQ], double* __restrict__ part) {
    __shared__ double red[4][NQ];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const double t = wave_allreduce_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) red[wave][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) t += red[k][threadIdx.x];
        part[(int64_t)blockIdx.x * NQ + threadIdx.x] = t;
    }
}
#endif

// out[j] = the sum over b < nblocks of part[b * nq + j], j < nq <= 4, in a fixed order (one wave per quantity): the finish of
// the kernels that end in block_partials_store.  The kernel is poisson.hip's, next to the other launchers the families share.
int block_sum_finish(const double* part, int nblocks, int nq, double* out, hipStream_t s);

}  // namespace dlsa
