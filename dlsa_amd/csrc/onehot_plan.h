// The structured one-hot plan (OhDesc, OhRole, OhTable, dlsa_onehot_plan), the sizing rules and small device helpers of its row
// passes, and the host functions of onehot.hip that other translation units call.  Included by onehot.hip (the logistic row
// pass, the Gram, plan creation), onehot_poisson.hip (the Poisson row pass) and irls.hip (the structured logistic fit); the
// row-pass kernel and its launch driver are onehot_pass.h.
#pragma once
#include "common.h"
#include <vector>
#include <algorithm>

namespace dlsa {

constexpr int OH_MAXD = 8;            // dense columns (intercept + numerics) handled in registers
constexpr int OH_MAXF = 8;            // factors
constexpr int OH_THREADS = 256;
constexpr int OH_LOGIT_REP = 8;             // LDS copies (at most) of the logit pass's residual histogram
// copies actually used: as many as keep the workgroup's LDS near 32 KB (several workgroups per CU), at least one
static int oh_logit_rep(int p) {
    int r = OH_LOGIT_REP;
    while (r > 1 && (size_t)(1 + r) * p * sizeof(double) > 32 * 1024) r /= 2;
    return r;
}

struct OhTable {                      // one factor-pair table of a Gram role (t <= u; t == u: the diagonal counts), or a BAND of its rows
    int t, u;                         // factor indices
    int lds_off;                      // offset (doubles) of its ltn x L_u (or ltn) cells in the role's LDS image
    int lt0, ltn;                     // the levels lt0 .. lt0 + ltn - 1 of factor t: a table larger than the LDS budget is cut into
                                      // row bands that go to different roles (300 x 300 levels: five bands of 64 rows)
};

struct OhRole {
    int ntab;
    OhTable tab[OH_MAXF * (OH_MAXF + 1) / 2];
    int with_dense;                   // this role also accumulates H_DD and H_D,dummy
    int dense_off;                    // offset of the D x nlev_total block (H_D,dummy), if with_dense
    int cells;                        // doubles in the LDS image (and in the role's partial)
    int dense_rep;                    // copies of the H_D,dummy block in LDS (copy r >= 1 sits after the image, at
                                      // cells + (r-1) * nlev_total * OH_MAXD): lanes spread over them, so the lanes of a
                                      // wave that share a hot level do not all serialise on the same eight addresses
};

struct OhDesc {                       // device-visible description of the design
    int p, D, f;
    int dense_kind[OH_MAXD];          // 0: constant 1, 1: numeric column dense_src
    int dense_src[OH_MAXD];
    double dense_shift[OH_MAXD], dense_scale[OH_MAXD];
    int dense_col[OH_MAXD];           // output column of dense column a
    int lvl_off[OH_MAXF + 1];         // factor t's levels occupy [lvl_off[t], lvl_off[t+1]) of level_col
    int nlev_total;
    int dbg;                          // DLSA_OH_DBG (timing experiments only, wrong results): 1 = no dense x level atomics, 2 = no pair-table atomics
    int ordered;                      // LDS accumulation of the passes.  2 (default, Gram): EXACT -- every addend goes in as a 64-bit
                                      // fixed-point integer (ds_add_u64), integer addition is associative, so all waves add at once
                                      // and the result is bit-identical from run to run whatever the order; 1: floating-point adds in
                                      // a fixed wave order (turn-taking in the logit pass, the systolic schedule in the Gram;
                                      // DLSA_OH_ORDERED=1, and the Gram's fall-back when an addend leaves the fixed-point range);
                                      // 0 (DLSA_OH_ORDERED=0): floating-point adds from all waves at once, last bits vary
    int* overflow;                    // exact mode: set to 1 by a thread whose addend exceeds OH_FIX_VMAX (or is not finite)
};

}  // namespace dlsa

struct dlsa_onehot_plan {
    dlsa::OhDesc desc;
    int32_t* d_level_col;             // device: column of every (factor, level), -1 = no column (baseline / dropped)
    std::vector<int32_t> h_level_col;
    std::vector<dlsa::OhRole> roles;
    dlsa::OhRole* d_roles;
    bool needs_num;                   // some dense column is numeric
};

namespace dlsa {

// standardised dense vector of row i (d[a], a < D)
__device__ __forceinline__ void oh_dense_row(const OhDesc& ds, const double* __restrict__ num, int64_t ldn, int64_t i,
                                             double (&d)[OH_MAXD]) {
#pragma unroll
    for (int a = 0; a < OH_MAXD; ++a) {
        d[a] = 0.0;
        if (a < ds.D) d[a] = ds.dense_kind[a] == 0 ? 1.0 : (num[i * ldn + ds.dense_src[a]] - ds.dense_shift[a]) / ds.dense_scale[a];
    }
}

__device__ __forceinline__ double oh_block_sum(double v, double* red) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += red[k];
    return s;
}

// The logit pass keeps little in LDS, so many small workgroups share a CU: four rows per thread, up to eight
// workgroups per CU (a 1e6-row partition: 977 workgroups instead of 244 -- one per CU, four waves, nothing to hide the
// row loads behind: 72 us for 76 MB)
constexpr int OH_LOGIT_MAX_BLOCKS = 2048;
static int oh_logit_blocks(int64_t n) {
    const int64_t want = (n + OH_THREADS * 4 - 1) / (OH_THREADS * 4);
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, OH_LOGIT_MAX_BLOCKS));
}

// g[j] = sum_b gpart[b][j], loglik = sum_b llpart[b] in a fixed order: the dense pass's finish kernel (logit.hip)
void logit_finish_launch(const double* gpart, const double* llpart, int nblocks, int pitch, int p, double* g,
                         double* loglik, hipStream_t stream, const double* s0part, double* s0);
// onehot.hip
int onehot_plan_p(const dlsa_onehot_plan* pl);
size_t onehot_workspace_bytes_impl(const dlsa_onehot_plan* pl, int64_t n);
int onehot_logit_pass_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                           const double* y, const double* beta, int64_t n, double* w_out, double* g, double* loglik,
                           void* ws, size_t ws_bytes, hipStream_t s);
int onehot_gram_impl(const dlsa_onehot_plan* pl, const double* num, int64_t ldn, const int32_t* codes, int64_t ldc,
                     const double* w, int64_t n, double* H, int64_t ldh, void* ws, size_t ws_bytes, hipStream_t s, bool irls_weights);

}  // namespace dlsa
