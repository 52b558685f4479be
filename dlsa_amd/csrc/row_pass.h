// The skeleton of the dense row passes that read X once in rowdot.h's layout (lane l holds the columns 128c + 2l + {0,1} of the
// RB rows of a wave's batch): count_pass_kernel (count_pass.h), mn_pass_kernel (multinomial.hip) and ord_pass_kernel (ordinal.hip)
// are written on it.  Device side: the batch load, the batch loop and the block reduction; host side: the chunk count, the rows
// per batch, the block count, the predicate of the 16-byte loads and the nc -> <NC, RB> dispatcher.  What a row contributes is
// the kernel's own.  Included inside namespace dlsa after rowdot.h; the library is built without relocatable device code, so a
// kernel is instantiated in the file that launches it.
#pragma once

typedef double count_d2v __attribute__((ext_vector_type(2)));

constexpr int COUNT_THREADS = 256;
constexpr int COUNT_WAVES = COUNT_THREADS / 64;
constexpr int COUNT_MAX_BLOCKS = 2048;

static __device__ __forceinline__ double2 count_ld2(const double* ptr) {
    const count_d2v t = __builtin_nontemporal_load(reinterpret_cast<const count_d2v*>(ptr));
    double2 r; r.x = t.x; r.y = t.y; return r;
}

// The X tile of batch bt: branch-free, rows past n read row n - 1 and columns past p read column 0 (they meet beta = 0 and a
// residual of 0).  Returns the clamped index of the lane's own row (myrow = row_of_lane<RB>(lane)), where the kernel loads the
// row's scalars.
template <int NC, int RB, bool VEC>
__device__ __forceinline__ int64_t row_pass_load(const double* X, int64_t ldx, int64_t n, int p, int64_t bt, int lane, int myrow,
                                                 double2 (&x)[RB][NC]) {
    const int64_t row0 = bt * RB;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int64_t r = min(row0 + i, n - 1);
        const double* rowp = X + r * ldx;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = c * 128 + 2 * lane;
            const int c0 = col < p ? col : 0;
            if (VEC) {                                            // VEC implies p even: a pair never straddles p
                x[i][c] = count_ld2(rowp + c0);
            } else {
                x[i][c].x = __builtin_nontemporal_load(rowp + c0);
                x[i][c].y = __builtin_nontemporal_load(rowp + (col + 1 < p ? col + 1 : 0));
            }
        }
    }
    return min(row0 + myrow, n - 1);
}

// The batches of this wave, COUNT_WAVES * gridDim.x apart: load(bt, x, s) fills the tile and the kernel's per-row scalars S,
// process(bt, x, s) consumes them.  At NC = 1 a second register set prefetches the next batch.
template <int NC, int RB, class S, class Load, class Process>
__device__ __forceinline__ void row_pass_stream(int64_t n, int wave, Load&& load, Process&& process) {
    const int64_t nbatch = (n + RB - 1) / RB;
    const int64_t stride = (int64_t)gridDim.x * COUNT_WAVES;
    int64_t bt = (int64_t)blockIdx.x * COUNT_WAVES + wave;
    if constexpr (NC == 1) {
        double2 xa[RB][NC], xb[RB][NC];
        S sa{}, sb{};
        if (n > 0) {
            load(bt, xa, sa);
            for (; bt < nbatch; bt += 2 * stride) {
                const int64_t b1 = bt + stride, b2 = bt + 2 * stride;
                load(b1, xb, sb);
                process(bt, xa, sa);
                load(b2, xa, sa);
                if (b1 < nbatch) process(b1, xb, sb);
            }
        }
    } else {
        for (; bt < nbatch; bt += stride) {
            double2 x[RB][NC];
            S s;
            load(bt, x, s);
            process(bt, x, s);
        }
    }
}

// Block reduction: the waves add into LDS one after another, wave 0 first (a fixed order: results are reproducible).
// sh[(k * NC + c) * 128 + 2 lane + {0,1}] = the sum of g[k][c], sh[SETS * NC * 128 + i] = the sum of sc[i] over the block's lanes.
template <int SETS, int NC, int NSC>
__device__ __forceinline__ void row_pass_reduce(const double2 (&g)[SETS][NC], double (&sc)[NSC], double* sh, int lane, int wave) {
#pragma unroll
    for (int i = 0; i < NSC; ++i) sc[i] = wave_allreduce_sum(sc[i]);
    for (int wv = 0; wv < COUNT_WAVES; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int k = 0; k < SETS; ++k) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    double* dst = sh + (k * NC + c) * 128 + 2 * lane;
                    if (wv == 0) { dst[0] = g[k][c].x; dst[1] = g[k][c].y; }
                    else { dst[0] += g[k][c].x; dst[1] += g[k][c].y; }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < NSC; ++i) {
                    if (wv == 0) sh[SETS * NC * 128 + i] = sc[i]; else sh[SETS * NC * 128 + i] += sc[i];
                }
            }
        }
        __syncthreads();
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int count_nc(int p) {
    const int chunks = (p + 127) / 128;
    int nc = 1;
    while (nc < chunks) nc *= 2;
    return nc;
}

constexpr int count_rb(int nc) { return nc <= 2 ? 8 : nc == 4 ? 4 : nc == 8 ? 2 : 1; }

static int count_blocks(int64_t n, int rb) {
    const int64_t nbatch = (n + rb - 1) / rb;
    int64_t blocks = (nbatch + COUNT_WAVES * 4 - 1) / (COUNT_WAVES * 4);   // >= 4 batches per wave
    return (int)std::min<int64_t>(std::max<int64_t>(blocks, 1), COUNT_MAX_BLOCKS);
}

// the 16-byte loads: every pair of a row starts at a multiple of 16 bytes and none straddles p
static bool row_pass_vec(const double* X, int64_t ldx, int p) { return (ldx % 2 == 0) && (p % 2 == 0) && (((uintptr_t)X & 15) == 0); }

template <int NC_>
struct RowShape { static constexpr int NC = NC_, RB = count_rb(NC_); };

// f(RowShape<NC>{}) for nc = count_nc(p) chunks
template <class F>
static auto row_pass_dispatch(int nc, F&& f) {
    switch (nc) {
        case 1: return f(RowShape<1>{});
        case 2: return f(RowShape<2>{});
        case 4: return f(RowShape<4>{});
        case 8: return f(RowShape<8>{});
        default: return f(RowShape<16>{});
    }
}
