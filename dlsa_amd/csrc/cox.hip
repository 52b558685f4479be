// Cox proportional-hazards map step (Breslow or Efron ties): one partition's log partial likelihood, score and observed information
// at a fixed beta, and the per-partition Newton fit on top of it.  The local objective of a partition is its own partial
// likelihood with risk sets taken inside the partition (a Cox model stratified by partition with a common beta); the blocks
// it returns (coef, Sig_inv = observed information at coef, Sig_inv coef) feed the unchanged one-round combine.
//
// Algebra (one partition, rows in DESCENDING time through the caller's permutation `order`; eta_j = x_j' beta; tie groups
// are runs of equal time; group i has d_i events and ends at position e_i):
//   S0_i = sum_{pos <= e_i} exp(eta),  S1_i = sum_{pos <= e_i} exp(eta) x,  a_i = S1_i / S0_i         (forward prefix)
//   loglik = sum_events eta - sum_i d_i log S0_i,   U = X' delta - A' d
//   H = X' diag(w) X - A' diag(d) A,  w_j = exp(eta_j) c_j,  c_j = sum_{i : e_i >= pos(j)} d_i / S0_i  (suffix over groups)
// so H is two weighted Grams on the existing MFMA kernels (X in its own row layout, and the D event rows of A) and no
// p x p work per event.
//
// Efron's approximation (ties = DLSA_COX_TIES_EFRON; every kernel below carries it as the instantiation EF, the Breslow
// instantiation is the code above): T0_i, T1_i are the sums of S0_i, S1_i over the EVENT rows of group i only,
// f_l = l / d_i, phi_il = S0_i - f_l T0_i for l = 0 .. d_i - 1, and
//   loglik = sum_events eta - sum_i sum_l log phi_il
//   U = X' delta - sum_i (h1_i S1_i - h2_i T1_i),            h1_i = sum_l 1 / phi_il, h2_i = sum_l f_l / phi_il
//   H = X' diag(w) X - sum_i [S1_i T1_i] K_i [S1_i T1_i]',   K_i = [[k0, -k1], [-k1, k2]], k_m = sum_l f_l^m / phi_il^2
//   w_j = exp(eta_j) (c_j - delta_j h2_g(j)),                c_j = sum_{i : e_i >= pos(j)} h1_i
// With the 2 x 2 Cholesky factor K = L L' a group gives the A rows L11 S1 + L21 T1 and (d_i >= 2) L22 T1, both of weight
// -1, so H stays two weighted Grams.  d_i = 1 gives k1 = k2 = 0 and Breslow's terms.  A group end costs O(p) vector work
// and the scalar sums over l, which the wave's 64 lanes share (lane t takes l = t, t + 64, ..; one fixed butterfly).
//
// Passes (every partial combines in a fixed order: no float atomics, no waits between workgroups inside a launch):
//   1 cox_eta_kernel      one wave per segment of L consecutive positions: eta (written per position), the segment's
//                         max eta M and sums of exp(eta - M) [1, x], and the tie-group bookkeeping of the segment;
//   2 cox_segscan_kernel  exclusive prefix over segments, one workgroup per column (a block total is rescaled by its
//                         max when combined), plus the open tie group entering every segment and the index of its
//                         first event row of A;
//   3 cox_scan_kernel     the segment re-walked from its prefix, with the recurrence of pass 1 (CoxRun, the one copy of it):
//                         A rows (a chunk of them per launch), the segment's partials of loglik and U, and d_i / S0_i
//                         (Efron: h1_i, and h2_i beside it) at every group end;
//   4 cox_finish_kernel + cox_w_kernel: the suffix sum of d_i / S0_i (over segments, then inside each segment by wave
//                         scans) and w; the column sums of the loglik and U partials;
//   5 the two Grams: dlsa_gram_f64(A, -d) per chunk and dlsa_gram_f64(X, w) accumulated into H.
// Scaled sums: a prefix (M, v) stands for v exp(M) with M the max eta it covers, a suffix (Q, v) for v exp(-Q) with Q the
// smallest group max it covers, so every exponential has a non-positive argument (no overflow at any eta range) and a
// ratio never sees an underflowed denominator.
//
// Strata (a nullable int32 code per row; every row kernel and the w kernel carry them as the instantiation ST): one common
// beta, one baseline hazard per stratum, so loglik, U and H are the sums over the strata of the quantities above on each
// stratum's rows.  `order` lists the partition's rows grouped by stratum, descending time inside each; position q STARTS a
// stratum when the codes of positions q and q - 1 differ (only equality of neighbours is read; position 0 needs no flag).
// One byte per position holds that flag, written once per partition next to cox_rows (`order` does not change between
// Newton iterations), so the three walks read it coalesced instead of gathering two codes per position each.  Every running
// quantity restarts at a flagged position:
//   1 eta pass   a tie group also ends where the next position starts a stratum; (M, s0, s1) restart from empty before the
//                row is added, so the segment emits the sums since its last stratum start, and the flag "holds a start";
//   2 segscan    a flagged segment replaces the (M, v) accumulator instead of combining with it (TcS's operator; every
//                caller runs this scan, without strata no segment is flagged); the open tie group's T carry restarts at a
//                segment with an end or a start;
//   3 scan pass  the same restart inside the walk; the segment emits the (Q, v) total of its ends BEFORE its first start;
//   4 finish     walking from the right, a flagged segment replaces the hazard accumulator with that head total;
//   5 w pass     the 64-lane suffix is segmented (lane l absorbs lanes below the first flagged lane above l) and the carry
//                of the steps already done is dropped once a start lies between them and the lane.
// M restarts per stratum, so a prefix (M, v) and a suffix (Q, v) only ever cover rows and group ends of one stratum: Q is
// the smallest group max among ends of the row's own stratum at or after the row, each such max covers the row's eta, and
// "every exponent <= 0" holds stratum by stratum.  A stratum without events has hazard 0 at all its ends and adds nothing.
#include "common.h"
#include "newton_fit.h"     // the Newton state, loop and epilogue; host_calls.h
#include <math.h>
#include <algorithm>
#include <type_traits>

typedef double dlsa_cox_d2v __attribute__((ext_vector_type(2)));

namespace dlsa {

#include "logistic.h"      // exp_neg
#include "rowdot.h"        // merged_reduce, row_of_lane, lane_of_row, read_lane_f64

constexpr int COX_THREADS = 256;
constexpr int COX_WAVES = COX_THREADS / 64;
constexpr int COX_RB = 4;                      // rows per batch of a wave (one merged butterfly for their dot products)
constexpr int64_t COX_MAX_SEGS = 4096;
constexpr size_t COX_A_BYTES = 256ull << 20;   // bound of the A chunk

static __device__ __forceinline__ double2 cox_ld2(const double* ptr, bool vec, int col, int p) {
    double2 r;
    const int c0 = col < p ? col : 0;
    if (vec) {
        const dlsa_cox_d2v t = __builtin_nontemporal_load(reinterpret_cast<const dlsa_cox_d2v*>(ptr + c0));
        r.x = t.x; r.y = t.y;
    } else {
        r.x = __builtin_nontemporal_load(ptr + c0);
        r.y = __builtin_nontemporal_load(ptr + (col + 1 < p ? col + 1 : 0));
    }
    if (col >= p) r.x = 0.0;
    if (col + 1 >= p) r.y = 0.0;
    return r;
}

// (M, v) = v exp(M): combination of two prefix sums
static __device__ __forceinline__ void pre_comb(double& M, double& v, double Mb, double vb) {
    if (Mb == -INFINITY) return;
    if (M == -INFINITY) { M = Mb; v = vb; return; }
    const double Mn = fmax(M, Mb);
    v = v * exp_neg(Mn - M) + vb * exp_neg(Mn - Mb);
    M = Mn;
}
// (Q, v) = v exp(-Q): combination of two suffix sums (v = 0 is empty)
static __device__ __forceinline__ void suf_comb(double& Q, double& v, double Qb, double vb) {
    if (vb == 0.0) return;
    if (v == 0.0) { Q = Qb; v = vb; return; }
    const double Qn = fmin(Q, Qb);
    v = v * exp_neg(Q - Qn) + vb * exp_neg(Qb - Qn);
    Q = Qn;
}

// One evaluation's kernel arguments, grouped by the pass that writes each array ((EF) / (ST): only allocated and touched under
// Efron ties / with strata; cox_workspace below is the one list of the arrays, their sizes and their order in the workspace).
struct CoxArgs {
    // the problem
    const double* X; int64_t ldx;
    const double* time; const double* event; const int64_t* order;
    int64_t n; int p; int ties;
    const double* beta;
    int64_t L; int nseg; int ld;     // segments of L positions; ld: columns of the column-major segment arrays = nseg
    const unsigned char* sflag;      // (ST) [n] per position: 1 = the position starts a stratum (position 0: 0); null = unstratified
    // pass 1 (eta)
    double* eta;                     // [n] per position
    double* segM; double* segV;      // [nseg], [(p + 1) x nseg]: segment totals (col 0 = S0, 1 + c = S1_c)
    int* tie;                        // [4 x nseg]: has_end, head events (up to the first end), tail events (after the last end), event ends
    int* tie2;                       // (EF) [nseg]: ends of the segment whose own run holds two events or more
    double* tailV;                   // (EF) [(p + 1) x nseg]: sums over the segment's event rows after its last end (all of them without one), scaled by segM
    int* sst;                        // (ST) [nseg]: the segment holds a stratum start
    // pass 2 (segment scan)
    double* preM; double* preV;      // exclusive prefixes of segM / segV, same layout
    double* tcM; double* tcV;        // (EF) [nseg], [(p + 1) x nseg]: T0 / T1 of the tie group open at the segment's start
    int* carry;                      // [nseg]: events of the tie group open at the segment's start
    int64_t* gidx;                   // [nseg + 1]: first A-row index of each segment; gidx[nseg] = D
    // pass 3 (scan), one launch per chunk of A rows
    double* A; int64_t lda; double* dA; int64_t g0; int64_t ca; int chunk; int nchunks;
    double* hzv; double* hzq;        // [n] d / S0 (EF: h1) at event-group ends as (Q, v), v = 0 elsewhere
    double* h2v;                     // (EF) [n] h2 at group ends as (hzq, v); -1 at every other position
    double* segLL; double* segU;     // [nseg], [p x nseg]
    double* segHq; double* segHv;    // [nseg] segment totals of d / S0 as (Q, v); (ST) of the segment's ends before its first stratum start
    double* segNq; double* segNv;    // (EF) [nseg] (Q, h2) of the segment's first end
    // pass 4 (finish, w)
    double* sufHq; double* sufHv;    // [nseg] exclusive suffix of segH over the later segments
    double* sufNq; double* sufNv;    // (EF) [nseg] (Q, h2) of the first end after the segment
    double* wv; int64_t vlo; int64_t vstep; int64_t vrows;      // Gram weights of the view rows [vlo + r vstep, r < vrows]
    double* w_out;                   // [n] per position, nullable
};

// The lane's pair (col, col + 1) of segment s in a column-major segment array whose column `col` is row `row0 + col` (1 under
// the S0 / T0 row of segV, preV, tailV, tcV; 0 in segU): a column at or beyond p loads as 0 and is not stored.
static __device__ __forceinline__ double2 seg_ld2(const CoxArgs& a, const double* V, int row0, int col, int s) {
    double2 r;
    r.x = col < a.p ? V[(int64_t)(row0 + col) * a.ld + s] : 0.0;
    r.y = col + 1 < a.p ? V[(int64_t)(row0 + col + 1) * a.ld + s] : 0.0;
    return r;
}
static __device__ __forceinline__ void seg_st2(const CoxArgs& a, double* V, int row0, int col, int s, double2 v) {
    if (col < a.p) V[(int64_t)(row0 + col) * a.ld + s] = v.x;
    if (col + 1 < a.p) V[(int64_t)(row0 + col + 1) * a.ld + s] = v.y;
}

// ---- the forward recurrence of the two walks (passes 1 and 3) -------------------------------------------------------------
// The running max M of eta and the sums of exp(eta - M) [1, x] since the last stratum start (s0, s1); under EF the same sums
// over the event rows of the open tie group (t0, t1), scaled by the same M.  Lane l holds columns c * 128 + 2 l, + 1 of pair c.
// The scan pass is the eta pass's segment re-walked from its prefix, so both walk with these operations and nothing else.
template <int NC, bool EF>
struct CoxRun {
    double M, s0, t0;
    double2 s1[NC], t1[EF ? NC : 1];

    __device__ __forceinline__ void clear_group() {
        if constexpr (EF) {
            t0 = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) { t1[c].x = 0.0; t1[c].y = 0.0; }
        }
    }
    // empty sums: the eta pass's segment before its first row, and every stratum start (the open tie group is not touched:
    // it closed at the position in front of the start)
    __device__ __forceinline__ void restart() {
        M = -INFINITY; s0 = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) { s1[c].x = 0.0; s1[c].y = 0.0; }
    }
    __device__ __forceinline__ void rescale(double Mn) {
        const double r = M == -INFINITY ? 0.0 : exp_neg(Mn - M);
        s0 *= r;
#pragma unroll
        for (int c = 0; c < NC; ++c) { s1[c].x *= r; s1[c].y *= r; }
        if constexpr (EF) {
            t0 *= r;
#pragma unroll
            for (int c = 0; c < NC; ++c) { t1[c].x *= r; t1[c].y *= r; }
        }
        M = Mn;
    }
    // the row (eta, x) joins the sums; returns its term e = exp(eta - M)
    __device__ __forceinline__ double add_row(double et, const double2 (&x)[NC]) {
        if (et > M) rescale(et);                            // wave-uniform: rescale the running sums to the new max
        const double e = exp_neg(M - et);
        s0 += e;
#pragma unroll
        for (int c = 0; c < NC; ++c) { s1[c].x = fma(e, x[c].x, s1[c].x); s1[c].y = fma(e, x[c].y, s1[c].y); }
        return e;
    }
    // an event row also joins the open tie group
    __device__ __forceinline__ void add_to_group(double e, const double2 (&x)[NC]) {
        if constexpr (EF) {
            t0 += e;
#pragma unroll
            for (int c = 0; c < NC; ++c) { t1[c].x = fma(e, x[c].x, t1[c].x); t1[c].y = fma(e, x[c].y, t1[c].y); }
        }
    }
};

// ---- pass 1 ----------------------------------------------------------------------------------------------------------
template <int RB, int I>
__device__ __forceinline__ void bcast_rows(double v, double (&out)[RB]) {
    if constexpr (I < RB) {
        out[I] = read_lane_f64<lane_of_row<RB>(I)>(v);
        bcast_rows<RB, I + 1>(v, out);
    }
}

template <int NC, bool VEC, bool EF, bool ST>
__global__ __launch_bounds__(COX_THREADS) void cox_eta_kernel(CoxArgs a) {
    constexpr int RB = NC >= 8 ? 1 : COX_RB;        // (wide rows: one row per step keeps the row registers from spilling)
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * COX_WAVES + (threadIdx.x >> 6);
    if (s >= a.nseg) return;
    double2 b[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 128 + 2 * lane;
        b[c].x = col < a.p ? a.beta[col] : 0.0;
        b[c].y = col + 1 < a.p ? a.beta[col + 1] : 0.0;
    }
    CoxRun<NC, EF> run;
    run.restart();
    run.clear_group();
    int has_end = 0, head = 0, tail = 0, nend = 0;
    int nend2 = 0, has_start = 0;                   // (EF) ends with two own events or more, (ST) the segment holds a stratum start
    (void)nend2; (void)has_start;
    const int64_t p0 = (int64_t)s * a.L, p1 = min(p0 + a.L, a.n);
    const int myrow = row_of_lane<RB>(lane);
    for (int64_t q0 = p0; q0 < p1; q0 += RB) {
        double2 x[RB][NC];
        double dot[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int64_t q = min(q0 + i, p1 - 1);
            const double* rowp = a.X + a.order[q] * a.ldx;
            double t = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                x[i][c] = cox_ld2(rowp, VEC, c * 128 + 2 * lane, a.p);
                t = fma(x[i][c].x, b[c].x, fma(x[i][c].y, b[c].y, t));
            }
            dot[i] = t;
        }
        const double eta = merged_reduce<RB>(dot, lane);
        if ((lane & rep_mask<RB>()) == 0 && q0 + myrow < p1) a.eta[q0 + myrow] = eta;
        double e_r[RB];
        bcast_rows<RB, 0>(eta, e_r);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int64_t q = q0 + i;
            if (q >= p1) break;
            const double et = e_r[i];
            if constexpr (ST) {
                if (a.sflag[q]) { has_start = 1; run.restart(); }       // a new stratum: the segment emits the sums since its last start
            }
            const double e = run.add_row(et, x[i]);
            const int64_t r = a.order[q];
            const int ev = a.event[r] != 0.0;
            bool end = q + 1 == a.n || a.time[a.order[q + 1]] != a.time[r];
            if constexpr (ST) end = end || a.sflag[q + 1];      // (equal times on the two sides of a boundary are not tied)
            tail += ev;
            if (ev) run.add_to_group(e, x[i]);
            if (end) {
                if (!has_end) head = tail;
                nend += tail > 0;
                if constexpr (EF) nend2 += tail > 1;
                run.clear_group();
                has_end = 1;
                tail = 0;
            }
        }
    }
    if (lane == 0) {
        a.segM[s] = run.M;
        a.segV[s] = run.s0;
        a.tie[s] = has_end; a.tie[a.ld + s] = head; a.tie[2 * a.ld + s] = tail; a.tie[3 * a.ld + s] = nend;
        if constexpr (EF) { a.tie2[s] = nend2; a.tailV[s] = run.t0; }
        if constexpr (ST) a.sst[s] = has_start;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 128 + 2 * lane;
        seg_st2(a, a.segV, 1, col, s, run.s1[c]);
        if constexpr (EF) seg_st2(a, a.tailV, 1, col, s, run.t1[c]);
    }
}

// ---- block-wide exclusive scan over the nseg segments, 256 threads each owning a contiguous range --------------------
// Op: void comb(State& acc, const State& next) (associative, applied left to right); load(s) / store(s, excl).
template <class State, class Load, class Comb, class Store>
__device__ void seg_scan(int nseg, State ident, Load load, Comb comb, Store store, State* sh, bool reverse) {
    const int t = threadIdx.x;
    const int per = (nseg + COX_THREADS - 1) / COX_THREADS;
    const int lo = min(nseg, t * per), hi = min(nseg, lo + per);
    // forward: segments in index order; reverse: walked from the end (suffix scans)
    auto seg = [&](int i) { return reverse ? nseg - 1 - i : i; };
    State acc = ident;
    for (int i = lo; i < hi; ++i) comb(acc, load(seg(i)));
    sh[t] = acc;
    __syncthreads();
    if (t == 0) {
        State run = ident;
        for (int k = 0; k < COX_THREADS; ++k) { const State v = sh[k]; sh[k] = run; comb(run, v); }
    }
    __syncthreads();
    State run = sh[t];
    for (int i = lo; i < hi; ++i) { const State v = load(seg(i)); store(seg(i), run); comb(run, v); }
    __syncthreads();
}

struct TieS { int f, c; };
struct TcS { int f; double M, v; };     // a scaled sum that a flagged segment restarts (Efron's T carry; strata: prefix and hazard suffix)
// the restart operator: a flagged segment replaces the accumulator, any other combines with it (associative: a range of
// segments is flagged when any of them is, and then holds the sum from its last flagged segment on).  Without strata no
// segment of the prefix and of the hazard suffix is flagged, and the operator is pre_comb / suf_comb.
static __device__ __forceinline__ void tcs_restart_pre(TcS& x, const TcS& y) {
    if (y.f) { x.M = y.M; x.v = y.v; x.f = 1; }
    else pre_comb(x.M, x.v, y.M, y.v);
}
static __device__ __forceinline__ void tcs_restart_suf(TcS& x, const TcS& y) {
    if (y.f) { x.M = y.M; x.v = y.v; x.f = 1; }
    else suf_comb(x.M, x.v, y.M, y.v);
}

// ---- pass 2: blocks 0 .. p: prefix of column (S0, S1_c); block p + 1: tie groups and A-row indices; Efron: blocks
// p + 2 .. 2 p + 2: column (T0, T1_c) of the tie group open at every segment's start -------------------------------------
__global__ __launch_bounds__(COX_THREADS) void cox_segscan_kernel(CoxArgs a) {
    __shared__ TieS sht[COX_THREADS];
    __shared__ int64_t shg[COX_THREADS];
    __shared__ TcS shc[COX_THREADS];
    const int c = blockIdx.x;
    if (c != a.p + 1) {
        // one scaled-sum scan for both: column cc of the prefix (segV -> preV, preM) or of the T carry (tailV -> tcV, tcM)
        const bool tc = c > a.p + 1;
        const int cc = tc ? c - a.p - 2 : c;
        const double* V = (tc ? a.tailV : a.segV) + (int64_t)cc * a.ld;
        double* P = (tc ? a.tcV : a.preV) + (int64_t)cc * a.ld;
        double* PM = tc ? a.tcM : a.preM;
        seg_scan<TcS>(a.nseg, TcS{0, -INFINITY, 0.0},
                      // strata: a segment with a stratum start replaces the prefix (its sums run from its last start); the prefix of a
                      // segment whose first position starts a stratum may hold anything, the walk restarts there.
                      // T carry (TieS's operator on scaled sums): a segment with an end restarts the sum at its tail, any other adds
                      // all its event rows; a segment that starts a stratum at its first position may hold no end, and restarts the
                      // group too.
                      [&](int s) { return TcS{(tc ? a.tie[s] : 0) | (a.sflag ? a.sst[s] : 0), a.segM[s], V[s]}; },
                      [](TcS& x, const TcS& y) { tcs_restart_pre(x, y); },
                      [&](int s, const TcS& e) { P[s] = e.v; if (cc == 0) PM[s] = e.M; }, shc, false);
        return;
    }
    // the open tie group entering segment s: (f, c) = (segment has an end, events after its last end / all its events)
    seg_scan<TieS>(a.nseg, TieS{0, 0},
                   [&](int s) { return TieS{a.tie[s], a.tie[2 * a.ld + s]}; },
                   [](TieS& x, const TieS& y) { x.c = y.f ? y.c : x.c + y.c; x.f |= y.f; },
                   [&](int s, const TieS& e) { a.carry[s] = e.c; }, sht, false);
    // event groups that END in segment s: its event ends, the first one counted with the events carried in
    auto count = [&](int s) -> int64_t {
        if (!a.tie[s]) return 0;
        const int head = a.tie[a.ld + s], nend = a.tie[3 * a.ld + s];
        int rows = nend - (head > 0) + (head + a.carry[s] > 0);
        // Efron: a second A row for every group of two events or more (the first end's group counted with its carry)
        if (a.ties) rows += a.tie2[s] - (head > 1) + (head + a.carry[s] > 1);
        return rows;
    };
    seg_scan<int64_t>(a.nseg, (int64_t)0, count, [](int64_t& x, const int64_t& y) { x += y; },
                      [&](int s, const int64_t& e) { a.gidx[s] = e; }, shg, false);
    if (threadIdx.x == 0) {
        int64_t tot = 0;
        for (int s = 0; s < a.nseg; ++s) tot += count(s);      // (one thread: nseg <= 4096 values already in L2)
        a.gidx[a.nseg] = tot;
    }
}

// ---- pass 3 ------------------------------------------------------------------------------------------------------------
// Efron's sums over l = 0 .. d - 1 at a group end (d >= 2; s0, t0, d are the same in every lane): lane t takes l = t, t + 64, ..
// in ascending order and one butterfly of fixed shape adds the 64 partials, so every lane holds the same bits.
struct EfronSums { double h1, h2, slog, k0, k1, k2; };
static __device__ __forceinline__ double wave_sum(double v) {
    v = xor_add<32>(v); v = xor_add<16>(v); v = xor_add<8>(v); v = xor_add<4>(v); v = xor_add<2>(v);
    return xor_add<1>(v);
}
static __device__ __forceinline__ EfronSums efron_sums(double s0, double t0, int d, int lane) {
    EfronSums r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double dd = (double)d;
    for (int l = lane; l < d; l += 64) {
        const double f = (double)l / dd;
        const double phi = s0 - f * t0;              // >= s0 / d: t0 <= s0 and f <= (d - 1) / d
        const double ip = 1.0 / phi, fp = f * ip;
        r.h1 += ip; r.h2 += fp; r.slog += log(phi);
        r.k0 = fma(ip, ip, r.k0); r.k1 = fma(fp, ip, r.k1); r.k2 = fma(fp, fp, r.k2);
    }
    r.h1 = wave_sum(r.h1);
    r.h2 = wave_sum(r.h2);
    r.slog = wave_sum(r.slog);
    r.k0 = wave_sum(r.k0);
    r.k1 = wave_sum(r.k1);
    r.k2 = wave_sum(r.k2);
    return r;
}

template <int NC, bool VEC, bool EF, bool ST>
__global__ __launch_bounds__(COX_THREADS) void cox_scan_kernel(CoxArgs a) {
    constexpr int RB = NC >= 8 ? 1 : COX_RB;
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * COX_WAVES + (threadIdx.x >> 6);
    if (s >= a.nseg) return;
    const int64_t gs = a.gidx[s], ge = a.gidx[s + 1];
    const int owner = (int)min<int64_t>(gs / a.ca, a.nchunks - 1);       // the chunk that also writes the segment's partials
    const bool own = owner == a.chunk;
    if (!own && (ge <= a.g0 || gs >= a.g0 + a.ca)) return;               // no A row of this chunk ends here
    CoxRun<NC, EF> run;                                                  // the segment's exclusive prefix
    run.M = a.preM[s]; run.s0 = a.preV[s];
    double2 u[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        run.s1[c] = seg_ld2(a, a.preV, 1, c * 128 + 2 * lane, s);
        u[c].x = 0.0; u[c].y = 0.0;
    }
    int open = a.carry[s];
    int64_t g = gs;
    double ll = 0.0, hq = 0.0, hv = 0.0;
    double nq = 0.0, nv = 0.0;                                           // (EF) the (Q, h2) of the segment's first end
    bool seen_end = false, seen_start = false;
    (void)nq; (void)nv; (void)seen_end; (void)seen_start;
    if constexpr (EF) {
        // T0 / T1 of the open tie group, brought under the prefix max (which covers the group's rows)
        const double cM = a.tcM[s];
        const double r = (cM == -INFINITY || run.M == -INFINITY) ? 0.0 : exp_neg(run.M - cM);
        run.t0 = a.tcV[s] * r;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double2 t = seg_ld2(a, a.tcV, 1, c * 128 + 2 * lane, s);
            run.t1[c].x = t.x * r; run.t1[c].y = t.y * r;
        }
    }
    // A row g (if the chunk holds it): the lane's pair c of it is val(c), its Gram weight wgt
    auto store_row = [&](int64_t gr, double wgt, auto val) {
        if (gr < a.g0 || gr >= a.g0 + a.ca) return;
        double* Ar = a.A + (gr - a.g0) * a.lda;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = c * 128 + 2 * lane;
            const double2 v = val(c);
            if (col < a.p) Ar[col] = v.x;
            if (col + 1 < a.p) Ar[col + 1] = v.y;
        }
        if (lane == 0) a.dA[gr - a.g0] = wgt;
    };
    const int64_t p0 = (int64_t)s * a.L, p1 = min(p0 + a.L, a.n);
    for (int64_t q0 = p0; q0 < p1; q0 += RB) {
        double2 x[RB][NC];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int64_t q = min(q0 + i, p1 - 1);
            const double* rowp = a.X + a.order[q] * a.ldx;
#pragma unroll
            for (int c = 0; c < NC; ++c) x[i][c] = cox_ld2(rowp, VEC, c * 128 + 2 * lane, a.p);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int64_t q = q0 + i;
            if (q >= p1) break;
            const double et = a.eta[q];
            if constexpr (ST) {
                if (a.sflag[q]) { seen_start = true; open = 0; run.restart(); run.clear_group(); }     // a new stratum: the prefix and the open group start empty
            }
            const double e = run.add_row(et, x[i]);
            const int64_t r = a.order[q];
            const bool ev = a.event[r] != 0.0;
            bool end = q + 1 == a.n || a.time[a.order[q + 1]] != a.time[r];
            if constexpr (ST) end = end || a.sflag[q + 1];
            if (ev) {
                ++open;
                run.add_to_group(e, x[i]);
                if (own) {
                    ll += et;
#pragma unroll
                    for (int c = 0; c < NC; ++c) { u[c].x += x[i][c].x; u[c].y += x[i][c].y; }
                }
            }
            // a group end with events: its terms of loglik and U, its A rows and its hazard increment (EF: h1, and h2 beside it)
            double hzv = 0.0, h2 = 0.0;
            (void)h2;
            if (end && open > 0) {
                const double d = (double)open;
                const double inv = 1.0 / run.s0;
                if constexpr (EF) {
                    // d = 1: Breslow's terms; otherwise the sums over l and the Cholesky factor of K
                    double h1 = inv, slog = 0.0, L11 = inv, L21 = 0.0, L22 = 0.0;
                    if (open > 1) {
                        const EfronSums es = efron_sums(run.s0, run.t0, open, lane);
                        h1 = es.h1; h2 = es.h2; slog = es.slog;
                        L11 = sqrt(es.k0);
                        L21 = -es.k1 / L11;
                        L22 = sqrt(fmax(es.k2 - L21 * L21, 0.0));
                    } else if (own) {
                        slog = log(run.s0);
                    }
                    if (own) {
                        ll -= d * run.M + slog;
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            u[c].x = fma(-h1, run.s1[c].x, fma(h2, run.t1[c].x, u[c].x));
                            u[c].y = fma(-h1, run.s1[c].y, fma(h2, run.t1[c].y, u[c].y));
                        }
                        hzv = h1;
                    }
                    store_row(g++, -1.0, [&](int c) {
                        return make_double2(fma(L11, run.s1[c].x, L21 * run.t1[c].x), fma(L11, run.s1[c].y, L21 * run.t1[c].y));
                    });
                    // (the group's two rows may lie in different chunks)
                    if (open > 1) store_row(g++, -1.0, [&](int c) { return make_double2(L22 * run.t1[c].x, L22 * run.t1[c].y); });
                } else {
                    if (own) {
                        ll -= d * (run.M + log(run.s0));
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            u[c].x = fma(-d * inv, run.s1[c].x, u[c].x);
                            u[c].y = fma(-d * inv, run.s1[c].y, u[c].y);
                        }
                        hzv = d * inv;
                    }
                    store_row(g++, -d, [&](int c) { return make_double2(run.s1[c].x * inv, run.s1[c].y * inv); });
                }
                // (walked forward: the segment's total needs no order among its terms but a fixed one)
                if (own && (!ST || !seen_start)) suf_comb(hq, hv, run.M, hzv);
            }
            if (end) {
                open = 0;
                run.clear_group();
                if constexpr (EF) {
                    if (!seen_end) { seen_end = true; nq = run.M; nv = h2; }
                }
            }
            if (own && lane == 0) {
                a.hzv[q] = hzv; a.hzq[q] = run.M;
                if constexpr (EF) a.h2v[q] = end ? h2 : -1.0;
            }
        }
    }
    if (!own) return;
    if (lane == 0) { a.segLL[s] = ll; a.segHq[s] = hq; a.segHv[s] = hv; }
    if constexpr (EF) {
        if (lane == 0) { a.segNq[s] = nq; a.segNv[s] = nv; }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) seg_st2(a, a.segU, 0, c * 128 + 2 * lane, s, u[c]);
}

// ---- pass 4: suffix of d / S0 over segments (block 0) and the column sums of loglik / U (blocks 1 ..) ------------------
// Efron: block p + 2: the (Q, h2) of the first group end after every segment.
__global__ __launch_bounds__(COX_THREADS) void cox_finish_kernel(CoxArgs a, double* g, double* loglik) {
    __shared__ double red[COX_THREADS];
    __shared__ TcS shc[COX_THREADS];
    if ((int)blockIdx.x == a.p + 2) {
        // walked from the last segment: the end met last is the nearest one
        seg_scan<TcS>(a.nseg, TcS{0, 0.0, 0.0},
                      [&](int s) { return TcS{a.tie[s], a.segNq[s], a.segNv[s]}; },
                      [](TcS& x, const TcS& y) { if (y.f) x = y; },
                      [&](int s, const TcS& e) { a.sufNq[s] = e.M; a.sufNv[s] = e.v; }, shc, true);
        return;
    }
    if (blockIdx.x == 0) {
        // strata: segH is the total of the segment's ends before its first stratum start, which is all that the positions
        // to its left may see of it and of everything after it
        seg_scan<TcS>(a.nseg, TcS{0, 0.0, 0.0},
                      [&](int s) { return TcS{a.sflag ? a.sst[s] : 0, a.segHq[s], a.segHv[s]}; },
                      [](TcS& x, const TcS& y) { tcs_restart_suf(x, y); },
                      [&](int s, const TcS& e) { a.sufHq[s] = e.M; a.sufHv[s] = e.v; }, shc, true);
        return;
    }
    // column c = blockIdx.x - 1 (c == p: loglik): thread t sums segments t, t + 256, ... in order, then a fixed tree
    const int c = blockIdx.x - 1;
    const double* src = c < a.p ? a.segU + (int64_t)c * a.ld : a.segLL;
    double acc = 0.0;
    for (int s = threadIdx.x; s < a.nseg; s += COX_THREADS) acc += src[s];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = COX_THREADS / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (c < a.p) { if (g) g[c] = red[0]; }
        else if (loglik) *loglik = red[0];
    }
}

// ---- pass 5: w per position from the suffix of d / S0: one wave per segment, 64 positions per step, walked backwards ---
// Efron: an event row also subtracts the h2 of its own group, which sits at the group's end at or after the row: the
// nearest end is copied backwards through the 64 positions, then taken from the steps done before or from sufN.
// Strata: the wave's 64 flags are one ballot; lane l's suffix stops below `bnd`, the first flagged lane above l (64 without
// one), which is also the bound of every lane it absorbs from, and the carry counts only for the lanes with bnd = 64.
template <bool EF, bool ST>
__global__ __launch_bounds__(COX_THREADS) void cox_w_kernel(CoxArgs a) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * COX_WAVES + (threadIdx.x >> 6);
    if (s >= a.nseg) return;
    double cq = a.sufHq[s], cv = a.sufHv[s];          // everything after the segment
    double nq = 0.0, nv = 0.0;
    (void)nq; (void)nv;
    if constexpr (EF) { nq = a.sufNq[s]; nv = a.sufNv[s]; }
    const int64_t p0 = (int64_t)s * a.L, p1 = min(p0 + a.L, a.n);
    for (int64_t top = p1; top > p0; top -= 64) {
        const int64_t q = top - 64 + lane;
        const bool valid = q >= p0;
        double hq = valid ? a.hzq[q] : 0.0, hv = valid ? a.hzv[q] : 0.0;
        double eq = hq, e2 = -1.0;
        (void)eq; (void)e2;
        int bnd = 64;
        bool start0 = false;       // the step's first position starts a stratum: nothing carries to the positions before it
        (void)start0;
        if constexpr (ST) {
            const unsigned long long fm = __ballot(valid && a.sflag[q] != 0);
            const unsigned long long above = (fm >> lane) >> 1;
            if (above) bnd = lane + 1 + __builtin_ctzll(above);
            start0 = fm & 1ull;
        }
        if constexpr (EF) {
            if (valid) e2 = a.h2v[q];
            int have = e2 >= 0.0;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const double oq = __shfl_down(eq, k, 64), o2 = __shfl_down(e2, k, 64);
                const int oh = __shfl_down(have, k, 64);
                if (lane + k < 64 && !have && oh) { eq = oq; e2 = o2; have = 1; }
            }
            if (!have) { eq = nq; e2 = nv; }
            nq = __shfl(eq, 0, 64); nv = __shfl(e2, 0, 64);
        }
        // inclusive suffix inside the 64 positions (lane l combines lanes >= l)
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const double oq = __shfl_down(hq, k, 64), ov = __shfl_down(hv, k, 64);
            if (lane + k < bnd) suf_comb(hq, hv, oq, ov);
        }
        double tq = hq, tv = hv;
        if (bnd == 64) suf_comb(tq, tv, cq, cv);
        if (valid) {
            const double et = a.eta[q];
            double w = tv == 0.0 ? 0.0 : tv * exp_neg(tq - et);
            if constexpr (EF) {
                if (a.event[a.order[q]] != 0.0 && e2 > 0.0) w -= e2 * exp_neg(eq - et);      // (c >= h1 >= h2: w >= 0)
            }
            if (a.w_out) a.w_out[q] = w;
            const int64_t rel = a.order[q] - a.vlo;
            if (rel >= 0 && rel % a.vstep == 0 && rel / a.vstep < a.vrows) a.wv[rel / a.vstep] = w;
        }
        cq = __shfl(tq, 0, 64); cv = __shfl(tv, 0, 64);
        if constexpr (ST) {
            if (start0) { cq = 0.0; cv = 0.0; }
        }
    }
}

// ---- layout of the partition's rows: lo, hi and whether they are exactly lo + j step (strided / contiguous) -------------
__global__ __launch_bounds__(1024) void cox_layout_kernel(const int64_t* __restrict__ order, int64_t n, int64_t* out) {
    __shared__ int64_t smn[16], smx[16];
    __shared__ int bad_sh;
    int64_t mn = INT64_MAX, mx = -1;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) { mn = min(mn, order[i]); mx = max(mx, order[i]); }
    for (int m = 32; m >= 1; m >>= 1) { mn = min(mn, (int64_t)__shfl_xor(mn, m, 64)); mx = max(mx, (int64_t)__shfl_xor(mx, m, 64)); }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    if (threadIdx.x == 0) bad_sh = 0;
    __syncthreads();
    mn = smn[0]; mx = smx[0];
    for (int k = 1; k < (int)blockDim.x / 64; ++k) { mn = min(mn, smn[k]); mx = max(mx, smx[k]); }
    const int64_t step = n > 1 ? (mx - mn) / (n - 1) : 1;
    // n distinct indices in [mn, mx] that are all mn + j step with mx - mn = (n - 1) step: exactly the progression
    bool bad = n > 1 && (step < 1 || (mx - mn) != step * (n - 1));
    for (int64_t i = threadIdx.x; i < n && !bad; i += blockDim.x) bad = (order[i] - mn) % step != 0;
    if (bad) atomicOr(&bad_sh, 1);
    __syncthreads();
    if (threadIdx.x == 0) { out[0] = mn; out[1] = mx; out[2] = bad_sh ? 0 : step; }
}

// ---- strata: the flag byte of every position of a partition (once per partition, like the row layout) -------------------
__global__ void cox_strata_flag_kernel(const int32_t* __restrict__ strata, const int64_t* __restrict__ order, int64_t n,
                                       unsigned char* __restrict__ flag) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) flag[q] = q > 0 && strata[order[q]] != strata[order[q - 1]];
}

__global__ void cox_fill_kernel(double* __restrict__ v, int64_t n, double val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = val;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The one list of the workspace: every array of a pass in its order, each 256-byte aligned, with the geometry that sizes them
// (segments of L positions, A chunks of ca rows of lda doubles).  With a null base only the sizes are walked, so the byte
// queries and the passes cannot disagree.  The Efron arrays follow the Breslow layout and the strata arrays follow both.
struct CoxWs {
    CoxArgs a;              // L, ca, lda and every array pointer; the entries fill in the problem
    int64_t* misc;          // cox_rows' read-back
    void* gram; size_t gram_bytes;
    size_t total;
};
static CoxWs cox_workspace(char* base, int64_t max_rows, int p, int ties, bool stratified) {
    CoxWs w{};
    CoxArgs& a = w.a;
    const size_t n = (size_t)std::max<int64_t>(max_rows, 1);
    a.L = std::max<int64_t>(64, ((int64_t)n + COX_MAX_SEGS - 1) / COX_MAX_SEGS);
    a.L = (a.L + COX_RB - 1) / COX_RB * COX_RB;
    a.lda = (p + 1) / 2 * 2;
    a.ca = std::max<int64_t>(1, std::min<int64_t>((int64_t)n, (int64_t)(COX_A_BYTES / (8 * (size_t)a.lda))));
    const size_t S = COX_MAX_SEGS;      // segment arrays sized for the largest count any n gives (the query stays monotone)
    const size_t P1 = (size_t)p + 1;
    size_t o = 0;
    auto take = [&](auto*& ptr, size_t bytes) {
        if (base) ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + o);
        o = align_up(o + bytes, 256);
    };
    take(a.eta, 8 * n); take(a.hzv, 8 * n); take(a.hzq, 8 * n); take(a.wv, 8 * n);
    take(a.segM, 8 * S); take(a.segV, 8 * S * P1);
    take(a.preM, 8 * S); take(a.preV, 8 * S * P1);
    take(a.tie, 4 * 4 * S); take(a.gidx, 8 * (S + 1)); take(a.carry, 4 * S);
    take(a.segLL, 8 * S); take(a.segU, 8 * S * (size_t)p);
    take(a.segHq, 8 * S); take(a.segHv, 8 * S);
    take(a.sufHq, 8 * S); take(a.sufHv, 8 * S);
    take(a.A, 8 * (size_t)a.ca * a.lda); take(a.dA, 8 * (size_t)a.ca);
    take(w.misc, 256);
    const size_t gram0 = o;
    take(w.gram, gram_workspace_bytes_impl(std::max<int64_t>((int64_t)n, a.ca), p, 8));
    w.gram_bytes = o - gram0;
    if (ties == DLSA_COX_TIES_EFRON) {
        take(a.h2v, 8 * n);
        take(a.tailV, 8 * S * P1);
        take(a.tcM, 8 * S); take(a.tcV, 8 * S * P1);
        take(a.tie2, 4 * S);
        take(a.segNq, 8 * S); take(a.segNv, 8 * S);
        take(a.sufNq, 8 * S); take(a.sufNv, 8 * S);
    }
    if (stratified) {                   // (the flags themselves: cox_strata_flags, once per partition)
        take(a.sflag, n);
        take(a.sst, 4 * S);
    }
    w.total = o;
    return w;
}

static bool cox_vec_ok(const double* X, int64_t ldx, int p) {
    return (p % 2 == 0) && (ldx % 2 == 0) && (((uintptr_t)X & 15) == 0);
}

// The runtime (Efron, stratified) pair as the template arguments <EF, ST>: f(std::bool_constant<EF>, std::bool_constant<ST>).
template <class F>
static void cox_dispatch(const CoxArgs& a, F f) {
    const bool efron = a.ties == DLSA_COX_TIES_EFRON;
    if (a.sflag) {
        if (efron) f(std::true_type{}, std::true_type{});
        else f(std::false_type{}, std::true_type{});
    } else {
        if (efron) f(std::true_type{}, std::false_type{});
        else f(std::false_type{}, std::false_type{});
    }
}

template <int NC, bool EF, bool ST>
static void launch_rows(bool scan, bool vec, const CoxArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.nseg + COX_WAVES - 1) / COX_WAVES));
    if (scan) {
        if (vec) hipLaunchKernelGGL((cox_scan_kernel<NC, true, EF, ST>), grid, dim3(COX_THREADS), 0, s, a);
        else hipLaunchKernelGGL((cox_scan_kernel<NC, false, EF, ST>), grid, dim3(COX_THREADS), 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((cox_eta_kernel<NC, true, EF, ST>), grid, dim3(COX_THREADS), 0, s, a);
        else hipLaunchKernelGGL((cox_eta_kernel<NC, false, EF, ST>), grid, dim3(COX_THREADS), 0, s, a);
    }
}
static int launch_row_pass(bool scan, const CoxArgs& a, hipStream_t s) {
    const bool vec = cox_vec_ok(a.X, a.ldx, a.p);
    const int nc = (a.p + 127) / 128;
    cox_dispatch(a, [&](auto ef, auto st) {
        constexpr bool EF = decltype(ef)::value, ST = decltype(st)::value;
        if (nc <= 1) launch_rows<1, EF, ST>(scan, vec, a, s);
        else if (nc <= 2) launch_rows<2, EF, ST>(scan, vec, a, s);
        else if (nc <= 4) launch_rows<4, EF, ST>(scan, vec, a, s);
        else if (nc <= 8) launch_rows<8, EF, ST>(scan, vec, a, s);
        else launch_rows<16, EF, ST>(scan, vec, a, s);
    });
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

// Row layout of a partition (once per partition: `order` does not change between iterations): the X-term Gram runs on
// the view rows vlo + r vstep; a partition that is no such progression is covered by views of n rows one after another.
struct CoxRows { int64_t lo, hi, step; };
static int cox_rows(const int64_t* order, int64_t n, int64_t* misc_dev, CoxRows* out, hipStream_t s) {
    hipLaunchKernelGGL(cox_layout_kernel, dim3(1), dim3(1024), 0, s, order, n, misc_dev);
    DLSA_HIP_CHECK(hipGetLastError());
    int64_t h[3];
    DLSA_HIP_CHECK(hipMemcpyAsync(h, misc_dev, sizeof(h), hipMemcpyDeviceToHost, s));
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    out->lo = h[0]; out->hi = h[1]; out->step = h[2];
    return DLSA_OK;
}

// The stratum-start flags of a partition's positions (null strata: nothing to do, the pass runs unstratified).
static int cox_strata_flags(const int32_t* strata, const int64_t* order, int64_t n, const CoxWs& w, hipStream_t s) {
    if (!strata) return DLSA_OK;
    hipLaunchKernelGGL(cox_strata_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, strata, order, n,
                       const_cast<unsigned char*>(w.a.sflag));
    DLSA_HIP_CHECK(hipGetLastError());
    return DLSA_OK;
}

// One partition at a fixed beta: H (and g, loglik, w_out) as described at the top.  *D_out: number of A rows (Breslow: the
// event groups; Efron: one more for every group of two events or more; 0 = no event).
static int cox_pass_impl(const double* X, int64_t ldx, const double* time, const double* event, const int64_t* order, int64_t n, int p,
                         int ties, const CoxRows& rows, const double* beta, double* H, int64_t ldh, double* g, double* loglik,
                         double* w_out, const CoxWs& w, int64_t* D_out, hipStream_t s) {
    CoxArgs a = w.a;
    a.X = X; a.ldx = ldx; a.time = time; a.event = event; a.order = order; a.n = n; a.p = p; a.ties = ties; a.beta = beta;
    a.nseg = (int)((n + a.L - 1) / a.L); a.ld = a.nseg;
    a.w_out = w_out;
    const bool efron = ties == DLSA_COX_TIES_EFRON;
    int rc;

    rc = launch_row_pass(false, a, s);
    if (rc) return rc;
    hipLaunchKernelGGL(cox_segscan_kernel, dim3(efron ? 2 * p + 3 : p + 2), dim3(COX_THREADS), 0, s, a);
    DLSA_HIP_CHECK(hipGetLastError());
    int64_t D = 0;
    DLSA_HIP_CHECK(hipMemcpyAsync(&D, a.gidx + a.nseg, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    *D_out = D;
    a.nchunks = (int)std::max<int64_t>(1, (D + a.ca - 1) / a.ca);
    bool first = true;
    for (int k = 0; k < a.nchunks; ++k) {
        a.chunk = k; a.g0 = (int64_t)k * a.ca;
        rc = launch_row_pass(true, a, s);
        if (rc) return rc;
        const int64_t rowsA = std::min<int64_t>(a.ca, D - a.g0);
        if (rowsA > 0) {
            rc = gram_impl_f64(a.A, a.lda, a.dA, rowsA, p, H, ldh, first ? 0 : 1, w.gram, w.gram_bytes, s);
            if (rc) return rc;
            first = false;
        }
    }
    hipLaunchKernelGGL(cox_finish_kernel, dim3(efron ? p + 3 : p + 2), dim3(COX_THREADS), 0, s, a, g, loglik);
    DLSA_HIP_CHECK(hipGetLastError());
    // w and the X-term Gram over views of the partition's rows
    const int64_t span = rows.step > 0 ? n : rows.hi - rows.lo + 1;
    const int64_t vstep = rows.step > 0 ? rows.step : 1;
    for (int64_t v0 = 0; v0 < span; v0 += n) {
        a.vlo = rows.lo + v0 * vstep; a.vstep = vstep; a.vrows = std::min<int64_t>(n, span - v0);
        if (rows.step == 0) {
            hipLaunchKernelGGL(cox_fill_kernel, dim3((unsigned)((a.vrows + 255) / 256)), dim3(256), 0, s, a.wv, a.vrows, 0.0);
            DLSA_HIP_CHECK(hipGetLastError());
        }
        if (v0 > 0) a.w_out = nullptr;
        const dim3 wgrid((unsigned)((a.nseg + COX_WAVES - 1) / COX_WAVES));
        cox_dispatch(a, [&](auto ef, auto st) {
            hipLaunchKernelGGL((cox_w_kernel<decltype(ef)::value, decltype(st)::value>), wgrid, dim3(COX_THREADS), 0, s, a);
        });
        DLSA_HIP_CHECK(hipGetLastError());
        rc = gram_impl_f64(X + a.vlo * ldx, ldx * vstep, a.wv, a.vrows, p, H, ldh, first ? 0 : 1, w.gram, w.gram_bytes, s);
        if (rc) return rc;
        first = false;
    }
    return DLSA_OK;
}

}  // namespace dlsa

extern "C" {

size_t dlsa_cox_strata_workspace_bytes(int64_t max_rows, int p, int ties, int stratified) {
    if (p <= 0 || p > 2048 || max_rows < 0 || (ties != DLSA_COX_TIES_BRESLOW && ties != DLSA_COX_TIES_EFRON)) return 0;
    if (stratified != 0 && stratified != 1) return 0;
    // the Newton state after the pass scratch
    return dlsa::align_up(dlsa::cox_workspace(nullptr, max_rows, p, ties, stratified != 0).total, 256) + dlsa::newton_state_bytes(p);
}

size_t dlsa_cox_ties_workspace_bytes(int64_t max_rows, int p, int ties) { return dlsa_cox_strata_workspace_bytes(max_rows, p, ties, 0); }

size_t dlsa_cox_workspace_bytes(int64_t max_rows, int p) { return dlsa_cox_ties_workspace_bytes(max_rows, p, DLSA_COX_TIES_BRESLOW); }

int dlsa_cox_pass_strata_f64(const double* X, int64_t ldx, const double* time, const double* event, const int32_t* strata,
                             const int64_t* order, int64_t n, int p, int ties, const double* beta, double* H, int64_t ldh, double* g,
                             double* loglik, double* w_out, void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && time && event && order && beta && H, "cox_pass: null argument");
    DLSA_REQUIRE(n >= 1 && p > 0 && p <= 2048 && ldx >= p && ldh >= p, "cox_pass: bad shape n=%lld p=%d ldx=%lld ldh=%lld",
                 (long long)n, p, (long long)ldx, (long long)ldh);
    DLSA_REQUIRE(ties == DLSA_COX_TIES_BRESLOW || ties == DLSA_COX_TIES_EFRON, "cox_pass: unknown ties method %d", ties);
    const CoxWs w = cox_workspace((char*)ws, n, p, ties, strata != nullptr);
    // (the pass carves w.total of it; the contract is the query, which also holds a fit's Newton state)
    int rc = newton_check_ws("cox", ws, ws_bytes, dlsa_cox_strata_workspace_bytes(n, p, ties, strata ? 1 : 0));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    CoxRows rows;
    rc = cox_rows(order, n, w.misc, &rows, s);
    if (rc) return rc;
    rc = cox_strata_flags(strata, order, n, w, s);
    if (rc) return rc;
    int64_t D = 0;
    return cox_pass_impl(X, ldx, time, event, order, n, p, ties, rows, beta, H, ldh, g, loglik, w_out, w, &D, s);
}

int dlsa_cox_pass_ties_f64(const double* X, int64_t ldx, const double* time, const double* event, const int64_t* order, int64_t n,
                           int p, int ties, const double* beta, double* H, int64_t ldh, double* g, double* loglik, double* w_out,
                           void* ws, size_t ws_bytes, void* stream) {
    return dlsa_cox_pass_strata_f64(X, ldx, time, event, nullptr, order, n, p, ties, beta, H, ldh, g, loglik, w_out, ws, ws_bytes, stream);
}

int dlsa_cox_pass_f64(const double* X, int64_t ldx, const double* time, const double* event, const int64_t* order, int64_t n, int p,
                      const double* beta, double* H, int64_t ldh, double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes,
                      void* stream) {
    return dlsa_cox_pass_ties_f64(X, ldx, time, event, order, n, p, DLSA_COX_TIES_BRESLOW, beta, H, ldh, g, loglik, w_out, ws, ws_bytes,
                                  stream);
}

int dlsa_cox_fit_strata_f64(const double* X, int64_t ldx, const double* time, const double* event, const int32_t* strata,
                            const int64_t* order, const int64_t* part_offsets_host, int K, int p, int ties, double tol, int max_iter,
                            double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host,
                            void* ws, size_t ws_bytes, void* stream) {
    using namespace dlsa;
    DLSA_REQUIRE(X && time && event && order && part_offsets_host && coef && Sig_inv && Sig_invMcoef, "cox_fit: null argument");
    DLSA_REQUIRE(K > 0 && p > 0 && p <= 2048 && ldx >= p, "cox_fit: bad shape K=%d p=%d ldx=%lld", K, p, (long long)ldx);
    DLSA_REQUIRE(max_iter > 0 && tol > 0, "cox_fit: bad tol/max_iter");
    DLSA_REQUIRE(ties == DLSA_COX_TIES_BRESLOW || ties == DLSA_COX_TIES_EFRON, "cox_fit: unknown ties method %d", ties);
    int64_t max_rows = 0;
    for (int k = 0; k < K; ++k) {
        DLSA_REQUIRE(part_offsets_host[k] >= 0 && part_offsets_host[k + 1] >= part_offsets_host[k], "cox_fit: part_offsets must be non-decreasing from 0");
        max_rows = std::max(max_rows, part_offsets_host[k + 1] - part_offsets_host[k]);
    }
    const bool stratified = strata != nullptr;
    char* wsc = (char*)ws;
    const CoxWs w = cox_workspace(wsc, max_rows, p, ties, stratified);
    int rcw = newton_check_ws("cox_fit", ws, ws_bytes, dlsa_cox_strata_workspace_bytes(max_rows, p, ties, stratified ? 1 : 0));
    if (rcw) return rcw;
    hipStream_t s = (hipStream_t)stream;
    const NewtonState st = newton_state_at(wsc + align_up(w.total, 256), p);
    int overall = DLSA_OK;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = part_offsets_host[k + 1] - part_offsets_host[k];
        const int64_t* ok = order + part_offsets_host[k];
        double* Hk = Sig_inv + (size_t)k * p * p;
        NewtonOutcome o{DLSA_PART_EMPTY, 0, 0, 0.0};
        if (nk > 0) {
            CoxRows rows;
            int rc = cox_rows(ok, nk, w.misc, &rows, s);
            if (rc) return rc;
            rc = cox_strata_flags(strata, ok, nk, w, s);
            if (rc) return rc;
            DLSA_HIP_CHECK(hipMemsetAsync(st.beta, 0, (size_t)p * sizeof(double), s));
            const auto eval = [&](bool& nothing) {
                int64_t D = 0;
                const int rce = cox_pass_impl(X, ldx, time, event, ok, nk, p, ties, rows, st.beta, Hk, p, st.g, st.stats + 3, nullptr, w, &D, s);
                nothing = D == 0;                   // no event: nothing to fit
                return rce;
            };
            rc = newton_fit_loop(NEWTON_COX, tol, max_iter + 1, eval, NewtonDevice{st, Hk, p, s}, newton_no_hook, o);
            if (rc) return rc;
        }
        const int rc = newton_fit_finish(o.status, o.n_iter, o.ll, st.beta, p, Hk, coef + (size_t)k * p, Sig_invMcoef + (size_t)k * p, k,
                                         n_iter_host, status_host, loglik_host, overall, s);
        if (rc) return rc;
    }
    DLSA_HIP_CHECK(hipStreamSynchronize(s));
    return overall;
}

int dlsa_cox_fit_ties_f64(const double* X, int64_t ldx, const double* time, const double* event, const int64_t* order,
                          const int64_t* part_offsets_host, int K, int p, int ties, double tol, int max_iter, double* coef,
                          double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, void* ws,
                          size_t ws_bytes, void* stream) {
    return dlsa_cox_fit_strata_f64(X, ldx, time, event, nullptr, order, part_offsets_host, K, p, ties, tol, max_iter, coef, Sig_inv,
                                   Sig_invMcoef, n_iter_host, status_host, loglik_host, ws, ws_bytes, stream);
}

int dlsa_cox_fit_f64(const double* X, int64_t ldx, const double* time, const double* event, const int64_t* order,
                     const int64_t* part_offsets_host, int K, int p, double tol, int max_iter, double* coef, double* Sig_inv,
                     double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, void* ws, size_t ws_bytes,
                     void* stream) {
    return dlsa_cox_fit_ties_f64(X, ldx, time, event, order, part_offsets_host, K, p, DLSA_COX_TIES_BRESLOW, tol, max_iter, coef, Sig_inv,
                                 Sig_invMcoef, n_iter_host, status_host, loglik_host, ws, ws_bytes, stream);
}

}  // extern "C"
