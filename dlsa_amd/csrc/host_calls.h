// The prototypes of the host functions one translation unit of the library calls in another.  The library is built without
// relocatable device code, so a kernel is launched by the file that defines it and the other files reach it through these HOST
// functions.  A caller includes this header instead of retyping a prototype, and so does the defining file: the compiler then holds
// the definition against the prototype, where the linker (-Wl,--no-undefined) would only have compared names.  Grouped by the
// defining file.
// NOT yet on this header: gram.hip, gram_wide / narrow / cyclic / plan.hip, logit.hip, irls_pass.hip, irls_wide.hip and
// onehot_plan.h.  The committed counter evidence under profiles/ is keyed to a hash of those files' text
// (tests/test_bench_cpu.py), so they change together with a new set of profiles; until then they keep the prototypes they type
// themselves (what they call in each other, and their copies of gram_impl_f64, gram_workspace_bytes_impl, logit_pass_impl,
// logit_workspace_bytes_impl and logit_finish_launch), and their definitions are not checked against this header.
// (Headers that already are the one declaration of their unit's functions stay: onehot_plan.h for onehot.hip, lars.h, options.h,
//  gram_plan.h, and poisson_internal.h for poisson.hip.)
#pragma once
#include "common.h"
#include "irls_batch.h"     // FusedSlab

namespace dlsa {

// ---- gram.hip ----------------------------------------------------------------------------------------------------------
int gram_impl_f64(const double* X, int64_t ldx, const double* w, int64_t n, int p, double* H, int64_t ldh,
                  int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);
size_t gram_workspace_bytes_impl(int64_t n, int p, int elem_bytes);

// ---- logit.hip ---------------------------------------------------------------------------------------------------------
size_t logit_workspace_bytes_impl(int64_t n, int p);
// intercept != 0: beta and g have p + 1 entries, [intercept | the p columns of X]; X itself has p columns
int logit_pass_impl(const double* X, int64_t ldx, const double* y, const double* beta, int64_t n, int p,
                    double* w_out, double* g, double* loglik, void* ws, size_t ws_bytes, hipStream_t stream, int intercept);
bool logit_border_ok(const double* X, int64_t ldx, int p);
int logit_pass_border_impl(const double* X, int64_t ldx, const double* y, const double* beta, int64_t n, int p,
                           double* w_out, double* g, double* loglik, double* border, void* ws, size_t ws_bytes, hipStream_t stream);
// g[j] = sum_b gpart[b][j], loglik = sum_b llpart[b] in a fixed order: the finish step of the dense logit pass, shared by the
// one-hot and the count-model row passes
void logit_finish_launch(const double* gpart, const double* llpart, int nblocks, int pitch, int p, double* g,
                         double* loglik, hipStream_t stream, const double* s0part, double* s0);
int xtv_impl(const double* X, int64_t ldx, const double* v, int64_t n, int p, double* g, double* vv, double* sv,
             void* ws, size_t ws_bytes, hipStream_t s);

// ---- irls.hip ----------------------------------------------------------------------------------------------------------
// H = [1 | X]' diag(w) [1 | X]; border: [sum w | X'w] where the pass that produced w left it (null: a pass of its own)
int gram_icpt_impl(const double* X, int64_t ldx, const double* w, int64_t n, int p, double* H, int64_t ldh,
                   void* ws, size_t ws_bytes, hipStream_t s, const double* border = nullptr);

// ---- irls_pass.hip: one Newton pass in one launch where the shape allows it (narrow designs: the rows staged for the MFMAs
// also feed the logistic terms -- one read of X per fresh Hessian instead of two), and its batched form ------------------------
bool irls_pass_fused_eligible(const double* X, int64_t ldx, const double* y, int64_t n, int p);
size_t irls_pass_workspace_bytes_impl(int64_t n, int p);
bool irls_pass_fused_icpt_eligible(const double* X, int64_t ldx, const double* y, int64_t n, int p);
int irls_pass_icpt_impl(const double* X, int64_t ldx, const double* y, const double* beta, int64_t n, int p, double* H, int64_t ldh,
                        double* g, double* loglik, double* w_out, void* ws, size_t ws_bytes, hipStream_t stream);
int irls_pass_impl(const double* X, int64_t ldx, const double* y, const double* beta, int64_t n, int p, double* H, int64_t ldh,
                   double* g, double* loglik, double* w_out, double* w_scratch, void* ws, size_t ws_bytes, hipStream_t stream,
                   int* fused_out);
int irls_pass_batched_pp(int p);
int irls_pass_batched_gp(int p);
int irls_pass_batched_ll_at(int p);
bool irls_pass_batched_shape_ok(const double* X, int64_t ldx, const double* y, int p, int intercept, int64_t base_ldx);
int irls_pass_batched_launch(const double* X, int64_t ldx, const double* y, const double* beta, int64_t beta_stride, int p, int intercept,
                             const FusedSlab* d_slabs, int nslab, const int* d_active, double* partial, double* gpart,
                             unsigned long long* clk, hipStream_t stream, int want_h);

// ---- irls_small.hip: all partitions in ONE launch, a workgroup each (many small partitions) ---------------------------------
bool irls_small_eligible(const int64_t* rows_host, int K, int pe, double* est_ms = nullptr);
size_t irls_small_workspace_bytes(int K);
int irls_small_fit(const double* X, int64_t ldx, const double* y, const int64_t* first_host, const int64_t* rows_host,
                   int64_t step, int K, int p, int intercept, double tol, int max_iter, double* coef, double* Sig_inv,
                   double* Sig_invMcoef, int* n_iter_host, int* status_host, double* loglik_host, void* ws, size_t ws_bytes,
                   hipStream_t s);

// ---- irls_wide.hip: the logit pass of a wide design that also yields the partition's own Hessian in reduced precision --------
bool irls_wide_eligible(const double* X, int64_t ldx, int64_t n, int p, int icpt);
size_t irls_wide_workspace_bytes(int64_t n, int p, int icpt);
int irls_wide_pass_impl(const double* X, int64_t ldx, const double* y, const double* beta, int64_t n, int p, int icpt, double* w_out,
                        double* g, double* loglik, double* Happrox, int64_t ldh, void* ws, size_t ws_bytes, hipStream_t stream);

// ---- irls_batch.hip: the lock-step fit of all partitions of a call together -------------------------------------------------
bool irls_batched_eligible(const double* X, int64_t ldx, const double* y, const int64_t* rows_host, int K, int p, int intercept, int64_t row_step,
                           double* est_ms = nullptr);
int irls_batched_fit(const double* X, int64_t ldx, const double* y, const int64_t* first_host, const int64_t* rows_host, int64_t row_step, int K,
                     int p, int intercept, double tol, int max_iter, double* coef, double* Sig_inv, double* Sig_invMcoef, int* n_iter_host, int* status_host,
                     double* loglik_host, hipStream_t stream);

// ---- chol.hip ----------------------------------------------------------------------------------------------------------
// the Newton-step solve: delta = A^-1 rhs, stats[0] = |delta|_inf, [1] = |ref|_inf, [2] = the factor status (0 fine, 1 not SPD, 2 NaN)
int launch_chol_solve(const double* A, int64_t lda, int64_t strideA, const double* rhs, int64_t stride_rhs,
                      const double* ref, int64_t stride_ref, int p, int nsys, double* Lws, double* xout,
                      int64_t stride_x, double* stats, int64_t stride_stats, hipStream_t s, int reuse_factor);
bool chol_small_ok(int p);
int launch_chol_small(const double* A, int64_t lda, int p, const double* rhs, const double* ref, double* Hinv, double* xout,
                      double* stats, hipStream_t s);
int launch_chol_small_batched(int count, const double* A, int64_t lda, int64_t sA, int p, const double* rhs, const double* ref, int64_t sV,
                              double* Hinv, int64_t sH, double* xout, double* stats, int64_t sS, const int* active, hipStream_t s);
int launch_tri_inverse(const double* L, int p, double* Linv, hipStream_t s);
int launch_inv_apply(const double* Linv, int p, const double* rhs, const double* ref, double* xout, double* stats, hipStream_t s);

// ---- dense.hip ---------------------------------------------------------------------------------------------------------
int launch_matvec(const double* A, int64_t lda, const double* x, int p, double* y, hipStream_t s);                        // y = A x
int launch_matvec_axpy(const double* A, int64_t lda, const double* x, int p, double alpha, const double* z, double beta, double* y, hipStream_t s);
int launch_step_stats(const double* delta, const double* ref, int p, double* stats, hipStream_t s);
int launch_axpby(const double* a, const double* b, double sc, int n, double* out, hipStream_t s);                         // out = a + sc b
int launch_advance(double* prev, double* beta, const double* delta, int n, hipStream_t s);                                // prev = beta, beta += delta

}  // namespace dlsa
