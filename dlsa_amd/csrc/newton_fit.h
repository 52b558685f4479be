// The per-partition safeguarded Newton fit of the count and Cox models (poisson.hip, onehot_poisson.hip, negbin.hip, cox.hip):
// the state block, the judgement of an evaluation, the loop and the partition epilogue -- one copy each.  Host code only.
// DESIGN.md 4.6 "The Newton loop" holds the table of what the three policies do; the logistic driver (irls.hip: newton_run) has
// its own loop and takes only newton_overshot and NEWTON_MAX_HALVINGS from here.
#pragma once
#include "common.h"
#include "host_calls.h"
#include <math.h>
#include <algorithm>

namespace dlsa {

// ---- the state -----------------------------------------------------------------------------------------------------------
// stats[8] ([0] |delta|_inf, [1] |beta|_inf, [2] factor status, [3] the log-likelihood the evaluation left), beta, prev, delta,
// g (pe each), then the pe x pe Cholesky factor -- one block of newton_state_bytes(pe), carved by newton_state_at
struct NewtonState { double *stats, *beta, *prev, *delta, *g, *Lf; };
static inline size_t newton_state_bytes(int pe) {
    return align_up(8 * (size_t)(4 * pe + 8), 256) + align_up(8 * (size_t)pe * pe, 256);
}
static inline NewtonState newton_state_at(void* block, int pe) {
    double* st = (double*)block;
    return {st, st + 8, st + 8 + pe, st + 8 + 2 * pe, st + 8 + 3 * pe, (double*)((char*)block + align_up(8 * (size_t)(4 * pe + 8), 256))};
}

// a partition's status folded into the fit's return code: the first soft failure stands
static inline void newton_fold_status(int st_k, int& overall) {
    if (overall != DLSA_OK) return;
    if (st_k == DLSA_PART_NOT_CONVERGED) overall = DLSA_ERR_NOT_CONVERGED;
    if (st_k == DLSA_PART_NOT_SPD) overall = DLSA_ERR_NOT_SPD;
    if (st_k == DLSA_PART_NAN) overall = DLSA_ERR_NAN;
}

static inline int newton_check_ws(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 255)) {
        set_error("%s: workspace %zu bytes needed (256-aligned), got %zu", who, need, ws_bytes);
        return DLSA_ERR_WORKSPACE;
    }
    return DLSA_OK;
}

// ---- the judgement (plain C++, no HIP call) ------------------------------------------------------------------------------
constexpr int NEWTON_MAX_HALVINGS = 30;
// the previous step overshot: the likelihood dropped by more than its rounding
static inline bool newton_overshot(double ll, double ll_prev) { return ll < ll_prev - 1e-12 * fabs(ll_prev); }

// what differs between the model families beyond their callables (the columns of DESIGN.md's table)
struct NewtonPolicy {
    bool nan_at_once;          // a non-finite likelihood is NAN at once (Cox); else it counts as "worse" and is halved first
    bool advance_at_budget;    // the last permitted evaluation, accepted and not converged, still advances (NB2); else coef stays
                               // the evaluated iterate
};
constexpr NewtonPolicy NEWTON_POISSON{false, false}, NEWTON_NB2{false, true}, NEWTON_COX{true, false};

struct NewtonGuard { double ll_prev = -INFINITY; bool have_prev = false; int halvings = 0; };
enum NewtonVerdict { NEWTON_HALVE, NEWTON_STOP, NEWTON_ACCEPTED };

// h = [|delta|_inf, |beta|_inf, factor flag, ll] as read back after the solve.  HALVE: the step from gd's point is halved
// (counted in gd); STOP: the fit ends with `status`; ACCEPTED: the point stands (after NEWTON_MAX_HALVINGS halvings a point that
// is still worse but finite is accepted too), the halving counter restarts.
static inline NewtonVerdict newton_judge(const double h[4], NewtonGuard& gd, bool nan_at_once, int& status) {
    const double ll = h[3];
    if (nan_at_once && !isfinite(ll)) { status = DLSA_PART_NAN; return NEWTON_STOP; }
    const bool worse = !isfinite(ll) || (gd.have_prev && newton_overshot(ll, gd.ll_prev));
    if (gd.have_prev && worse && gd.halvings < NEWTON_MAX_HALVINGS) { ++gd.halvings; return NEWTON_HALVE; }
    if (!isfinite(ll)) { status = DLSA_PART_NAN; return NEWTON_STOP; }
    gd.halvings = 0;
    if (h[2] == 1.0) { status = DLSA_PART_NOT_SPD; return NEWTON_STOP; }
    if (h[2] == 2.0) { status = DLSA_PART_NAN; return NEWTON_STOP; }
    return NEWTON_ACCEPTED;
}

// ---- the loop --------------------------------------------------------------------------------------------------------------
// The loop's device calls on a NewtonState and the partition's H.  They are an argument of newton_fit_loop so that the test
// entry dlsa_newton_replay (newton_replay.cpp) drives the same loop from a script.
struct NewtonDevice {
    NewtonState st; double* H; int pe; hipStream_t s;
    int solve(double h[4]) const {                      // delta = H^-1 g, then the four doubles of stats
        const int rc = launch_chol_solve(H, pe, 0, st.g, 0, st.beta, 0, pe, 1, st.Lf, st.delta, 0, st.stats, 0, s, 0);
        if (rc) return rc;
        DLSA_HIP_CHECK(hipMemcpyAsync(h, st.stats, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        DLSA_HIP_CHECK(hipStreamSynchronize(s));
        return DLSA_OK;
    }
    int halve() const {
        int rc = launch_axpby(st.beta, st.prev, -1.0, pe, st.delta, s);      // delta = beta - prev
        if (rc) return rc;
        return launch_axpby(st.prev, st.delta, 0.5, pe, st.beta, s);         // beta = prev + delta / 2
    }
    int advance() const { return launch_advance(st.prev, st.beta, st.delta, pe, s); }
};

struct NewtonOutcome {
    int status;       // DLSA_PART_*
    int n_iter;       // evaluations up to and including the last accepted one
    int evals;        // evaluations made, whatever became of them
    double ll;        // the last likelihood read back
};

// At most `budget` evaluations (halved ones count).  eval(bool& nothing): H, g and the likelihood (stats[3]) at beta; nothing =
// true: the partition has nothing to fit (EMPTY, before any solve).  hook(bool& leave, double& first_step, double& ll_shift)
// runs after an accepted evaluation: leave ends the loop as it stands (NOT_CONVERGED, the caller deals with it), first_step
// (<= 100 tol) is a second condition of "converged", ll_shift moves this point's likelihood to where the next one is judged.
template <class Eval, class Dev, class Hook>
int newton_fit_loop(NewtonPolicy pol, double tol, int budget, Eval&& eval, Dev&& dev, Hook&& hook, NewtonOutcome& out) {
    NewtonGuard gd;
    out = NewtonOutcome{DLSA_PART_NOT_CONVERGED, 0, 0, 0.0};
    for (int it = 0; it < budget; ++it) {
        bool nothing = false;
        int rc = eval(nothing);
        if (rc) return rc;
        ++out.evals;
        if (nothing) { out.status = DLSA_PART_EMPTY; break; }
        double h[4];
        rc = dev.solve(h);
        if (rc) return rc;
        out.ll = h[3];
        int st = DLSA_PART_NOT_CONVERGED;
        const NewtonVerdict v = newton_judge(h, gd, pol.nan_at_once, st);
        if (v == NEWTON_HALVE) {
            // (kept as it was: a halving that uses the last permitted evaluation leaves an UNEVALUATED halved point in beta, with
            //  H and the likelihood of the rejected point)
            rc = dev.halve();
            if (rc) return rc;
            continue;
        }
        if (v == NEWTON_STOP) { out.status = st; break; }
        out.n_iter = it + 1;
        bool leave = false;
        double first_step = 0.0, ll_shift = 0.0;
        rc = hook(leave, first_step, ll_shift);
        if (rc) return rc;
        if (leave) break;
        if (h[0] <= tol * std::max(1.0, h[1]) && first_step <= 100.0 * tol) { out.status = DLSA_PART_OK; break; }     // H, g, ll are at beta
        // (kept as it was: with advance_at_budget the last evaluation's step is still taken, so coef is a point H was not evaluated at)
        if (it == budget - 1 && !pol.advance_at_budget) break;
        rc = dev.advance();
        if (rc) return rc;
        gd.ll_prev = h[3] + ll_shift;
        gd.have_prev = true;
    }
    return DLSA_OK;
}
static inline int newton_no_hook(bool&, double&, double&) { return DLSA_OK; }

// ---- the epilogue of a partition -----------------------------------------------------------------------------------------
// EMPTY: the zero block and loglik 0; else coef = beta and Sig_inv coef.  Then the host outputs (nullable) and the status fold.
static inline int newton_fit_finish(int status, int n_iter, double ll, const double* beta, int pe, double* Hk, double* ck, double* sk,
                                    int k, int* n_iter_host, int* status_host, double* loglik_host, int& overall, hipStream_t s) {
    if (status == DLSA_PART_EMPTY) {
        ll = 0.0;
        DLSA_HIP_CHECK(hipMemsetAsync(Hk, 0, (size_t)pe * pe * sizeof(double), s));
        DLSA_HIP_CHECK(hipMemsetAsync(ck, 0, (size_t)pe * sizeof(double), s));
        DLSA_HIP_CHECK(hipMemsetAsync(sk, 0, (size_t)pe * sizeof(double), s));
    } else {
        DLSA_HIP_CHECK(hipMemcpyAsync(ck, beta, (size_t)pe * sizeof(double), hipMemcpyDeviceToDevice, s));
        const int rc = launch_matvec(Hk, pe, beta, pe, sk, s);
        if (rc) return rc;
    }
    if (n_iter_host) n_iter_host[k] = n_iter;
    if (status_host) status_host[k] = status;
    if (loglik_host) loglik_host[k] = ll;
    newton_fold_status(status, overall);
    return DLSA_OK;
}

}  // namespace dlsa
