// dlsa_newton_replay (a test entry): the Newton loop of the count and Cox fits (newton_fit.h: newton_fit_loop) driven by a script
// of read-backs instead of a device.  The loop is the one the fits run; only its callables differ.  No HIP call.
#include "common.h"
#include "newton_fit.h"

namespace dlsa {

struct ReplayDevice {
    const double* readback; int* actions; int evals;      // evals: evaluations made so far
    int solve(double h[4]) const {
        for (int i = 0; i < 4; ++i) h[i] = readback[4 * (size_t)(evals - 1) + i];
        return DLSA_OK;
    }
    int halve() const { actions[evals - 1] = DLSA_NEWTON_HALVE; return DLSA_OK; }
    int advance() const { actions[evals - 1] = DLSA_NEWTON_ADVANCE; return DLSA_OK; }
};

}  // namespace dlsa

extern "C" int dlsa_newton_replay(int policy, double tol, int budget, int n_script, const double* readback, const int* nothing,
                                  const double* first_step, const double* ll_shift, const int* fell, int* actions, int* status,
                                  int* n_iter, int* advanced_last) {
    using namespace dlsa;
    DLSA_REQUIRE(policy >= DLSA_NEWTON_POLICY_POISSON && policy <= DLSA_NEWTON_POLICY_COX, "newton_replay: unknown policy %d", policy);
    DLSA_REQUIRE(tol > 0 && budget > 0 && n_script > 0 && readback && actions && status && n_iter && advanced_last,
                 "newton_replay: null argument, or tol, budget or n_script not positive");
    const bool nb2 = policy == DLSA_NEWTON_POLICY_NB2;
    DLSA_REQUIRE(nb2 ? ((first_step != nullptr) == (ll_shift != nullptr) && (first_step != nullptr) == (fell != nullptr))
                     : (!first_step && !ll_shift && !fell),
                 "newton_replay: first_step, ll_shift and fell come together, with the NB2 policy only");
    DLSA_REQUIRE(policy == DLSA_NEWTON_POLICY_COX || !nothing, "newton_replay: only the Cox policy knows \"nothing to fit\"");
    const NewtonPolicy pol = nb2 ? NEWTON_NB2 : policy == DLSA_NEWTON_POLICY_COX ? NEWTON_COX : NEWTON_POISSON;
    for (int i = 0; i < budget; ++i) actions[i] = DLSA_NEWTON_NOT_REACHED;
    ReplayDevice dev{readback, actions, 0};
    bool ran_out = false;
    const auto eval = [&](bool& none) {
        if (dev.evals == n_script) { ran_out = true; return (int)DLSA_ERR_INVALID; }
        actions[dev.evals] = DLSA_NEWTON_STOP;       // until a halving or an advance follows this evaluation
        none = nothing && nothing[dev.evals];
        ++dev.evals;
        return (int)DLSA_OK;
    };
    const auto hook = [&](bool& leave, double& fs, double& shift) {
        if (!first_step) return (int)DLSA_OK;
        fs = first_step[dev.evals - 1]; shift = ll_shift[dev.evals - 1]; leave = fell[dev.evals - 1] != 0;
        return (int)DLSA_OK;
    };
    NewtonOutcome o;
    const int rc = newton_fit_loop(pol, tol, budget, eval, dev, hook, o);
    if (ran_out) set_error("newton_replay: the script of %d evaluations ran out", n_script);
    if (rc) return rc;
    *status = o.status;
    *n_iter = nb2 ? o.evals : o.n_iter;              // what each family reports: NB2 its row passes
    *advanced_last = actions[o.evals - 1] == DLSA_NEWTON_ADVANCE;
    return DLSA_OK;
}
