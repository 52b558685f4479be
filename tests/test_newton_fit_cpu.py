"""CPU: the safeguarded Newton loop of the Poisson, NB2 and Cox fits (csrc/newton_fit.h), driven through dlsa_newton_replay: the
loop the fits run, with callables that read a script of read-backs instead of launching kernels.  Every expectation below is
written out literally from the table in DESIGN.md 4.6 ("The Newton loop"); nothing is recomputed by a Python copy of the loop."""
import ctypes

import numpy as np
import pytest

POISSON, NB2, COX = 0, 1, 2
ALL = [POISSON, NB2, COX]
OK, NOT_CONVERGED, NOT_SPD, NAN, EMPTY = 0, 1, 2, 3, 4
H, A, S = 1, 2, 3                     # what followed an evaluation: halving, advance, stop (0: never evaluated)
TOL = 1e-8
BIG = (1.0, 1.0)                      # |delta|, |beta|: a step far above TOL max(1, |beta|)
SMALL = (1e-9, 1.0)                   # ... and one below it


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def replay(lib, policy, budget, rows, nothing=None, hook=None, tol=TOL):
    """rows: (|delta|, |beta|, factor flag, ll) per evaluation; hook: (first_step, ll_shift, fell) per evaluation (NB2).
    Returns (actions of the evaluations made, status, n_iter, advanced_last)."""
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rb = np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(-1, 4))
    nt = None if nothing is None else np.ascontiguousarray(np.array(nothing, dtype=np.int32))
    fs = sh = fl = None
    if hook is not None:
        fs = np.ascontiguousarray(np.array([h[0] for h in hook], dtype=np.float64))
        sh = np.ascontiguousarray(np.array([h[1] for h in hook], dtype=np.float64))
        fl = np.ascontiguousarray(np.array([h[2] for h in hook], dtype=np.int32))
    actions = np.full(budget, -1, dtype=np.int32)
    st, it, adv = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.dlsa_newton_replay(policy, tol, budget, len(rb), P(rb), P(nt), P(fs), P(sh), P(fl), P(actions), st, it, adv)
    assert rc == 0, rc
    made = [int(a) for a in actions if a != 0]
    assert list(actions[len(made):]) == [0] * (budget - len(made))          # nothing recorded beyond the last evaluation
    return made, st.value, it.value, bool(adv.value)


@pytest.mark.parametrize("policy", ALL)
def test_monotone_likelihood_converges_at_the_fourth_evaluation(lib, policy):
    rows = [BIG + (0, -10.0), BIG + (0, -5.0), BIG + (0, -2.0), SMALL + (0, -1.0)]
    assert replay(lib, policy, 10, rows) == ([A, A, A, S], OK, 4, False)


@pytest.mark.parametrize("policy", ALL)
def test_one_drop_is_halved_once_and_the_halved_evaluation_counts(lib, policy):
    rows = [BIG + (0, -10.0), BIG + (0, -12.0), BIG + (0, -8.0), SMALL + (0, -7.0)]
    assert replay(lib, policy, 10, rows) == ([A, H, A, S], OK, 4, False)


@pytest.mark.parametrize("policy", ALL)
def test_a_drop_within_rounding_of_the_previous_value_is_no_overshoot(lib, policy):
    # the predicate is ll < ll_prev - 1e-12 |ll_prev|: -10 - 5e-12 lies inside the band, -10 - 2e-11 outside
    assert replay(lib, policy, 10, [BIG + (0, -10.0), SMALL + (0, -10.0 - 5e-12)]) == ([A, S], OK, 2, False)
    assert replay(lib, policy, 10, [BIG + (0, -10.0), SMALL + (0, -10.0 - 2e-11), SMALL + (0, -9.0)]) == ([A, H, S], OK, 3, False)


@pytest.mark.parametrize("policy", ALL)
def test_thirty_halvings_then_the_worse_point_is_accepted(lib, policy):
    # evaluation 1 is accepted; 2 .. 31 are worse and halved (30 halvings); 32, the 31st worse point, is accepted and advanced
    # from, and its likelihood becomes the one to beat; 33 meets the step rule
    rows = [BIG + (0, -10.0)] + [BIG + (0, -20.0)] * 31 + [SMALL + (0, -20.0)]
    assert replay(lib, policy, 40, rows) == ([A] + [H] * 30 + [A, S], OK, 33, False)


@pytest.mark.parametrize("policy", ALL)
def test_a_halving_on_the_last_permitted_evaluation_ends_the_fit_unevaluated(lib, policy):
    # budget 5: the fit ends NOT_CONVERGED on a halving (beta holds a halved point that no pass evaluated: kept as it was)
    rows = [BIG + (0, -10.0)] + [BIG + (0, -20.0)] * 4
    # n_iter: Poisson and Cox report the last accepted evaluation (the first), NB2 its five row passes
    assert replay(lib, policy, 5, rows) == ([A, H, H, H, H], NOT_CONVERGED, 5 if policy == NB2 else 1, False)


@pytest.mark.parametrize("policy", ALL)
@pytest.mark.parametrize("bad", [float("nan"), float("-inf"), float("inf")])
def test_non_finite_likelihood_at_the_first_evaluation_is_nan(lib, policy, bad):
    # no previous point to halve towards: NAN for every family
    assert replay(lib, policy, 10, [BIG + (0, bad)]) == ([S], NAN, 1 if policy == NB2 else 0, False)


@pytest.mark.parametrize("bad", [float("nan"), float("-inf")])
def test_non_finite_likelihood_at_the_third_evaluation(lib, bad):
    rows = [BIG + (0, -10.0), BIG + (0, -8.0), BIG + (0, bad), SMALL + (0, -7.0)]
    for policy in (POISSON, NB2):          # counts as "worse": halved, then the halved point converges
        assert replay(lib, policy, 10, rows) == ([A, A, H, S], OK, 4, False)
    # Cox: NAN at once, after three evaluations, two of them accepted
    assert replay(lib, COX, 10, rows) == ([A, A, S], NAN, 2, False)


@pytest.mark.parametrize("policy", ALL)
def test_non_finite_likelihood_after_thirty_halvings_is_nan(lib, policy):
    rows = [BIG + (0, -10.0)] + [BIG + (0, -20.0)] * 30 + [BIG + (0, float("nan"))]
    # Poisson and NB2 have no halving left for it, Cox never halves it
    assert replay(lib, policy, 40, rows) == ([A] + [H] * 30 + [S], NAN, 32 if policy == NB2 else 1, False)


@pytest.mark.parametrize("policy", ALL)
def test_factor_flags(lib, policy):
    evals = lambda n_acc, n_all: n_all if policy == NB2 else n_acc
    # on a fresh point: flag 1 is NOT_SPD, flag 2 is NAN
    assert replay(lib, policy, 10, [BIG + (1, -10.0)]) == ([S], NOT_SPD, evals(0, 1), False)
    assert replay(lib, policy, 10, [BIG + (2, -10.0)]) == ([S], NAN, evals(0, 1), False)
    # on a later point that is no worse than the previous one
    assert replay(lib, policy, 10, [BIG + (0, -10.0), BIG + (1, -9.0)]) == ([A, S], NOT_SPD, evals(1, 2), False)
    assert replay(lib, policy, 10, [BIG + (0, -10.0), BIG + (2, -9.0)]) == ([A, S], NAN, evals(1, 2), False)
    # on a point that is also worse the halving wins, and the flag of the halved point decides
    assert replay(lib, policy, 10, [BIG + (0, -10.0), BIG + (1, -12.0), SMALL + (0, -9.0)]) == ([A, H, S], OK, 3, False)
    assert replay(lib, policy, 10, [BIG + (0, -10.0), BIG + (2, -12.0), BIG + (1, -9.0)]) == ([A, H, S], NOT_SPD, evals(1, 3), False)


def test_budget_used_up_on_an_accepted_point(lib):
    rows = [BIG + (0, -10.0), BIG + (0, -5.0), BIG + (0, -2.0)]
    for policy in (POISSON, COX):          # stop before advancing: coef is the evaluated iterate
        assert replay(lib, policy, 3, rows) == ([A, A, S], NOT_CONVERGED, 3, False)
    # NB2 advances after its last evaluation (kept as it was)
    assert replay(lib, NB2, 3, rows) == ([A, A, A], NOT_CONVERGED, 3, True)
    assert replay(lib, NB2, 3, rows, hook=[(0.0, 0.0, 0)] * 3) == ([A, A, A], NOT_CONVERGED, 3, True)


def test_nb2_dispersion_hook(lib):
    # the step rule holds at evaluation 2 but the dispersion moved by more than 100 tol: not converged until it stands still
    rows = [BIG + (0, -10.0), SMALL + (0, -9.0), SMALL + (0, -8.5)]
    assert replay(lib, NB2, 10, rows, hook=[(0.5, 0.0, 0), (101 * TOL, 0.0, 0), (0.0, 0.0, 0)]) == ([A, A, S], OK, 3, False)
    assert replay(lib, NB2, 10, rows, hook=[(0.5, 0.0, 0), (100 * TOL, 0.0, 0), (0.0, 0.0, 0)]) == ([A, S], OK, 2, False)
    # "fell to Poisson" after evaluation 2: the loop ends as it stands, NOT_CONVERGED, no advance
    assert replay(lib, NB2, 10, rows, hook=[(0.5, 0.0, 0), (0.5, 0.0, 1), (0.0, 0.0, 0)]) == ([A, S], NOT_CONVERGED, 2, False)
    # the likelihood to beat is the accepted one moved to the new alpha: -10 - 5 = -15, so -12 is no overshoot; unmoved it is
    rows = [BIG + (0, -10.0), SMALL + (0, -12.0), SMALL + (0, -9.0)]
    assert replay(lib, NB2, 10, rows, hook=[(0.5, -5.0, 0), (0.0, 0.0, 0), (0.0, 0.0, 0)]) == ([A, S], OK, 2, False)
    assert replay(lib, NB2, 10, rows, hook=[(0.5, 0.0, 0), (0.0, 0.0, 0), (0.0, 0.0, 0)]) == ([A, H, S], OK, 3, False)
    # a hook is not run on a halved or a failed evaluation: "fell" scripted there changes nothing
    rows = [BIG + (0, -10.0), BIG + (0, -12.0), BIG + (1, -9.0)]
    assert replay(lib, NB2, 10, rows, hook=[(0.5, 0.0, 0), (0.5, 0.0, 1), (0.5, 0.0, 1)]) == ([A, H, S], NOT_SPD, 3, False)


def test_cox_nothing_to_fit_is_empty_before_the_solve(lib):
    # the read-back of evaluation 1 is poison: were it judged, the status would be NAN
    nan = float("nan")
    assert replay(lib, COX, 10, [(nan, nan, 2, nan)], nothing=[1]) == ([S], EMPTY, 0, False)
    assert replay(lib, COX, 10, [BIG + (0, -10.0), (nan, nan, 2, nan)], nothing=[0, 1]) == ([A, S], EMPTY, 1, False)


def test_replay_checks_its_arguments(lib):
    from dlsa_amd import _lib
    rb = np.array([BIG + (0, -10.0)], dtype=np.float64)
    one = np.zeros(4, dtype=np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    st, it, adv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    call = lambda policy, budget=4, n=1, nothing=None, fs=None: lib.dlsa_newton_replay(policy, TOL, budget, n, P(rb), nothing, fs, None, None,
                                                                                    P(one), st, it, adv)
    assert call(3) == 1 and "policy 3" in _lib.last_error()
    assert call(POISSON, budget=0) == 1
    assert call(POISSON, nothing=P(one)) == 1 and "Cox" in _lib.last_error()
    assert call(NB2, fs=P(rb)) == 1 and "come together" in _lib.last_error()
    assert call(POISSON) == 1 and "ran out" in _lib.last_error()           # one scripted evaluation, and the loop advances
