"""CPU checks of Efron's approximation in the Cox map step: the numpy reference (tests/cox_efron_reference.py) checks itself
(both forms agree, Breslow on untied data, a hand case, finite differences), the tied inputs of the GPU tests separate the
two methods (so that a Breslow kernel cannot pass them), and the C ABI validates the tie method before any HIP call."""
import ctypes

import numpy as np
import pytest

import cox_efron_cases as cases
import cox_efron_reference as er
import cox_reference as cr


def _data(seed, n, p, ties=None, censor=0.3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    t = rng.exponential(1.0, n) / np.exp(X @ (np.arange(p) % 3 - 1) * 0.3)
    if ties:
        t = np.round(t * ties) / ties
    ev = (rng.random(n) > censor).astype(np.float64)
    return X, t, ev


def _agree(a, b, X, tol):
    (l1, U1, H1), (l2, U2, H2) = a, b
    assert abs(l1 - l2) <= tol * abs(l1), (l1, l2)
    assert np.max(np.abs(U1 - U2)) <= tol * np.abs(X).sum(0).max()
    assert np.max(np.abs(H1 - H2)) <= tol * np.max(np.abs(H1))


@pytest.mark.parametrize("ties", [3, 20])
def test_reference_forms_agree_on_tied_data(ties):
    X, t, ev = _data(2, 400, 6, ties=ties)
    b = np.linspace(-0.4, 0.4, 6)
    _agree(er.efron_loop(X, t, ev, b), er.efron_cumsum(X, t, ev, b), X, 1e-12)


def test_reference_forms_agree_with_one_group_over_all_rows():
    X, t, ev = _data(4, 300, 3)
    t[:] = 2.0
    b = np.array([0.3, -0.2, 0.1])
    _agree(er.efron_loop(X, t, ev, b), er.efron_cumsum(X, t, ev, b), X, 1e-12)


def test_efron_is_breslow_on_untied_data():
    X, t, ev = _data(5, 400, 6)
    assert len(np.unique(t)) == len(t)
    b = np.linspace(-0.4, 0.4, 6)
    ref = cr.breslow_loop(X, t, ev, b)
    _agree(ref, er.efron_loop(X, t, ev, b), X, 1e-13)
    _agree(ref, er.efron_cumsum(X, t, ev, b), X, 1e-13)


def test_hand_case():
    """three rows at risk, scalar x, two tied events, beta = 0: the risk sums are 3 and 3 - (1/2) 2 = 2"""
    X = np.array([[0.7], [-0.2], [1.5]])
    t = np.array([1.0, 1.0, 2.0])
    ev = np.array([1.0, 1.0, 0.0])
    for form in (er.efron_loop, er.efron_cumsum):
        ll, U, H = form(X, t, ev, np.zeros(1))
        assert abs(ll - (-np.log(3.0) - np.log(2.0))) <= 1e-15
        # z_0 = mean of all three, z_1 = (sum x - (x_0 + x_1) / 2) / 2
        z0, z1 = X.sum() / 3, (X.sum() - 0.5 * (X[0, 0] + X[1, 0])) / 2
        assert abs(U[0] - (X[0, 0] + X[1, 0] - z0 - z1)) <= 1e-15
        s2 = (X ** 2).sum()
        h = s2 / 3 - z0 ** 2 + (s2 - 0.5 * (X[0, 0] ** 2 + X[1, 0] ** 2)) / 2 - z1 ** 2
        assert abs(H[0, 0] - h) <= 1e-15


def test_reference_finite_differences():
    X, t, ev = _data(1, 120, 4, ties=5)
    b = np.array([0.2, -0.1, 0.3, 0.05])
    ll, U, H = er.efron_loop(X, t, ev, b)
    h = 1e-6
    for j in range(4):
        e = np.zeros(4); e[j] = h
        lp, Up, _ = er.efron_loop(X, t, ev, b + e)
        lm, Um, _ = er.efron_loop(X, t, ev, b - e)
        assert abs((lp - lm) / (2 * h) - U[j]) <= 1e-6 * max(1.0, abs(U[j]))
        assert np.max(np.abs((Up - Um) / (2 * h) + H[:, j])) <= 1e-6 * max(1.0, np.max(np.abs(H)))


def test_reference_score_vanishes_at_mle():
    X, t, ev = _data(3, 500, 5, ties=10)
    beta, H, _ = er.fit(X, t, ev)
    _, U, _ = er.efron_loop(X, t, ev, beta)
    assert np.max(np.abs(U)) <= 1e-11 * np.abs(X).sum(0).max()
    assert np.all(np.linalg.eigvalsh(H) > 0)


def _separated(X, t, ev, beta):
    form_e, form_b = (er.efron_loop, cr.breslow_loop) if len(t) <= 2000 else (er.efron_cumsum, cr.breslow_cumsum)
    le, _, He = form_e(X, t, ev, beta)
    lb, _, Hb = form_b(X, t, ev, beta)
    return abs(le - lb) / abs(lb), np.max(np.abs(He - Hb)) / np.max(np.abs(Hb))


@pytest.mark.parametrize("p", [1, 50, 500])
@pytest.mark.parametrize("n", [7, 300, 5000])
def test_gpu_pass_inputs_separate_efron_from_breslow(p, n):
    """the condition behind the GPU pass test: on its tied inputs the two methods differ by far more than its bar
    (a single row, n = 1, has no ties and is left out)"""
    dl, dH = _separated(*cases.pass_case(p, n))
    assert dl > 1e-4 and dH > 1e-4, (dl, dH)


@pytest.mark.parametrize("case", ["all_tied", "no_censoring", "pairs", "eta_range"])
def test_gpu_edge_inputs_separate_efron_from_breslow(case):
    dl, dH = _separated(*cases.edge_case(case))
    assert dl > 1e-4 and dH > 1e-4, (dl, dH)


def test_pairs_case_is_pairs():
    _, t, _, _ = cases.edge_case("pairs")
    assert np.all(np.unique(t, return_counts=True)[1] == 2)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def test_abi_rejects_unknown_tie_methods(lib):
    from dlsa_amd import _lib
    fake = ctypes.c_void_p(256)
    args = [fake, 4, fake, fake, fake, 10, 4, 0, fake, fake, 4, None, None, None, fake, 1 << 20, None]
    offs = (ctypes.c_int64 * 3)(0, 5, 10)
    fargs = [fake, 4, fake, fake, fake, offs, 2, 4, 0, 1e-13, 100, fake, fake, fake, None, None, None, fake, 1 << 20, None]
    for bad in (7, -1, 2):
        a = list(args); a[7] = bad
        assert lib.dlsa_cox_pass_ties_f64(*a) == 1
        assert "ties" in _lib.last_error()
        a = list(fargs); a[8] = bad
        assert lib.dlsa_cox_fit_ties_f64(*a) == 1
        assert "ties" in _lib.last_error()
        assert lib.dlsa_cox_ties_workspace_bytes(1000, 5, bad) == 0
    # the other argument checks are those of the Breslow entries
    for ties in (0, 1):
        a = list(args); a[7] = ties; a[0] = None
        assert lib.dlsa_cox_pass_ties_f64(*a) == 1 and "null" in _lib.last_error()
        a = list(fargs); a[8] = ties; a[6] = 0
        assert lib.dlsa_cox_fit_ties_f64(*a) == 1


def test_ties_workspace_query(lib):
    for p in (1, 5, 100, 500):
        prev = 0
        for n in (0, 1, 63, 64, 65, 1000, 4096 * 64, 4096 * 64 + 1, 10 ** 6, 10 ** 7):
            b0, b1 = lib.dlsa_cox_ties_workspace_bytes(n, p, 0), lib.dlsa_cox_ties_workspace_bytes(n, p, 1)
            assert b0 == lib.dlsa_cox_workspace_bytes(n, p)
            # Efron: the T segment arrays and one more array per position
            assert b1 >= b0 + 8 * max(n, 1) + 2 * 8 * 4096 * (p + 1)
            assert b1 >= prev, (p, n)
            prev = b1


def test_python_rejects_unknown_tie_methods_before_any_gpu_work():
    import pandas as pd
    import torch
    import dlsa_amd
    from dlsa_amd import engine
    assert engine.cox_ties("Efron") == 1 and engine.cox_ties("BRESLOW") == 0
    x = torch.zeros(4, 2, dtype=torch.float64)          # (CPU tensors: the name is checked first)
    for bad in ("exact", "", None, 1):
        with pytest.raises(ValueError, match="ties"):
            engine.cox_pass(x, x[:, 0], x[:, 0], torch.arange(4), x[0], ties=bad)
        with pytest.raises(ValueError, match="ties"):
            engine.cox_fit(x, x[:, 0], x[:, 0], torch.arange(4), [0, 4], ties=bad)
        with pytest.raises(ValueError, match="ties"):
            dlsa_amd.fit_cox_partitions(x, x[:, 0], x[:, 0], ties=bad)
        with pytest.raises(ValueError, match="ties"):
            dlsa_amd.cox_model(pd.DataFrame({"time": [1.0], "event": [1.0], "x0": [0.5]}), "time", "event", ties=bad)
