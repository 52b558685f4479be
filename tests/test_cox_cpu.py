"""CPU checks of the Cox map step: the numpy Breslow reference checks itself (finite differences, both forms agree, the
score vanishes at its MLE), and the C ABI validates its arguments before any HIP call."""
import ctypes

import numpy as np
import pytest

import cox_reference as cr


def _data(seed, n, p, ties=None, censor=0.3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    t = rng.exponential(1.0, n) / np.exp(X @ (np.arange(p) % 3 - 1) * 0.3)
    if ties:
        t = np.round(t * ties) / ties
    ev = (rng.random(n) > censor).astype(np.float64)
    return X, t, ev


def test_reference_finite_differences():
    X, t, ev = _data(1, 120, 4, ties=5)
    b = np.array([0.2, -0.1, 0.3, 0.05])
    ll, U, H = cr.breslow_loop(X, t, ev, b)
    h = 1e-6
    for j in range(4):
        e = np.zeros(4); e[j] = h
        lp, Up, _ = cr.breslow_loop(X, t, ev, b + e)
        lm, Um, _ = cr.breslow_loop(X, t, ev, b - e)
        assert abs((lp - lm) / (2 * h) - U[j]) <= 1e-6 * max(1.0, abs(U[j]))
        assert np.max(np.abs((Up - Um) / (2 * h) + H[:, j])) <= 1e-6 * max(1.0, np.max(np.abs(H)))


@pytest.mark.parametrize("ties", [None, 3, 20])
def test_reference_forms_agree(ties):
    X, t, ev = _data(2, 400, 6, ties=ties)
    b = np.linspace(-0.4, 0.4, 6)
    l1, U1, H1 = cr.breslow_loop(X, t, ev, b)
    l2, U2, H2 = cr.breslow_cumsum(X, t, ev, b)
    assert abs(l1 - l2) <= 1e-13 * abs(l1)
    assert np.max(np.abs(U1 - U2)) <= 1e-13 * np.abs(X).sum(0).max()
    assert np.max(np.abs(H1 - H2)) <= 1e-13 * np.max(np.abs(H1))


def test_reference_score_vanishes_at_mle():
    X, t, ev = _data(3, 500, 5, ties=10)
    beta, H, _ = cr.fit(X, t, ev)
    _, U, _ = cr.breslow_loop(X, t, ev, beta)
    assert np.max(np.abs(U)) <= 1e-11 * np.abs(X).sum(0).max()
    assert np.all(np.linalg.eigvalsh(H) > 0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def test_abi_rejects_bad_arguments(lib):
    from dlsa_amd import _lib
    fake = ctypes.c_void_p(256)
    # pass: null pointers, n < 1, p out of range, ldx < p
    args = [fake, 4, fake, fake, fake, 10, 4, fake, fake, 4, None, None, None, fake, 1 << 20, None]
    for i in (0, 2, 3, 4, 7, 8):
        a = list(args); a[i] = None
        assert lib.dlsa_cox_pass_f64(*a) == 1
    assert "null" in _lib.last_error()
    for i, v in ((5, 0), (6, 0), (6, 4096), (1, 3), (9, 3)):
        a = list(args); a[i] = v
        assert lib.dlsa_cox_pass_f64(*a) == 1
    # fit: null pointers, K < 1, bad tol / max_iter, decreasing offsets
    offs = (ctypes.c_int64 * 3)(0, 5, 10)
    fargs = [fake, 4, fake, fake, fake, offs, 2, 4, 1e-13, 100, fake, fake, fake, None, None, None, fake, 1 << 20, None]
    for i in (0, 2, 3, 4, 5, 10, 11, 12):
        a = list(fargs); a[i] = None
        assert lib.dlsa_cox_fit_f64(*a) == 1
    for i, v in ((6, 0), (7, 0), (8, 0.0), (9, 0), (1, 2)):
        a = list(fargs); a[i] = v
        assert lib.dlsa_cox_fit_f64(*a) == 1
    a = list(fargs); a[5] = (ctypes.c_int64 * 3)(0, 6, 5)
    assert lib.dlsa_cox_fit_f64(*a) == 1


def test_workspace_query_is_monotone(lib):
    assert lib.dlsa_cox_workspace_bytes(100, 0) == 0
    assert lib.dlsa_cox_workspace_bytes(-1, 5) == 0
    for p in (1, 5, 100, 500):
        prev = 0
        for n in (0, 1, 63, 64, 65, 1000, 4096 * 64, 4096 * 64 + 1, 10 ** 6, 10 ** 7):
            b = lib.dlsa_cox_workspace_bytes(n, p)
            assert b >= prev, (p, n)
            prev = b
