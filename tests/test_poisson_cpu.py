"""CPU checks of the Poisson map step: the numpy reference checks itself (finite differences, a zero score at its MLE, agreement
with scikit-learn's Newton solver), and the C ABI validates its arguments before any HIP call."""
import ctypes

import numpy as np
import pytest

import poisson_reference as pr


def _data(seed, n, p, intercept=True, offset=True):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.linspace(-0.6, 0.6, p)
    o = rng.uniform(-0.5, 0.5, n) if offset else None
    eta = X @ beta + (0.3 if intercept else 0.0) + (0.0 if o is None else o)
    y = rng.poisson(np.exp(eta)).astype(np.float64)
    return X, y, o


@pytest.mark.parametrize("intercept,offset", [(False, False), (True, False), (True, True), (False, True)])
def test_reference_finite_differences(intercept, offset):
    X, y, o = _data(1, 200, 4, intercept, offset)
    pe = 4 + intercept
    b = np.linspace(-0.3, 0.4, pe)
    ll, g, H, mu = pr.terms(X, y, b, o, intercept)
    assert np.allclose(mu, np.exp(pr.design(X, intercept) @ b + (0 if o is None else o)))
    h = 1e-6
    for j in range(pe):
        e = np.zeros(pe); e[j] = h
        lp, gp, _, _ = pr.terms(X, y, b + e, o, intercept)
        lm, gm, _, _ = pr.terms(X, y, b - e, o, intercept)
        assert abs((lp - lm) / (2 * h) - g[j]) <= 1e-6 * max(1.0, abs(g[j]))
        assert np.max(np.abs((gp - gm) / (2 * h) + H[:, j])) <= 1e-6 * max(1.0, np.max(np.abs(H)))


def test_reference_score_vanishes_at_mle():
    X, y, o = _data(2, 2000, 6)
    b, H, ll = pr.fit(X, y, o, True)
    l2, g, H2, _ = pr.terms(X, y, b, o, True)
    assert np.max(np.abs(g)) <= 1e-10 * max(1.0, y.sum())
    assert np.array_equal(H, H2) and ll == l2
    assert np.all(np.linalg.eigvalsh(H) > 0)


def test_reference_halving_from_a_far_start():
    # large counts: the full Newton step from the intercept-only start overshoots and is halved; the fit still lands on the MLE
    rng = np.random.default_rng(3)
    X = rng.uniform(-0.5, 0.5, (500, 3))
    y = rng.poisson(np.exp(5.0 + X @ np.array([4.0, -3.0, 2.0]))).astype(np.float64)
    b, H, _ = pr.fit(X, y, None, False)
    _, g, _, _ = pr.terms(X, y, b, None, False)
    assert np.max(np.abs(g)) <= 1e-9 * y.sum()


@pytest.mark.parametrize("offset", [False, True])
def test_reference_matches_sklearn(offset):
    lm = pytest.importorskip("sklearn.linear_model")
    X, y, o = _data(4, 3000, 5, True, offset)
    b, _, _ = pr.fit(X, y, o, True)
    if o is None:
        m = lm.PoissonRegressor(alpha=0, solver="newton-cholesky", tol=1e-12, max_iter=1000).fit(X, y)
    else:
        # an offset is exposure e^o: PoissonRegressor fits the rate y / e^o with sample weights e^o, the same likelihood in beta
        m = lm.PoissonRegressor(alpha=0, solver="newton-cholesky", tol=1e-12, max_iter=1000).fit(X, y / np.exp(o), sample_weight=np.exp(o))
    ref = np.concatenate([[m.intercept_], m.coef_])
    assert np.max(np.abs(b - ref)) / np.max(np.abs(ref)) <= 1e-8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def test_abi_rejects_bad_arguments(lib):
    from dlsa_amd import _lib
    fake = ctypes.c_void_p(256)
    # pass: null pointers, n < 1, p out of range, ldx < p, ldh < p + intercept, short workspace
    args = [fake, 4, fake, None, fake, 10, 4, 1, fake, 5, None, None, None, fake, 1 << 30, None]
    for i in (0, 2, 4):
        a = list(args); a[i] = None
        assert lib.dlsa_poisson_pass_f64(*a) == 1
    assert "null" in _lib.last_error()
    for i, v in ((5, 0), (6, 0), (6, 2048), (1, 3), (9, 4)):
        a = list(args); a[i] = v
        assert lib.dlsa_poisson_pass_f64(*a) == 1, (i, v)
    a = list(args); a[14] = 1024
    assert lib.dlsa_poisson_pass_f64(*a) == 3
    a = list(args); a[13] = None
    assert lib.dlsa_poisson_pass_f64(*a) == 3
    # fit: null pointers, K < 1, p out of range, ldx < p, bad row_step, bad tol / max_iter, negative partition shapes, workspace
    first, rows = (ctypes.c_int64 * 2)(0, 5), (ctypes.c_int64 * 2)(5, 5)
    fargs = [fake, 4, fake, None, first, rows, 1, 2, 4, 1, 1e-13, 100, fake, fake, fake, None, None, None, fake, 1 << 30, None]
    for i in (0, 2, 4, 5, 12, 13, 14):
        a = list(fargs); a[i] = None
        assert lib.dlsa_poisson_fit_f64(*a) == 1, i
    for i, v in ((7, 0), (8, 0), (8, 2048), (1, 3), (6, 0), (10, 0.0), (11, 0)):
        a = list(fargs); a[i] = v
        assert lib.dlsa_poisson_fit_f64(*a) == 1, (i, v)
    a = list(fargs); a[5] = (ctypes.c_int64 * 2)(5, -1)
    assert lib.dlsa_poisson_fit_f64(*a) == 1
    assert "partition 1" in _lib.last_error()
    a = list(fargs); a[4] = (ctypes.c_int64 * 2)(-3, 5)
    assert lib.dlsa_poisson_fit_f64(*a) == 1
    a = list(fargs); a[19] = 4096
    assert lib.dlsa_poisson_fit_f64(*a) == 3
    a = list(fargs); a[18] = ctypes.c_void_p(257)
    assert lib.dlsa_poisson_fit_f64(*a) == 3


def test_workspace_query_is_monotone(lib):
    assert lib.dlsa_poisson_workspace_bytes(100, 0, 0, 1) == 0
    assert lib.dlsa_poisson_workspace_bytes(100, 2048, 1, 1) == 0
    assert lib.dlsa_poisson_workspace_bytes(-1, 5, 0, 1) == 0
    assert lib.dlsa_poisson_workspace_bytes(100, 5, 0, 0) == 0
    for p in (1, 5, 100, 500, 2047):
        for icpt in (0, 1):
            for step in (1, 7):
                prev = 0
                for n in (0, 1, 63, 64, 65, 1000, 4096 * 64, 10 ** 6, 10 ** 7, 2 * 10 ** 7):
                    b = lib.dlsa_poisson_workspace_bytes(n, p, icpt, step)
                    assert b >= prev, (p, icpt, step, n)
                    prev = b
                # the strided form gathers counts and offsets: never less than the contiguous one
                assert lib.dlsa_poisson_workspace_bytes(10 ** 6, p, icpt, step) >= lib.dlsa_poisson_workspace_bytes(10 ** 6, p, icpt, 1)


# (max_rows, p) -> dlsa_poisson_workspace_bytes for (intercept, row_step) = (0, 1), (0, 25), (1, 1), (1, 25): the values of the library
# before the pass scratch went through count_pass.h's one take list
WORKSPACE_BYTES = {
    (0, 1): (4523264, 4523776, 4523264, 4523776),
    (0, 100): (5393408, 5393920, 5394944, 5395456),
    (0, 130): (10955008, 10955520, 10957056, 10957568),
    (0, 600): (62739200, 62739712, 62748928, 62749440),
    (0, 1025): (151381248, 151381760, 151397632, 151398144),
    (1, 1): (4523264, 4523776, 4523264, 4523776),
    (1, 100): (5393408, 5393920, 5394944, 5395456),
    (1, 130): (10955008, 10955520, 10957056, 10957568),
    (1, 600): (62739200, 62739712, 62748928, 62749440),
    (1, 1025): (151381248, 151381760, 151397632, 151398144),
    (3001, 1): (4809216, 4857344, 4809216, 4857344),
    (3001, 100): (6465792, 6513920, 6467328, 6515456),
    (3001, 130): (13338112, 13386240, 13340160, 13388288),
    (3001, 600): (88977408, 89025536, 88987136, 89035264),
    (3001, 1025): (227164672, 227212800, 227181056, 227229184),
    (10 ** 6, 1): (29038080, 45038080, 29038080, 45038080),
    (10 ** 6, 100): (79453696, 95453696, 79455232, 95455232),
    (10 ** 6, 130): (167590400, 183590400, 167592448, 183592448),
    (10 ** 6, 600): (175596544, 191596544, 175606272, 191606272),
    (10 ** 6, 1025): (310900224, 326900224, 310916608, 326916608),
}


def test_workspace_bytes_are_pinned(lib):
    """the layout takes the pass's six scratch arrays through the helper it shares with negbin.hip: sizes, order and alignment are
    those of the list it replaced"""
    assert len(WORKSPACE_BYTES) == 4 * 5
    for (n, p), want in WORKSPACE_BYTES.items():
        got = tuple(lib.dlsa_poisson_workspace_bytes(n, p, icpt, step) for icpt in (0, 1) for step in (1, 25))
        assert got == want, (n, p, got, want)
