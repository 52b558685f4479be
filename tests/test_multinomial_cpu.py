"""CPU: the numpy reference of the multinomial logistic map step (tests/multinomial_reference.py) held against itself -- the fp64
run against a longdouble run of the same code, the score and the information against finite differences, the information's
structure, C = 2 against a plain logistic Newton fit, the convergence of the fit on every shape the GPU file uses and the
calibration seed -- and the Python layer's argument checks that need no GPU.

The bar of the fp64-against-longdouble comparison is 1e-13 (what test_tweedie_cpu.py uses): the GPU file holds the kernels to 1e-12
against the fp64 run, so the reference's own error has to sit an order below."""
import numpy as np
import pytest

import multinomial_reference as mr

WIDTHS = [1, 7, 50, 100, 130, 260]
CLASSES = [2, 3, 5, 8]


def rel(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _wide_errors(X, y, theta, C, intercept, h_cols):
    t64 = mr.terms(X, y, theta, C, intercept, np.float64, h_cols)
    tld = mr.terms(X, y, theta, C, intercept, np.longdouble, h_cols)
    return {"ll": abs(float((t64[0] - tld[0]) / tld[0])), "g": rel(t64[1], tld[1]), "H": rel(t64[2], tld[2]), "P": rel(t64[3], tld[3])}


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("intercept", [False, True])
def test_fp64_terms_match_longdouble(p, C, intercept):
    n = 3 * p + 37
    X, y = mr.data(10 + p, n, p, C, intercept)
    errs = _wide_errors(X, y, mr.away_from_optimum((C - 1) * (p + intercept)), C, intercept, min(p + intercept, 8))
    print("multinomial reference p=%d C=%d icpt=%d: %s" % (p, C, intercept, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-13 for v in errs.values()), errs


def test_fp64_terms_match_longdouble_on_an_eta_span_of_600():
    X, y, theta = mr.eta_span_case()
    C = mr.ETA_SPAN_CLASSES
    eta = mr.design(X, True) @ theta.reshape(C - 1, -1).T
    assert np.ptp(np.concatenate([np.zeros((len(X), 1)), eta], 1), axis=1).max() > 590
    ll, g, H, P = mr.terms(X, y, theta, C, True)
    assert all(np.isfinite(v).all() for v in (ll, g, H, P))
    errs = _wide_errors(X, y, theta, C, True, None)
    print("multinomial reference, eta span 600: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    assert all(v <= 1e-13 for v in errs.values()), errs


@pytest.mark.parametrize("p,C,intercept", [(3, 3, True), (7, 4, False), (5, 8, True), (4, 2, True)])
def test_score_and_information_are_derivatives(p, C, intercept):
    """central differences in longdouble: g against ll (step 1e-6, truncation ~1e-12 relative), H against g"""
    n = 3 * p + 37
    X, y = mr.data(70 + p, n, p, C, intercept)
    m = (C - 1) * (p + intercept)
    theta = mr.away_from_optimum(m).astype(np.longdouble)
    ll, g, H, _ = mr.terms(X, y, theta, C, intercept, np.longdouble)
    h = np.longdouble(1e-6)
    gfd, Hfd = np.zeros(m, np.longdouble), np.zeros((m, m), np.longdouble)
    for i in range(m):
        d = np.zeros(m, np.longdouble)
        d[i] = h
        up, dn = mr.terms(X, y, theta + d, C, intercept, np.longdouble), mr.terms(X, y, theta - d, C, intercept, np.longdouble)
        gfd[i] = (up[0] - dn[0]) / (2 * h)
        Hfd[:, i] = -(up[1] - dn[1]) / (2 * h)
    assert rel(gfd, g) <= 1e-9, rel(gfd, g)
    assert rel(Hfd, H) <= 1e-9, rel(Hfd, H)


@pytest.mark.parametrize("p,C,intercept", [(7, 3, True), (50, 5, False), (20, 8, True)])
def test_information_is_symmetric_and_psd(p, C, intercept):
    n = 3 * p + 37
    X, y = mr.data(80 + p, n, p, C, intercept)
    H = mr.terms(X, y, mr.away_from_optimum((C - 1) * (p + intercept)), C, intercept)[2]
    assert np.array_equal(H, H.T)
    ev = np.linalg.eigvalsh(H)
    assert ev[0] >= -1e-12 * ev[-1], ev[0]


@pytest.mark.parametrize("p,intercept", [(7, True), (7, False), (50, True)])
def test_two_classes_are_the_logistic_model(p, intercept):
    n = 600
    X, y = mr.data(90 + p, n, p, 2, intercept)
    b, S, ll, n_iter = mr.fit(X, y, 2, intercept)
    bl, Sl, lll = mr.logistic_fit(X, y, intercept)
    errs = {"coef": rel(b, bl), "Sig_inv": rel(S, Sl), "ll": abs((ll - lll) / lll)}
    print("multinomial C = 2 against the logistic fit p=%d: %s" % (p, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-12 for v in errs.values()), errs
    # the terms at one point away from the optimum
    theta = mr.away_from_optimum(p + intercept)
    t = mr.terms(X, y, theta, 2, intercept)
    D = mr.design(X, intercept)
    mu = 1.0 / (1.0 + np.exp(-(D @ theta)))
    assert rel(t[1], D.T @ (y - mu)) <= 1e-13 and rel(t[2], (D * (mu * (1 - mu))[:, None]).T @ D) <= 1e-13 and rel(t[3][0], mu) <= 1e-13


@pytest.mark.parametrize("n,p,C,intercept", mr.FIT_SHAPES)
def test_fit_converges_from_the_start(n, p, C, intercept):
    X, y = mr.data(40 + p, n, p, C, intercept)
    b, S, ll, n_iter = mr.fit(X, y, C, bool(intercept))
    g = mr.terms(X, y, b, C, bool(intercept))[1]
    print("multinomial reference fit n=%d p=%d C=%d icpt=%d: %d evaluations, |g| %.1e" % (n, p, C, intercept, n_iter, np.max(np.abs(g))))
    assert n_iter <= 12 and np.max(np.abs(g)) <= 1e-9 * n
    assert np.linalg.eigvalsh(S)[0] > 0


def test_start_is_the_mle_of_the_intercept_only_model():
    X, y = mr.data(5, 400, 3, 4, True)
    theta = mr.start(y, 3, 4, True)
    g = mr.terms(X, y, theta, 4, True)[1].reshape(3, 4)
    assert np.max(np.abs(g[:, 0])) <= 1e-11


def test_calibration_seed_sits_within_two_sigma():
    """Q = sum_k (theta_k - theta*)' Sig_inv_k (theta_k - theta*) is chi-square on 240 degrees of freedom (sigma = sqrt(480)): the GPU
    file asserts 240 +- 88 (4 sigma) on the engine's blocks; here the reference alone lies within 240 +- 44 for the chosen seed, so a
    1e-10 difference cannot tip that test"""
    X, y = mr.calibration_case()
    K = mr.CALIBRATION_K
    fits = [mr.fit(X[k::K], y[k::K], mr.CALIBRATION_CLASSES, True) for k in range(K)]
    q = mr.calibration_q([f[0] for f in fits], [f[1] for f in fits])
    print("multinomial calibration (reference): Q = %.1f on 240" % q)
    assert abs(q - 240.0) <= 44.0, q


def test_column_names_are_class_major():
    models = pytest.importorskip("dlsa_amd.models")
    assert models.multinomial_column_names(["intercept", "a", "b"], 3) == ["intercept:1", "a:1", "b:1", "intercept:2", "a:2", "b:2"]


@pytest.mark.parametrize("classes,p,text", [(1, 5, "classes must lie in 2 .. 8"), (9, 5, "classes must lie in 2 .. 8"),
                                            (8, 300, "exceed the solver's 2048"), (2.5, 5, "must be an integer")])
def test_class_count_is_checked_without_a_gpu(classes, p, text):
    engine = pytest.importorskip("dlsa_amd.engine")
    with pytest.raises(ValueError, match=text):
        engine.multinomial_classes("multinomial_fit_ex", classes, p)
    assert engine.multinomial_classes("multinomial_fit_ex", 8, 292) == 8
