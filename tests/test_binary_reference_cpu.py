"""CPU: the reference of the probit and cloglog row terms (tests/binary_reference.py) is itself checked -- the bounds it derives can
be met by a plain fp64 evaluation, they are tight enough to mean something, and they reject every textbook form they are there for.

Measured here (the model evaluation's worst ulp error E per regime and response, profiles/binary_stats.txt has the table): probit
z <= -2: E <= 6.5; probit -2.5 <= z < 0 (K by the continued fraction down to a = 1/4): E_w <= 10.5; cloglog eta <= -3: E <= 2.5; cloglog
-3 < eta <= 2: E <= 5.0; cloglog eta > 2: 13 .. 470, the floor of a term that is a function of the rounded mu."""
import math

import mpmath
import numpy as np
import pytest

import binary_reference as br

CASES = [(link, name) for link in br.LINKS for name in br.REGIMES[link]]


@pytest.mark.parametrize("link,name", CASES)
def test_model_evaluation_accuracy_class(link, name):
    """E <= 8 for l, r and w on every probit regime with z <= -2 and every cloglog regime with eta <= -3; E <= 64 on every other
    regime whose centre has |z| <= 8, respectively eta <= 2 (by the centre: the unit interval round 8 reaches 8.5 and is not to
    fall under no condition at all)"""
    b = br.bounds(link, name)
    print(repr(b))
    for y in (0, 1):
        lo, hi = br.z_range(link, name, y)
        centre = br.regime_centre(name)
        for key in br.KEYS:
            E = b.E[y][key]
            assert math.isfinite(E), (link, name, y, key)
            if hi <= (-2.0 if link == "probit" else -3.0):
                assert E <= 8.0, (link, name, y, key, E)
            elif (link == "probit" and abs(centre) <= 8.0) or (link == "cloglog" and centre <= 2.0):
                assert E <= 64.0, (link, name, y, key, E)


@pytest.mark.parametrize("link", br.LINKS)
def test_full_grid_is_finite_and_w_is_positive(link):
    """no NaN anywhere, w >= 0 in fp64 and w > 0 in the reference on every point of the sweep"""
    g = br.grid(link, "full")
    for y in (0, 1):
        t = br.ref_terms(link, g, y)
        assert all(w > 0 for w in t.w), (link, y)
        m = br.model_terms(link, g, y)
        for key in br.KEYS:
            assert np.all(np.isfinite(m[key])), (link, y, key, g[~np.isfinite(m[key])][:5])
        assert np.all(m["w"] >= 0.0)
        b = br.bounds(link, "full")
        assert all(math.isfinite(v) for v in b.E[y].values()), repr(b)


@pytest.mark.parametrize("link", br.LINKS)
def test_reference_derivatives(link):
    """r and w of the reference against mpmath's own numerical derivatives of l at 30 points"""
    pts = np.linspace(-6.0, 6.0, 30) if link == "probit" else np.linspace(-12.0, 3.0, 30)
    fn = br._probit_mp if link == "probit" else br._cloglog_mp
    with mpmath.workdps(80):
        for v in pts:
            for y in (0, 1):
                x = mpmath.mpf(float(v))
                l, r, w, _ = fn(x, y)
                d1 = mpmath.diff(lambda e: fn(e, y)[0], x)
                d2 = mpmath.diff(lambda e: fn(e, y)[0], x, 2)
                assert abs(d1 - r) <= mpmath.mpf(10) ** -25 * (1 + abs(r)), (link, v, y)
                assert abs(-d2 - w) <= mpmath.mpf(10) ** -20 * (1 + abs(w)), (link, v, y)


def test_cloglog_floor_derivatives():
    """the floor's d / dmu of l, r, w against numerical derivatives in mu"""
    with mpmath.workdps(800):
        for v in (2.1, 3.0, 5.0, 6.5):
            eta = mpmath.mpf(v)
            mu = mpmath.exp(eta)
            d = br._cloglog_mp(eta, 1)[3]
            for j in range(3):
                num = mpmath.diff(lambda m: br._cloglog_mp(mpmath.log(m), 1)[j], mu)
                assert abs(num - d[j]) <= mpmath.mpf(10) ** -20 * abs(d[j]), (v, j)


@pytest.mark.parametrize("link,name", CASES + [("probit", "full"), ("cloglog", "full")])
def test_numpy_pass_meets_the_bounds(link, name):
    """the CPU stand-in for a kernel passes check_rows and check_sums on a design with and without the intercept and with offsets"""
    b = br.bounds(link, name)
    for p, b0, offset in ((3, None, False), (4, br.regime_centre(name), False), (5, None, True)):
        d = br.Design(link, name, p, b0=b0, offset=offset)
        w, g, Hd, ll = br.numpy_pass(d)
        what = "%s %s p=%d b0=%r offset=%r" % (link, name, p, b0, offset)
        br.check_rows(link, w, "w", d.eta(), d.y, b, what)
        ratio = br.check_sums(d, b, g=g, Hdiag=Hd, ll=ll, what=what)
        assert ratio <= 1.0


# each textbook form must FAIL its bound on the grid that exposes it
MUTANTS = [
    ("probit", "w_lam_plus_z", 30.0, "w"),           # lambda (lambda + z) at z <= -30
    ("probit", "w_lam_plus_z", 100.0, "w"),
    ("probit", "square_unsplit", 30.0, "w"),         # z * z unsplit at z >= 30
    ("probit", "square_unsplit", 38.0, "l"),
    ("cloglog", "w_direct", -20.0, "w"),             # mu + r - 1 direct at mu <= 1e-6
    ("cloglog", "w_direct", -400.0, "w"),
    ("cloglog", "ll_log_expm1", 5.0, "l"),           # log(-expm1(-mu)) at mu >= 40 ...
    ("cloglog", "ll_log_expm1", -720.0, "l"),        # ... and at eta <= -720 (a subnormal mu)
    ("cloglog", "ll_log_expm1", -745.0, "l"),
]


@pytest.mark.parametrize("link,mutant,name,key", MUTANTS)
def test_bounds_reject_the_textbook_forms(link, mutant, name, key):
    b = br.bounds(link, name)
    d = br.Design(link, name, 3)
    eta = d.eta()
    rows = {k: np.empty(d.n) for k in br.KEYS}
    for y in (0, 1):
        sel = d.y == y
        m = br.model_terms(link, eta[sel], y, mutant)
        for k in br.KEYS:
            rows[k][sel] = m[k]
    with pytest.raises(AssertionError):
        br.check_rows(link, rows[key], key, eta, d.y, b, "%s %s" % (mutant, name))
    # (the per-row bound is the judge: in a sum of 514 terms the summation term can hide a loss that has no common sign)
    clean = {k: np.where(d.y == 1, br.model_terms(link, eta, 1)[k], br.model_terms(link, eta, 0)[k]) for k in br.KEYS}
    br.check_rows(link, clean[key], key, eta, d.y, b, "unmutated %s" % name)


def test_no_regime_within_the_asserted_range_is_left_unasserted():
    """every probit regime with a centre up to 8 and every cloglog regime with a centre up to 2 falls under one of the two conditions"""
    for link, top in (("probit", 8.0), ("cloglog", 2.0)):
        inside = [n for n in br.REGIMES[link] if (abs(br.regime_centre(n)) if link == "probit" else br.regime_centre(n)) <= top]
        assert len(inside) >= 9 and (8.0 in inside if link == "probit" else 1.5 in inside)
        for name in inside:
            b = br.bounds(link, name)
            assert max(max(b.E[y].values()) for y in (0, 1)) <= 64.0, repr(b)


def test_designs_reach_the_grid_exactly():
    for link in br.LINKS:
        for name in (br.REGIMES[link][0], br.REGIMES[link][-1], "full"):
            g = br.grid(link, name)
            for b0, offset in ((None, False), (br.regime_centre(name), False), (None, True), (0.0, True)):
                d = br.Design(link, name, 4, b0=b0, offset=offset)
                assert d.n == 2 * g.size and set(np.unique(d.y)) == {0.0, 1.0}
                if name != "full" or b0 is None:            # (full grid with an intercept: tiny points round into b0)
                    assert np.array_equal(d.eta_k(), g), (link, name, b0, offset)
                assert np.all(d.counts() == 1)


def test_newton_fit_recovers_a_known_model():
    rng = np.random.default_rng(5)
    X = rng.uniform(-1.0, 1.0, (600, 2))
    o = np.log(rng.uniform(0.5, 2.0, 600))
    for link in br.LINKS:
        eta = -0.3 + X @ np.array([0.8, -0.5]) + o
        prob = -np.expm1(-np.exp(eta)) if link == "cloglog" else 0.5 * (1.0 + np.vectorize(math.erf)(eta / math.sqrt(2.0)))
        y = (rng.uniform(size=600) < prob).astype(np.float64)
        coef, H, Hc, ll = br.newton_fit(link, X, y, offset=o, fit_intercept=True)
        # the score vanishes at coef (fp64 model terms suffice to see 1e-9)
        D = np.concatenate([np.ones((600, 1)), X], 1)
        e = D @ coef + o
        r = np.where(y == 1, br.model_terms(link, e, 1)["r"], br.model_terms(link, e, 0)["r"])
        assert np.max(np.abs(D.T @ r)) <= 1e-9
        assert np.allclose(H @ coef, Hc, rtol=1e-13) and np.all(np.linalg.eigvalsh(H) > 0) and ll < 0
        assert np.max(np.abs(coef - np.array([-0.3, 0.8, -0.5]))) < 0.6
