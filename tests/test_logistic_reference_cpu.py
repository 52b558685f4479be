"""No GPU, no library: the reference, the designs and the bounds of tests/logistic_reference.py checked against themselves.
The 50-digit terms agree with the oracle where the oracle is accurate; the plain numpy evaluation and an operation-by-operation
emulation of csrc/logistic.h MEET every bound on every grid (so the bounds ask nothing a correct kernel cannot give); and every
mutant a kernel could plausibly be -- a cancelling w, a log without log1p, a flushed subnormal, a clamp too early, a branch
switch without its constant, an fp32 exp, the wrong half of the sigmoid, rows swapped / dropped / doubled, a stray off-diagonal,
a flipped sign -- is REJECTED by the checker that guards it, on the full grid and on a regime.  The suite's older assertions
(rel_inf < 1e-12 on |eta| of a few units; atol = 1e-16 on four rows) let the first four of them through, which is shown too.
(The form follows test_exact_designs_cpu.py.)"""
import mpmath
import numpy as np
import pytest

import logistic_reference as lr


def rel_inf(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def on_unique(fn):
    """evaluate a (slow) row-term function once per distinct eta"""
    def wrapped(eta):
        u, inv = np.unique(np.asarray(eta, dtype=np.float64).view(np.int64), return_inverse=True)
        out = fn(u.view(np.float64))
        return {k: v[inv] for k, v in out.items()}
    return wrapped


def full_design(b0=None):
    return lr.Design("full", 2 * lr.full_grid().size, 7, b0=b0)            # two tiles: every eta meets both labels


def check_pass(d, term_fn, what, rows=("w", "mu", "sp")):
    bd = lr.bounds(d.name)
    eta = d.eta()
    tr = term_fn(eta)
    for key in rows:
        lr.check_rows(tr[key], key, eta, bd, what=what)
    w, g, H, ll = lr.numpy_pass(d, term_fn)
    return lr.check_sums(d, bd, g=g, H=H, ll=ll, what=what)


def test_grids_hold_what_they_promise():
    g = lr.full_grid()
    assert 4000 <= g.size <= 4200 and g.min() == -1e6 and g.max() == 1e6
    for v in lr.BRANCH_POINTS + (5e-324, 1e-300, 1.0):
        assert v in g and -v in g
    assert set(np.signbit(g[g == 0.0]).tolist()) == {False, True}               # +0 and -0
    assert len(lr.REGIMES) == 22
    for c in lr.REGIMES:
        r = lr.regime_grid(c)
        assert r.size == 257 and np.unique(r).size == 257
        if c != "tiny":
            assert r.min() == c - 0.5 and r.max() == c + 0.5
    t = lr.regime_grid("tiny")
    assert np.abs(t).max() == 1e-8 and abs(np.abs(t).min() - 1e-300) < 1e-312 and (t > 0).sum() == 129


def test_design_gives_eta_exactly_whatever_the_order():
    for name, n, p, b0 in (("full", 4099, 129, None), (-37.5, 3001, 7, -37.5), (745.0, 67, 1030, None), ("tiny", 67, 1, 0.0)):
        d = lr.Design(name, n, p, b0=b0)
        X = d.dense()
        assert np.all((X != 0).sum(1) <= 1)
        beta = d.beta
        fwd = np.zeros(n); bwd = np.zeros(n)
        for j in range(p):
            fwd += X[:, j] * beta[j]
            bwd += X[:, p - 1 - j] * beta[p - 1 - j]
        eta = d.eta()
        want = fwd + b0 if b0 is not None else fwd
        assert np.array_equal(want, eta) and np.array_equal(fwd, bwd)
        big = np.sort(np.abs(d.dot_k))[-4]
        assert np.any(np.abs(d.dot_k[d.col_k == 0]) >= big) and np.any(np.abs(d.dot_k[d.col_k == p - 1]) >= big)
        if n >= 2 * d.G:
            assert np.all(d.counts() >= 1)
    assert not np.array_equal(lr.Design("full", 4099, 7).k[:64], np.arange(64))     # permuted


def test_reference_agrees_with_the_oracle_where_the_oracle_is_accurate():
    from oracle import dlsa_oracle as orc
    g = lr.full_grid()
    eta = g[np.abs(g) <= 20.0]
    t = lr.terms(eta)
    y = (np.arange(eta.size) % 2).astype(np.float64)
    wo, go, llo = orc.logit_pass(eta[:, None], y, np.array([1.0]))
    assert np.max(np.abs(t.f_w - wo) / t.f_w) < 1e-6 * 1e-1            # w = mu (1 - mu) keeps 1e-7 at |eta| = 20
    assert np.max(np.abs(t.f_w - wo)) < 4 * lr.U                       # (its 1 - mu carries half an ulp of 1)
    with mpmath.workdps(lr.DPS):
        ll = sum(yv * mpmath.mpf(float(e)) - s for yv, e, s in zip(y, eta, t.sp))
        gg = sum((yv - m) * mpmath.mpf(float(e)) for yv, e, m in zip(y, eta, t.mu))
        assert abs(float(ll) - llo) < 1e-13 * abs(llo) and abs(float(gg) - go[0]) < 1e-12 * np.abs(eta).sum()
        # symmetries of the reference itself, over the whole grid
        tp, tn = lr.terms(np.abs(g)), lr.terms(-np.abs(g))
        for k in range(g.size):
            assert tp.w[k] == tn.w[k]
            assert abs(tp.mu[k] + tn.mu[k] - 1) < mpmath.mpf(10) ** -45
            assert abs(tp.sp[k] - tn.sp[k] - mpmath.mpf(float(abs(g[k])))) < mpmath.mpf(10) ** -45 * max(1.0, float(abs(g[k])))


def test_plain_numpy_meets_every_bound_on_every_grid():
    worst = check_pass(full_design(), lr.plain_terms, "numpy full")
    worst = max(worst, check_pass(full_design(b0=0.0), lr.plain_terms, "numpy full + intercept"))
    print("full grid:", lr.bounds("full"), "worst sum error / bound %.3f" % worst)
    for c in lr.REGIMES:
        for n, p in ((67, 7), (3001, 7), (3001, 130)):
            for b0 in (None, lr.regime_centre(c)):
                r = check_pass(lr.Design(c, n, p, b0=b0), lr.plain_terms, "numpy %s n=%d p=%d b0=%r" % (c, n, p, b0))
                assert r <= 1.0
        print("regime", c, lr.bounds(c))


def test_emulated_logistic_h_meets_every_bound_on_every_grid():
    emu = on_unique(lr.emulate_logistic_h)
    check_pass(full_design(), emu, "logistic.h emulated, full")
    for c in lr.REGIMES:
        check_pass(lr.Design(c, 3001, 7), emu, "logistic.h emulated, %s" % (c,))
    # what the header's accuracy sentence has to say: the emulation's own worst errors
    g = lr.full_grid()
    t, em = lr.terms(g), lr.emulate_logistic_h(g)
    for key in ("w", "mu", "sp"):
        e = lr.ulp_errors(em[key], getattr(t, key), getattr(t, "f_" + key))
        print("emulation: %s worst %.2f ulp at eta = %r" % (key, e.max(), g[int(np.argmax(e))]))
        assert e.max() <= lr.bounds("full").B[key]


# ---------------------------------------------------------------------------------------------------------- mutants
def mutant_terms(name):
    return lambda eta: lr.plain_terms(eta, mutant=name)


def pass_with(d, term_fn=lr.plain_terms, row_weight=None, yeta_sign=1.0):
    """numpy_pass with per-row multiplicities in the sums (0: the row dropped, 2: doubled) or the sign of y eta flipped"""
    eta = d.eta()
    tr = term_fn(eta)
    rw = np.ones(d.n) if row_weight is None else row_weight
    resid = (d.y - tr["mu"]) * rw
    g = np.bincount(d.col, weights=resid * d.x, minlength=d.p)
    H = np.diag(np.bincount(d.col, weights=tr["w"] * d.x * d.x * rw, minlength=d.p))
    ll = float(np.sum((yeta_sign * d.y * eta - tr["sp"]) * rw))
    return tr["w"].copy(), g, H, ll


def heavy_row(d):
    """a row whose terms of g, H and loglik are all far above the sums' rounding: label 0 at eta ~ 3 (full grid), else the label
    that leaves a residual of order one"""
    eta = d.eta()
    if d.name == "full":
        cand = np.nonzero(d.y == 0.0)[0]
        return int(cand[np.argmin(np.abs(eta[cand] - 3.0))])
    return int(np.nonzero(d.y == (0.0 if eta[0] > 0 else 1.0))[0][0])


# mutant -> (the row terms that must be rejected on the full grid, [(regime, n, what must be rejected there)]).  The regimes are
# those where the mutant differs from the truth by more than the bounds' floor: w = mu (1 - mu) is accurate for eta < 0, a
# flushed e of half a subnormal ulp at 745 is within B_w, and the y sp(eta) floor of a row with label 1 hides a softplus off by
# 1e-17 at eta = -37.5 -- a call whose labels are all 0 (n = 67: one tile) shows it.
TERM_MUTANTS = {
    "w_mu_1_minus_mu": (("w",), [(37.5, 67, "wH"), (37.5, 3001, "wH"), (100.0, 3001, "wH"), (720.0, 67, "wH")]),
    "log_1_plus_e": (("sp",), [(-37.5, 67, "sl"), (-100.0, 67, "sl"), (-720.0, 67, "sl"), (-37.5, 3001, "s")]),
    "flush_subnormal": (("w", "mu"), [(720.0, 67, "wH"), (720.0, 3001, "wH"), (-720.0, 67, "wmgHl"), (-720.0, 3001, "wmH")]),
    "clamp700": (("w",), [(720.0, 3001, "wH"), (-745.0, 67, "wmgHl"), (-745.0, 3001, "wH"), (1e6, 67, "wH")]),
    "branch_at_half": (("sp",), [(0.88, 67, "sl"), (0.88, 3001, "sl"), (-0.88, 67, "sl"), (-0.88, 3001, "sl")]),
    "exp_fp32": (("w", "mu", "sp"), [(5.0, 67, "wmsgHl"), (5.0, 3001, "wgHl"), (-20.0, 3001, "wH"), (400.0, 67, "wH"), ("tiny", 67, "gl")]),
    "mu_of_positive": (("mu",), [(-5.0, 67, "mg"), (-0.88, 3001, "mg"), (-400.0, 3001, "mg"), (-745.0, 67, "mg"), ("tiny", 3001, "mg")]),
}
KINDS = {"w": "w", "m": "mu", "s": "sp", "g": "g", "H": "H", "l": "ll"}


@pytest.mark.parametrize("name", sorted(TERM_MUTANTS))
def test_row_term_mutants_are_rejected(name):
    rows, cases = TERM_MUTANTS[name]
    fn = mutant_terms(name)
    d = full_design()
    eta = d.eta()
    tr = fn(eta)
    for key in rows:
        with pytest.raises(AssertionError):
            lr.check_rows(tr[key], key, eta, lr.bounds("full"), what=name)
    for c, n, kinds in cases:
        dr = lr.Design(c, n, 7)
        etar = dr.eta()
        trr = fn(etar)
        w, g, H, ll = lr.numpy_pass(dr, fn)
        for kind in kinds:
            key = KINDS[kind]
            with pytest.raises(AssertionError):
                if key in ("w", "mu", "sp"):
                    lr.check_rows(trr[key], key, etar, lr.bounds(c), what=name)
                else:
                    lr.check_sums(dr, lr.bounds(c), **{key: {"g": g, "H": H, "ll": ll}[key]}, what=name)


@pytest.mark.parametrize("name", ["full", 5.0, -20.0, -0.88, 400.0])
def test_row_bookkeeping_mutants_are_rejected(name):
    d = full_design() if name == "full" else lr.Design(name, 3001, 7)
    bd = lr.bounds(name)
    eta = d.eta()
    w, g, H, ll = pass_with(d)
    lr.check_rows(w, "w", eta, bd); lr.check_sums(d, bd, g=g, H=H, ll=ll)            # the unmutated pass is accepted
    # two rows of one 8-row batch swap w
    b = next(b for b in range(d.n // 8) if w[8 * b + 1] != w[8 * b + 2])
    ws = w.copy(); ws[[8 * b + 1, 8 * b + 2]] = ws[[8 * b + 2, 8 * b + 1]]
    with pytest.raises(AssertionError):
        lr.check_rows(ws, "w", eta, bd, what="swapped w")
    # ... and in H, for the batch whose swap moves H most (two rows deep in one tail swap weights that no sum can tell apart)
    x2 = d.x * d.x
    gain = np.abs((w[1::8][:d.n // 8 - 1] - w[2::8][:d.n // 8 - 1]) * (x2[1::8][:d.n // 8 - 1] - x2[2::8][:d.n // 8 - 1]))
    b = int(np.argmax(gain))
    ws = w.copy(); ws[[8 * b + 1, 8 * b + 2]] = ws[[8 * b + 2, 8 * b + 1]]
    with pytest.raises(AssertionError):
        lr.check_sums(d, bd, H=np.diag(np.bincount(d.col, weights=ws * x2, minlength=d.p)), what="swapped w in H")
    # one row dropped, one row doubled: each of g, H, loglik on its own
    r = heavy_row(d)
    for mult in (0.0, 2.0):
        rw = np.ones(d.n); rw[r] = mult
        _, g1, H1, ll1 = pass_with(d, row_weight=rw)
        for kw in ({"g": g1}, {"H": H1}, {"ll": ll1}):
            with pytest.raises(AssertionError):
                lr.check_sums(d, bd, what="row x %g" % mult, **kw)
    # a nonzero in one off-diagonal (kept symmetric: only the exact-zero check can see it), an empty column that is not zero
    H2 = H.copy(); H2[2, 5] = H2[5, 2] = 5e-324
    with pytest.raises(AssertionError):
        lr.check_sums(d, bd, H=H2, what="off-diagonal")
    H3 = H.copy(); H3[1, 4] = 1e-300
    with pytest.raises(AssertionError):
        lr.check_sums(d, bd, H=H3, what="asymmetric")
    # the sign of y eta
    _, _, _, ll4 = pass_with(d, yeta_sign=-1.0)
    with pytest.raises(AssertionError):
        lr.check_sums(d, bd, ll=ll4, what="sign of y eta")


def test_empty_columns_must_be_exact_zeros():
    d = lr.Design(-100.0, 67, 1030)
    w, g, H, ll = lr.numpy_pass(d)
    lr.check_sums(d, lr.bounds(-100.0), g=g, H=H, ll=ll)
    empty = np.setdiff1d(np.arange(d.p), d.col)
    assert empty.size > 900
    g1 = g.copy(); g1[empty[3]] = 5e-324
    with pytest.raises(AssertionError):
        lr.check_sums(d, lr.bounds(-100.0), g=g1)
    H1 = H.copy(); H1[empty[5], empty[5]] = 5e-324
    with pytest.raises(AssertionError):
        lr.check_sums(d, lr.bounds(-100.0), H=H1)


def test_gather_design_is_checked_like_a_dense_one():
    for name in ("full", -37.5, 720.0):
        base = lr.Design(name, 4099, 1)
        eta_k = lr.grid(name)[:1400]
        rows = np.nonzero(base.k < eta_k.size)[0]
        d = lr.GatherDesign(name, eta_k, base.k[rows], base.y[rows])
        tr = lr.plain_terms(d.eta())
        g = np.bincount(d.k, weights=d.y - tr["mu"], minlength=d.p)
        ll = float(np.sum(d.y * d.eta() - tr["sp"]))
        lr.check_rows(tr["w"], "w", d.eta(), lr.bounds(name))
        lr.check_sums(d, lr.bounds(name), g=g, ll=ll)
        r = int(np.argmax(np.abs(d.y - tr["mu"])))                           # a row with a residual of order one, doubled
        g1 = g.copy(); g1[d.k[r]] += (d.y[r] - tr["mu"][r])
        with pytest.raises(AssertionError):
            lr.check_sums(d, lr.bounds(name), g=g1)


FIRST_FOUR = ("w_mu_1_minus_mu", "log_1_plus_e", "flush_subnormal", "clamp700")


@pytest.mark.parametrize("name", FIRST_FOUR)
def test_the_older_assertions_let_the_first_four_mutants_through(name):
    """What the suite asserted on the logistic terms before: rel_inf(w) < 1e-12 (relative to the LARGEST weight), g and loglik
    to 1e-12 on Gaussian designs with |eta| of a few units (test_logit_pass_matches_oracle and its fused / wide siblings), and
    atol = 1e-16 on the four rows of test_logit_pass_extreme_eta.  Each of the four mutants passes them."""
    from oracle import dlsa_oracle as orc
    fn = mutant_terms(name)
    rng = np.random.default_rng(5)
    n, p = 4000, 20
    X = rng.standard_normal((n, p))
    beta = 0.5 * rng.standard_normal(p)
    y = (rng.random(n) < 0.5).astype(np.float64)
    wo, go, llo = orc.logit_pass(X, y, beta)
    eta = X @ beta
    tr = fn(eta)
    w, g, ll = tr["w"], X.T @ (y - tr["mu"]), float(np.sum(y * eta - tr["sp"]))
    assert rel_inf(w, wo) < 1e-12
    assert np.max(np.abs(g - go)) < 1e-12 * np.max(np.abs(X).sum(0))
    assert abs(ll - llo) < 1e-12 * abs(llo)
    # the four rows of test_logit_pass_extreme_eta, with its assertions
    X4 = np.array([[800.0, 0.0], [-800.0, 0.0], [0.0, 0.0], [30.0, 1.0]])
    y4 = np.array([1.0, 0.0, 1.0, 0.0])
    b4 = np.array([1.0, 1.0])
    wo, go, llo = orc.logit_pass(X4, y4, b4)
    eta = X4 @ b4
    tr = fn(eta)
    w, ll = tr["w"], float(np.sum(y4 * eta - tr["sp"]))
    assert np.all(np.isfinite(w)) and np.isfinite(ll)
    assert np.allclose(w, wo, rtol=1e-12, atol=1e-16)
    assert abs(ll - llo) < 1e-12 * abs(llo)
    exact = np.exp(-31.0) / (1 + np.exp(-31.0)) ** 2
    if name == "w_mu_1_minus_mu":
        # that test's one relative check (row 4, eta = 31) does see the cancellation -- at that single eta, on that single route
        assert abs(w[3] - exact) > 1e-14 * exact
    else:
        assert abs(w[3] - exact) < 1e-14 * exact
    # ... and the new checker rejects the same four rows' terms
    key = TERM_MUTANTS[name][0][0]
    eta_new = np.array([800.0, -800.0, 36.8, -36.8, 720.0, -720.0])
    with pytest.raises(AssertionError):
        lr.check_rows(fn(eta_new)[key], key, eta_new, lr.bounds("full"), what=name)
