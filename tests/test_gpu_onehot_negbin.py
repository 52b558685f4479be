"""GPU: the structured one-hot NB2 map step (csrc/onehot_negbin.hip) -- the negative-binomial pass and fit on raw numerics +
level codes -- against the numpy / scipy reference (tests/negbin_reference.py) on the dense matrix
oracle.dlsa_oracle.design_matrix builds: the pass at a fixed (beta, alpha), eta beyond 700, alpha mu beyond the double range,
the per-partition fit and its stationarity, structured = dense, the alpha = 0 and fixed-alpha branches, edge cases,
reproducibility, the frame-level negbin_model / negbin_model_eval, the end-to-end DLSA combine, and a 1.4e7-row fit with its
memory bound."""
import math
import os
import sys
import warnings

import numpy as np
import pytest

import negbin_reference as nr
from test_gpu_negbin import _theta_terms_mp
from test_gpu_onehot import _plan, _random_design
from test_gpu_onehot_poisson import SHAPES, _frame, _spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL_PASS = 1e-12
TOL_FIT = 1e-10


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import dlsa_amd
    return dlsa_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import dlsa_oracle
    return dlsa_oracle


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_pass(plan, num, codes, y, o, beta, alpha, X, tag=None, theta=True):
    """structured pass == the reference on the dense matrix X, every figure printed before it is asserted"""
    from dlsa_amd import engine
    q = num.shape[1]
    H, g, ll, w, mu, tt = engine.onehot_negbin_pass(plan, dev(num) if q else None, dev(codes), dev(y), dev(beta), alpha, offset=dev(o),
                                                    want_w=True, want_theta=True)
    llr, gr, Hr, mur, sr, ir, per = nr.terms(X, y, beta, alpha, o, False)
    Hn = H.cpu().numpy()
    figs = (abs(float(ll.item()) - llr) / abs(llr), rel(g.cpu().numpy(), gr), rel(mu.cpu().numpy(), mur),
            rel(w.cpu().numpy(), mur / (1.0 + alpha * mur)), rel(Hn, Hr))
    print("pass", tag, "alpha", alpha, "rel err ll %.2e g %.2e mu %.2e w %.2e H %.2e" % figs)
    assert math.isfinite(llr) and np.all(np.isfinite(Hr))
    assert max(figs) <= TOL_PASS, figs
    assert np.array_equal(Hn, Hn.T)
    if not theta:
        return H, g, ll, w, mu
    # s, i, pearson under the rule of test_gpu_negbin._check_pass: the scipy reference's own error against mpmath on the same (y, mu),
    # times 10, floored at eps sum |terms| (the rounding any fp64 evaluation of a cancelling sum carries).  The rule is written in
    # absolute form -- both sides multiplied by |truth| -- so that it also holds where a sum is exactly 0 (one row).
    truth = [float(v) for v in _theta_terms_mp(y, mur, alpha)]
    th = 1.0 / alpha
    from scipy import special
    mag = [float(np.sum(np.abs(special.digamma(y + th) - special.digamma(th)) + np.abs(np.log1p(alpha * mur)) + np.abs((mur - y) / (mur + th)))),
           float(np.sum(np.abs(special.polygamma(1, th) - special.polygamma(1, y + th)) + 1.0 / th + 2.0 / (mur + th) + (y + th) / (mur + th) ** 2)),
           truth[2]]
    got = tt.cpu().numpy()
    for name, t, r, k, m in zip(("s", "i", "pearson"), truth, (sr, ir, per), got, mag):
        e_ref, e_k, floor = abs(r - t), abs(k - t), np.finfo(float).eps * m
        print("  theta terms %s: truth %.6e abs err scipy %.2e kernel %.2e floor %.2e" % (name, t, e_ref, e_k, floor))
        assert e_k <= 10 * max(e_ref, floor), (name, e_k, e_ref, floor)
    return H, g, ll, w, mu


def _counts(rng, X, beta, o, alpha):
    """gamma-mixed counts around half the linear predictor: any counts do, the pass is checked away from the MLE"""
    eta = X @ beta + (0.0 if o is None else o)
    return rng.poisson(np.exp(np.clip(0.5 * eta, -20, 4)) * rng.gamma(1.0 / alpha, alpha, len(eta))).astype(np.float64)


@pytest.mark.parametrize("alpha", [0.05, 0.5, 5.0])
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("intercept,baseline", [(True, True), (False, False)])
@pytest.mark.parametrize("n,q,nlevels", SHAPES)
def test_pass_matches_reference(api, orc, n, q, nlevels, intercept, baseline, offset, alpha):
    rng = np.random.default_rng(n + q)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels, intercept=intercept, baseline=baseline)
    codes[rng.integers(0, n, max(1, n // 50)), 0] = -1          # unknown level: no column
    plan = _plan(api, p, desc, nl, level_col)
    if nlevels[:2] == (110, 110):
        assert plan.roles >= 2                                  # several Gram roles
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.4                             # eta spans a few units
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    y = _counts(rng, X, beta, o, alpha)
    _check_pass(plan, num, codes, y, o, beta, alpha, X, (n, q, nlevels, intercept, baseline, offset))


def test_pass_with_unordered_adds(api, orc):
    """DLSA_OH_ORDERED=0: all waves add at once, last bits vary from run to run -- against the reference only."""
    from dlsa_amd import engine
    n, q, nlevels = 777, 7, (40, 40, 9, 2)
    rng = np.random.default_rng(n + q)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.4
    o = np.log(rng.uniform(0.5, 2.0, n))
    with engine.kernel_options(onehot_ordered=0):
        _check_pass(plan, num, codes, _counts(rng, X, beta, o, 0.5), o, beta, 0.5, X, (n, q, nlevels, "unordered"))


def test_pass_with_row_banded_pair_tables(api, orc):
    n, q, nlevels = 30000, 2, (300, 300)
    rng = np.random.default_rng(n)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    assert plan.roles >= 2                                      # a pair table beyond LDS, cut into row bands
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.4
    o = np.log(rng.uniform(0.5, 2.0, n))
    _check_pass(plan, num, codes, _counts(rng, X, beta, o, 0.5), o, beta, 0.5, X, (n, q, nlevels))


def test_pass_eta_spanning_700(api, orc):
    """Level coefficients of +-400 with a compensating offset: the gathered part of eta spans 800, and with a ramp in the offset
    log mu itself spans more than 700 -- the log-likelihood stays finite and everything equals the reference."""
    rng = np.random.default_rng(700)
    n, q, nlevels, alpha = 4000, 2, (3, 5), 0.5
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.2
    c1, c2 = level_col[1], level_col[2]                         # levels 1 and 2 of factor 0
    beta[c1], beta[c2] = 400.0, -400.0
    o = -400.0 * (codes[:, 0] == 1) + 400.0 * (codes[:, 0] == 2) + np.linspace(-352.0, 352.0, n)
    y = rng.poisson(1.0, n).astype(np.float64)
    ll, g, H, mu = nr.terms(X, y, beta, alpha, o, False)[:4]
    assert np.ptp(X @ beta) > 700 and np.ptp(np.log(mu)) > 700 and np.isfinite(ll) and np.all(np.isfinite(H)) and np.all(np.isfinite(g))
    H2, g2, ll2, _, _ = _check_pass(plan, num, codes, y, o, beta, alpha, X, "eta>700", theta=False)
    assert math.isfinite(float(ll2.item())) and bool(torch.isfinite(g2).all()) and bool(torch.isfinite(H2).all())


def test_pass_stays_finite_where_alpha_mu_overflows(api):
    """one numeric column with coefficient 1 (eta is the column itself) and a factor whose rows all sit on the baseline: alpha mu
    overflows above eta = 709.78 - log(alpha) while mu is finite up to 709.78 -- w, g and loglik take NbRow's limits, as in
    test_gpu_negbin.test_pass_stays_finite_where_alpha_mu_overflows"""
    from dlsa_amd import engine
    x = np.array([-800.0, -746.0, -700.0, 0.0, 700.0, 705.0, 709.0, 709.7])
    n, alpha = len(x), 1e3
    arr = lambda v, t: np.asarray(v, dtype=t)
    desc = (arr([1, 2], np.int32), arr([0, 0], np.int32), arr([0, 1], np.int32), arr([0.0, 0.0], np.float64), arr([1.0, 1.0], np.float64))
    plan = _plan(api, 2, desc, [2], [-1, 1])
    num, codes, y, beta = x[:, None].copy(), np.zeros((n, 1), np.int32), np.full(n, 3.0), np.array([1.0, 0.0])
    H, g, ll, w, mu, _ = engine.onehot_negbin_pass(plan, dev(num), dev(codes), dev(y), dev(beta), alpha, want_w=True)
    w, mu = w.cpu().numpy(), mu.cpu().numpy()
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(mu)) and math.isfinite(float(ll.item())) and bool(torch.isfinite(g).all())
    assert bool(torch.isfinite(H).all())
    assert np.all(w[x >= 700] == 1.0 / alpha) and np.all(w[x <= -746] == 0.0)
    # the reference's limits: r = (y - mu) q -> -1 / alpha where alpha mu overflowed; g = sum x r over the column
    with np.errstate(over="ignore"):
        q_ = 1.0 / (1.0 + alpha * mu)
        r = np.where(alpha * mu > 1e300, -1.0 / alpha, (y - mu) * q_)
    assert abs(float(g[0].item()) - float(np.sum(x * r))) <= 1e-12 * float(np.sum(np.abs(x * r)))
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    th = 1 / mp.mpf(alpha)
    want = sum(mp.loggamma(3 + th) - mp.loggamma(th) - mp.loggamma(4) + th * mp.log(th) + 3 * mp.mpf(v) - (th + 3) * mp.log(th + mp.exp(mp.mpf(v)))
               for v in x)
    assert abs(float(ll.item()) - float(want)) <= 1e-12 * abs(float(want))
    # past 709.78 mu itself is +inf: the driver's failed step
    ll2 = engine.onehot_negbin_pass(plan, dev(np.array([[0.0], [720.0]])), dev(codes[:2]), dev(y[:2]), dev(beta), alpha, want_H=False)[2]
    assert float(ll2.item()) == -math.inf


# ---- fit ----------------------------------------------------------------------------------------------------------------
def _nb_case(orc, n, q, nlevels, seed, alpha, intercept=True):
    """a design of _random_design (uniform level frequencies) with NB2(mu, alpha) counts, mu = exposure * exp(X bt), bt ~ 0.2 N(0, 1)
    and, with an intercept, bt[0] = 0.5: a mean count near 2, so that every level has events and the dispersion is well determined"""
    rng = np.random.default_rng(seed)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels, intercept=intercept)
    X, _ = orc.design_matrix(num, codes, *desc)
    bt = rng.normal(size=p) * 0.2
    bt[:q + (1 if intercept else 0)] *= 0.25          # the standardised numerics reach +-10
    if intercept:
        bt[0] = 0.5
    e = rng.uniform(0.5, 2.0, n)
    y = rng.poisson(e * np.exp(X @ bt) * rng.gamma(1.0 / alpha, alpha, n)).astype(np.float64)
    return p, num, codes, desc, nl, level_col, X, y, e


# the fit cases: 12000 rows, 2 numerics, factors of 6, 4 and 9 levels (p = 19; 19 levels in all, >= 660 rows of every level in either
# half).  With these seeds tests/negbin_reference.fit converges on both partitions, contiguous and i % 2, with alpha-hat > 0 (checked
# on the CPU with nr.fit alone before the seeds were committed; test_fit_matches_reference asserts it again).
FIT_SHAPE = (12_000, 2, (6, 4, 9))
_REF = {}


def _fit_reference(orc, alpha, strided):
    """the case and the reference's fit of its two partitions, computed once per (alpha, strided) and shared"""
    key = (alpha, strided)
    if key not in _REF:
        n, q, nlevels = FIT_SHAPE
        case = _nb_case(orc, n, q, nlevels, 1000 + int(alpha * 10), alpha)
        X, y, e = case[6], case[7], case[8]
        parts = [slice(k, n, 2) for k in range(2)] if strided else [slice(0, n // 2), slice(n // 2, n)]
        _REF[key] = (case, parts, [nr.fit(X[sl], y[sl], np.log(e[sl]), False) for sl in parts])
    return _REF[key]


def _fit_ex(api, case, parts, strided, **kw):
    from dlsa_amd import engine
    p, num, codes, desc, nl, level_col, X, y, e = case
    n = len(y)
    if strided:
        first, rows, step = [0, 1], [len(range(k, n, 2)) for k in range(2)], 2
    else:
        first, rows, step = [s.start for s in parts], [s.stop - s.start for s in parts], 1
    plan = _plan(api, p, desc, nl, level_col)
    return engine.onehot_negbin_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step, offset=dev(np.log(e)), **kw)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_fit_matches_reference(api, orc, alpha, strided):
    case, parts, refs = _fit_reference(orc, alpha, strided)
    r = _fit_ex(api, case, parts, strided)
    assert r["status"] == [0, 0], r["status"]
    for k, (b, H, ll, a, info, pearson) in enumerate(refs):
        assert a > 0 and r["alpha"][k] > 0
        figs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H), rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b),
                abs(r["loglik"][k] - ll) / abs(ll), abs(r["alpha"][k] - a) / a, abs(r["alpha_info"][k] - info) / info,
                abs(r["pearson"][k] - pearson) / pearson)
        print("fit alpha=%g strided=%s partition %d: alpha_hat %.6f, %d row passes, rel err coef %.1e Sig_inv %.1e Sig_invMcoef %.1e "
              "loglik %.1e alpha %.1e alpha_info %.1e pearson %.1e" % ((alpha, strided, k, r["alpha"][k], r["n_iter"][k]) + figs))
        assert max(figs[:4]) <= TOL_FIT, figs
        assert figs[4] <= 1e-9 and figs[5] <= 1e-6 and figs[6] <= 1e-9, figs


@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_fit_is_stationary(api, orc, alpha):
    """a certificate that does not depend on the reference's route: both scores vanish at the returned (coef, alpha)"""
    case, parts, _ = _fit_reference(orc, alpha, True)
    X, y, e = case[6], case[7], case[8]
    r = _fit_ex(api, case, parts, True)
    assert r["status"] == [0, 0]
    for k, sl in enumerate(parts):
        b, a = r["coef"][k].cpu().numpy(), r["alpha"][k]
        _, g, H, _, s, i, _ = nr.terms(X[sl], y[sl], b, a, np.log(e[sl]), False)
        db = float(np.max(np.abs(np.linalg.solve(H, g))))
        print("stationarity alpha=%g partition %d: |H^-1 g| %.1e, |s/(i theta)| %.1e" % (alpha, k, db, abs(s * a / i)))
        assert db <= 1e-10 * max(1.0, float(np.max(np.abs(b))))
        assert abs(s * a / i) <= 1e-9


def test_fixed_alpha_fit(api, orc):
    case, parts, _ = _fit_reference(orc, 1.0, False)
    X, y, e = case[6], case[7], case[8]
    r = _fit_ex(api, case, parts, False, alpha=0.3)
    assert r["status"] == [0, 0] and r["alpha"] == [0.3, 0.3]
    for k, sl in enumerate(parts):
        b, H, ll, a, info, pearson = nr.fit(X[sl], y[sl], np.log(e[sl]), False, alpha=0.3)
        figs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H), abs(r["loglik"][k] - ll) / abs(ll),
                abs(r["alpha_info"][k] - info) / info, abs(r["pearson"][k] - pearson) / pearson)
        print("fixed alpha partition", k, figs)
        assert max(figs[:3]) <= TOL_FIT and figs[3] <= 1e-6 and figs[4] <= 1e-9, figs


def _compare_blocks(a, d, tag):
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(d, f).cpu().numpy())
        print(tag, f, "%.2e" % err)
        assert err <= TOL_FIT
    figs = (rel(a.loglik, d.loglik), rel(a.extra["alpha"], d.extra["alpha"]), rel(a.extra["alpha_info"], d.extra["alpha_info"]),
            rel(a.extra["pearson"], d.extra["pearson"]))
    print(tag, "loglik %.2e alpha %.2e alpha_info %.2e pearson %.2e" % figs)
    assert figs[0] <= TOL_FIT and figs[1] <= 1e-9 and figs[2] <= 1e-6 and figs[3] <= 1e-9


def test_structured_equals_dense_and_strided_equals_contiguous(api, orc):
    """fit_negbin_design(structured=True) against structured=False on the same rows.  The design has no constant column: the dense
    fit of the built matrix then starts where the structured one does (beta = 0; with a constant column the structured Poisson start
    puts it at log(sum y / sum e^o) and the built matrix's does not, see tests/test_gpu_onehot_poisson.py), so the two take the same
    evaluations and n_iter and status are compared too."""
    n, q, nlevels, K = 15_001, 2, (5, 4, 6), 3
    p, num, codes, desc, nl, level_col, X, y, e = _nb_case(orc, n, q, nlevels, 41, 0.5, intercept=False)
    spec = _spec(api, q, nlevels, desc)
    assert spec.onehot_plan() is not None
    dn, dc, dy, de = dev(num), dev(codes), dev(y), dev(e)
    a = api.fit_negbin_design(dn, dc, dy, spec, partition_num=K, exposure=de)
    d = api.fit_negbin_design(dn, dc, dy, spec, partition_num=K, exposure=de, structured=False)
    print("structured / dense n_iter", a.n_iter, d.n_iter, "status", a.status, d.status, "alpha", a.extra["alpha"])
    assert a.status == [0] * K and d.status == [0] * K and a.names == spec.names and d.names == spec.names
    assert all(v > 0 for v in a.extra["alpha"]) and set(a.extra) == {"alpha", "alpha_info", "pearson"}
    _compare_blocks(a, d, "structured vs dense")
    assert a.n_iter == d.n_iter
    # the same with a constant column (values only)
    p2, num2, codes2, desc2, nl2, lc2, X2, y2, e2 = _nb_case(orc, n, q, nlevels, 42, 0.5)
    spec2 = _spec(api, q, nlevels, desc2)
    a2 = api.fit_negbin_design(dev(num2), dev(codes2), dev(y2), spec2, partition_num=K, exposure=dev(e2))
    d2 = api.fit_negbin_design(dev(num2), dev(codes2), dev(y2), spec2, partition_num=K, exposure=dev(e2), structured=False)
    assert a2.status == [0] * K and d2.status == [0] * K
    _compare_blocks(a2, d2, "structured vs dense, with a constant column")
    # strided partitions equal contiguous copies of their rows
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    c = api.fit_negbin_design(dev(num[perm]), dev(codes[perm]), dev(y[perm]), spec, part_offsets=offs, offset=dev(np.log(e[perm])))
    assert c.status == [0] * K and c.n_iter == a.n_iter
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(c, f).cpu().numpy())
        print("strided vs contiguous", f, "%.2e" % err)
        assert err <= 1e-13
    assert rel(a.extra["alpha"], c.extra["alpha"]) <= 1e-13
    with pytest.raises(ValueError):
        api.fit_negbin_design(dn, dc, dy, spec, offset=torch.log(de), exposure=de)
    with pytest.raises(ValueError):
        api.fit_negbin_design(dn, dc, -dy - 1.0, spec)
    with pytest.raises(ValueError):
        api.fit_negbin_design(dn, dc, dy, spec, alpha=0.0)               # alpha = 0 is fit_poisson_design


def _poisson_mle_at_the_start(orc, seed, n, q, nlevels):
    """a design with a constant column and 'counts' (real numbers: only the host loop is under test) whose Poisson MLE is the fit's own
    start -- the constant column at log(sum y / sum e^o), zeros elsewhere: y = mu + r with r orthogonal to every column.  The
    construction of tests/test_gpu_negbin.py on the columns of a one-hot design."""
    rng = np.random.default_rng(seed)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    X, _ = orc.design_matrix(num, codes, *desc)
    assert desc[0][0] == 0 and np.all(X[:, 0] == 1.0)           # column 0 is the plan's constant column
    o = np.log(rng.uniform(0.5, 2.0, n))
    mu = 3.0 * np.exp(0.3 + o)
    z = rng.standard_normal(n) * mu
    r = z - X @ np.linalg.lstsq(X, z, rcond=None)[0]
    r *= 0.9 * np.min(mu / np.abs(r))
    return p, num, codes, desc, nl, level_col, X, mu + r, o


@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_max_iter_counts_passes_as_the_dense_fit_does(api, orc, max_iter):
    """one driver behind both fits (as test_gpu_negbin.test_budget_counts_the_poisson_start_and_advances_after_the_last_pass): one
    partition of 600 rows at a fixed alpha whose Poisson start converges at once, so the budget cuts the NB2 loop -- the row passes
    are the Poisson start's, the pass for mu at the Poisson MLE and max_iter + 1 evaluations, coef is one step beyond where Sig_inv
    was evaluated, and the dense fit of the built matrix's other columns with the implicit intercept counts the same."""
    import newton_reference as nw
    from dlsa_amd import engine
    n, alpha = 600, 0.5
    p, num, codes, desc, nl, level_col, X, y, o = _poisson_mle_at_the_start(orc, 9, n, 2, (3,))
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc, dy, do = dev(num), dev(codes), dev(y), dev(o)
    rp = engine.onehot_poisson_fit_ex(plan, dn, dc, dy, [0], [n], offset=do, max_iter=max_iter)
    assert rp["status"] == [0]
    bp = rp["coef"][0].cpu().numpy()
    evals, bs, lls = nw.undamped(lambda b: nr.terms(X, y, b, alpha, o, False)[:3], bp, 1e-13)
    assert evals is not None and evals > max_iter + 1 and nw.monotone(lls[:max_iter + 1])       # no halving in the budget
    r = engine.onehot_negbin_fit_ex(plan, dn, dc, dy, [0], [n], offset=do, alpha=alpha, max_iter=max_iter)
    d = engine.negbin_fit_ex(dev(X[:, 1:]), dy, [0], [n], offset=do, fit_intercept=True, alpha=alpha, max_iter=max_iter)
    print("max_iter", max_iter, "n_iter", r["n_iter"], d["n_iter"], "poisson start", rp["n_iter"], "status", r["status"], "rc", r["rc"])
    assert r["status"] == [1] and r["rc"] == 5
    assert r["n_iter"] == [rp["n_iter"][0] + max_iter + 2]
    assert r["n_iter"] == d["n_iter"] and r["status"] == d["status"] and r["rc"] == d["rc"]
    assert rel(r["coef"][0].cpu().numpy(), bs[max_iter + 1]) <= 1e-10
    assert rel(r["Sig_inv"][0].cpu().numpy(), nr.terms(X, y, bs[max_iter], alpha, o, False)[2]) <= 1e-10


def test_underdispersed_partition_is_the_poisson_block(api, orc):
    rng = np.random.default_rng(8)
    n, q, nlevels, K = 12_000, 2, (4, 3), 3
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    X, _ = orc.design_matrix(num, codes, *desc)
    bt = rng.normal(size=p) * 0.05
    bt[0] = 0.2
    mu = np.exp(X @ bt)
    assert mu.max() < 4
    y = rng.binomial(4, mu / 4).astype(np.float64)              # the Poisson mean with the variance mu (1 - mu / 4)
    spec = _spec(api, q, nlevels, desc)
    dn, dc, dy = dev(num), dev(codes), dev(y)
    a = api.fit_negbin_design(dn, dc, dy, spec, partition_num=K)
    b = api.fit_poisson_design(dn, dc, dy, spec, partition_num=K)
    assert a.status == [0] * K and a.extra["alpha"] == [0.0] * K and a.extra["alpha_info"] == [0.0] * K
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik
    assert all(0 < v < n / K for v in a.extra["pearson"])       # Pearson below the rows: underdispersed
    assert api.combine_dispersion(a) == 0.0


def test_fit_empty_and_all_zero_partitions(api, orc):
    from dlsa_amd import engine
    n, q, nlevels = 8000, 2, (4, 3)
    p, num, codes, desc, nl, level_col, X, y, e = _nb_case(orc, n, q, nlevels, 50, 0.5)
    y[2000:4000] = 0.0
    offs = [0, 2000, 4000, 4000, n]
    plan = _plan(api, p, desc, nl, level_col)
    r = engine.onehot_negbin_fit_ex(plan, dev(num), dev(codes), dev(y), offs[:-1], [offs[k + 1] - offs[k] for k in range(4)],
                                    offset=dev(np.log(e)))
    assert r["status"] == [0, 4, 4, 0], r["status"]
    for k in (1, 2):
        assert not r["Sig_inv"][k].any() and not r["coef"][k].any() and not r["Sig_invMcoef"][k].any()
        assert r["loglik"][k] == 0.0 and r["alpha"][k] == 0.0 and r["alpha_info"][k] == 0.0
    b, H, ll, a, info, pearson = nr.fit(X[4000:], y[4000:], np.log(e[4000:]), False)
    assert a > 0 and rel(r["coef"][3].cpu().numpy(), b) <= TOL_FIT and rel(r["Sig_inv"][3].cpu().numpy(), H) <= TOL_FIT
    assert abs(r["alpha"][3] - a) <= 1e-9 * a


def test_invalid_counts_are_refused_and_arguments_checked(api, orc):
    from dlsa_amd import engine, _lib
    import ctypes
    n, q, nlevels = 1000, 2, (4, 3)
    p, num, codes, desc, nl, level_col, X, y, e = _nb_case(orc, n, q, nlevels, 61, 0.5)
    o = np.log(e)
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc = dev(num), dev(codes)
    fit = lambda yy, oo: engine.onehot_negbin_fit_ex(plan, dn, dc, dev(yy), [0, 500], [500, 500], offset=dev(oo))
    y_bad = y.copy(); y_bad[700] = -1.0
    with pytest.raises(_lib.DlsaError) as ex:
        fit(y_bad, o)
    assert ex.value.code == 1 and "partition 1" in str(ex.value) and "onehot_negbin_fit" in str(ex.value)
    y_nan = y.copy(); y_nan[3] = np.nan
    with pytest.raises(_lib.DlsaError) as ex:
        fit(y_nan, o)
    assert ex.value.code == 1 and "partition 0" in str(ex.value)
    y_inf = y.copy(); y_inf[999] = np.inf
    with pytest.raises(_lib.DlsaError) as ex:
        fit(y_inf, o)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    o_bad = o.copy(); o_bad[600] = np.inf
    with pytest.raises(_lib.DlsaError) as ex:
        fit(y, o_bad)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    # the pass reports an invalid count as a NaN log-likelihood
    ll = engine.onehot_negbin_pass(plan, dn, dc, dev(y_bad), dev(np.zeros(p)), 0.5, want_H=False)[2]
    assert math.isnan(float(ll.item()))
    with pytest.raises(ValueError):
        engine.onehot_negbin_pass(plan, dn, dc, dev(y), dev(np.zeros(p)), 0.0)
    with pytest.raises(ValueError):
        engine.onehot_negbin_fit_ex(plan, dn, dc, dev(y), [0], [n], alpha=float("inf"))
    # argument checks that need a plan (before any launch), and the workspace query
    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    # pass(plan, num, ldn, codes, ldc, y, offset, beta, alpha, n, H, ldh, g, loglik, w_out, mu_out, theta_terms, ws, ws_bytes, stream)
    args = [plan._h, fake, q, fake, len(nlevels), fake, None, fake, 0.5, 10, fake, p, None, None, None, None, None, fake, 1 << 30, None]
    for i, v in ((1, None), (3, None), (9, 0), (2, q - 1), (4, len(nlevels) - 1), (11, p - 1), (8, 0.0), (8, -1.0), (8, float("inf")),
                 (8, float("nan"))):
        a = list(args); a[i] = v
        assert lib.dlsa_onehot_negbin_pass_f64(*a) == 1, (i, v)
    a = list(args); a[18] = 1024
    assert lib.dlsa_onehot_negbin_pass_f64(*a) == 3
    a = list(args); a[17] = ctypes.c_void_p(257)
    assert lib.dlsa_onehot_negbin_pass_f64(*a) == 3
    first, rows = (ctypes.c_int64 * 2)(0, 5), (ctypes.c_int64 * 2)(5, 5)
    fargs = [plan._h, fake, q, fake, len(nlevels), fake, None, first, rows, 1, 2, 0.0, 1e-13, 100, fake, fake, fake, None, None, None, None,
             None, None, fake, 1 << 30, None]
    for i, v in ((9, 0), (10, 0), (12, 0.0), (13, 0), (2, q - 1), (4, len(nlevels) - 1), (11, float("inf"))):
        a = list(fargs); a[i] = v
        assert lib.dlsa_onehot_negbin_fit_f64(*a) == 1, (i, v)
    a = list(fargs); a[8] = (ctypes.c_int64 * 2)(5, -1)
    assert lib.dlsa_onehot_negbin_fit_f64(*a) == 1 and "partition 1" in _lib.last_error()
    a = list(fargs); a[24] = 4096
    assert lib.dlsa_onehot_negbin_fit_f64(*a) == 3
    prev = 0
    for rows_ in (0, 1, 63, 64, 65, 1000, 4096 * 64, 10 ** 6, 10 ** 7, 2 * 10 ** 7):
        for step in (1, 7):
            b = lib.dlsa_onehot_negbin_workspace_bytes(plan._h, rows_, step)
            assert b > 0 and b >= lib.dlsa_onehot_negbin_workspace_bytes(plan._h, rows_, 1)
            assert b >= lib.dlsa_onehot_poisson_workspace_bytes(plan._h, rows_, step)
        b = lib.dlsa_onehot_negbin_workspace_bytes(plan._h, rows_, 1)
        assert b >= prev, rows_
        prev = b
    assert lib.dlsa_onehot_negbin_workspace_bytes(plan._h, -1, 1) == 0 and lib.dlsa_onehot_negbin_workspace_bytes(plan._h, 10, 0) == 0


def test_fit_is_bit_reproducible(api, orc):
    n, q, nlevels, K = 60_000, 7, (11, 6, 20, 110, 110), 3
    p, num, codes, desc, nl, level_col, X, y, e = _nb_case(orc, n, q, nlevels, 80, 0.5)
    spec = _spec(api, q, nlevels, desc)
    dn, dc, dy, de = dev(num), dev(codes), dev(y), dev(e)
    a = api.fit_negbin_design(dn, dc, dy, spec, partition_num=K, exposure=de)
    b = api.fit_negbin_design(dn, dc, dy, spec, partition_num=K, exposure=de)
    assert all(v > 0 for v in a.extra["alpha"])
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik and a.extra == b.extra and a.n_iter == b.n_iter and a.status == b.status


def test_end_to_end_dlsa(api, orc):
    n, q, nlevels, K = 40_000, 3, (6, 4, 9), 4
    p, num, codes, desc, nl, level_col, X, y, e = _nb_case(orc, n, q, nlevels, 90, 0.5)
    o = np.log(e)
    spec = _spec(api, q, nlevels, desc)
    mb = api.fit_negbin_design(dev(num), dev(codes), dev(y), spec, partition_num=K, offset=dev(o))
    md = api.fit_negbin_design(dev(num), dev(codes), dev(y), spec, partition_num=K, offset=dev(o), structured=False)
    assert mb.status == [0] * K and md.status == [0] * K and all(v > 0 for v in mb.extra["alpha"])
    out, outd = api.dlsa_mapred(mb), api.dlsa_mapred(md)
    for c in ("beta_byOLS", "beta_byONESHOT"):
        assert rel(out[c].to_numpy(), outd[c].to_numpy()) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), outd.iloc[:, 2:].to_numpy()) <= 1e-10
    res = api.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    resd = api.dlsa(outd.iloc[:, 2:].to_numpy(), outd["beta_byOLS"].to_numpy(), n)
    for c in ("beta_byBIC", "beta_byAIC"):
        print("end to end", c, "%.2e" % rel(res[c].to_numpy(), resd[c].to_numpy()))
        assert rel(res[c].to_numpy(), resd[c].to_numpy()) <= 1e-10
    # and against the reference's blocks of one partition
    b, H, _ = nr.block(X[1::K], y[1::K], o[1::K], False)
    assert rel(mb.coef[1].cpu().numpy(), b) <= TOL_FIT and rel(mb.Sig_inv[1].cpu().numpy(), H) <= TOL_FIT
    assert abs(api.combine_dispersion(mb) - api.combine_dispersion(md)) <= 1e-9 * api.combine_dispersion(md)


# ---- frames -------------------------------------------------------------------------------------------------------------
def _nb_frame(seed, n, alpha=0.6):
    """the frame of tests/test_gpu_onehot_poisson.py with gamma-mixed counts of the same mean"""
    df, dummy_info, baseline, names, Xo = _frame(seed, n)
    rng = np.random.default_rng(seed + 1000)
    eta = -0.3 + 0.1 * (df["dist"] - 5) - 0.02 * (df["age"] - 40) + 0.4 * (df["carrier"] == "BB") - 0.3 * (df["carrier"] == "CC") \
        + 0.2 * (df["region"] == "s") - 0.25 * (df["region"] == "w")
    df["y"] = rng.poisson(df["expo"] * np.exp(eta) * rng.gamma(1.0 / alpha, alpha, n)).astype(float)
    return df, dummy_info, baseline, names, Xo


def test_negbin_model_structured_frame_and_eval(api):
    import pandas as pd
    df, dummy_info, baseline, names, Xo = _nb_frame(2, 6000)
    kw = dict(fit_intercept=True, exposure_name="expo", dummy_info=dummy_info, dummy_factors_baseline=baseline)
    out = api.negbin_model(df, "y", structured=True, **kw)
    dense = api.negbin_model(df, "y", structured=False, **kw)
    default = api.negbin_model(df, "y", **kw)
    want = ["par_id", "coef", "Sig_invMcoef"] + names
    assert list(out.columns) == want and list(dense.columns) == want
    assert default.equals(dense) and default.to_numpy().tobytes() == dense.to_numpy().tobytes()      # the default is the dense path
    assert default.attrs["alpha"] == dense.attrs["alpha"]
    figs = (rel(out["coef"], dense["coef"]), rel(out[names].to_numpy(), dense[names].to_numpy()),
            rel(out["Sig_invMcoef"], dense["Sig_invMcoef"]), abs(out.attrs["alpha"] - dense.attrs["alpha"]) / dense.attrs["alpha"])
    print("negbin_model structured vs dense", figs, "alpha", out.attrs["alpha"])
    assert dense.attrs["alpha"] > 0 and max(figs) <= TOL_FIT
    o = np.log(df["expo"].to_numpy())
    b, H, ll, a, _, _ = nr.fit(Xo, df["y"].to_numpy(), o, True)
    assert rel(out["coef"], b) <= TOL_FIT and rel(out[names].to_numpy(), H) <= TOL_FIT and abs(out.attrs["alpha"] - a) <= 1e-9 * a
    # a missing level: the zero block and the reference's warning, from the codes
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = api.negbin_model(sub, "y", structured=True, **kw)
    assert any("missing in this data chunk" in str(w.message) and "Skip modeling" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (8, 11) and float(np.abs(zero.to_numpy()).max()) == 0.0
    assert zero.attrs["alpha"] == 0.0
    # eval: the log-likelihood of each estimator column at the fitted dispersion
    par = pd.DataFrame({"mle": out["coef"].to_numpy(), "ref": b, "zero": np.zeros(8)})
    al = out.attrs["alpha"]
    ev = api.negbin_model_eval(df, "y", par, al, structured=True, **kw)
    assert list(ev.columns) == ["mle", "ref", "zero"] and ev.shape == (1, 3)
    evd = api.negbin_model_eval(df, "y", par, al, structured=False, **kw)
    ev0 = api.negbin_model_eval(df, "y", par, al, **kw)
    assert ev0.to_numpy().tobytes() == evd.to_numpy().tobytes()
    print("negbin_model_eval structured vs dense %.2e" % rel(ev.to_numpy()[0], evd.to_numpy()[0]))
    assert rel(ev.to_numpy()[0], evd.to_numpy()[0]) <= TOL_FIT
    refs = [nr.terms(Xo, df["y"].to_numpy(), par[c].to_numpy(), al, o, True)[0] for c in par.columns]
    assert rel(ev.to_numpy()[0], refs) <= 1e-12


# ---- at scale -----------------------------------------------------------------------------------------------------------
def test_at_scale_fit_on_raw_rows(api):
    from conftest import need_hbm
    from dlsa_amd import engine
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench"))
    import surrogates                            # bench/surrogates.py: test / bench data, not product code
    need_hbm(8e9)
    n, K, alpha = 14_000_000, 14, 0.5
    d = surrogates.airline_shaped(n, dense=False)
    num, codes, beta, plan = d["num"], d["codes"], d["beta"], d["plan"]
    q, levels = num.shape[1], d["levels"]
    g = torch.Generator(device="cuda").manual_seed(5)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    eta = beta[0] + ((num - 1.5) / 3.0) @ beta[1:1 + q]
    pos = 1 + q
    for fi, L in enumerate(levels):
        tab = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), beta[pos:pos + L - 1]])
        eta = eta + tab[codes[:, fi].long()]
        pos += L - 1
    u = torch.rand((2, n), dtype=torch.float64, device="cuda", generator=g).clamp_min_(1e-300)
    mix = -alpha * (torch.log(u[0]) + torch.log(u[1]))           # Gamma(2, 1/2): NB2 with alpha = 0.5
    y = torch.poisson(torch.exp(eta + o) * mix, generator=g)
    del eta, tab, u, mix, d["y"]
    raw = num.numel() * 8 + codes.numel() * 4 + y.numel() * 8 + o.numel() * 8
    assert abs(raw - 1.288e9) < 1e6
    torch.cuda.synchronize()
    engine.release_workspace()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    r = engine.onehot_negbin_fit_ex(plan, num, codes, y, first, rows, row_step=K, offset=o)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("at scale: peak %.3f GB, raw %.3f GB, iters %s, alpha %s" % (peak / 1e9, raw / 1e9, r["n_iter"], r["alpha"]))
    assert peak < raw + 1e9, (peak, raw)
    assert r["status"] == [0] * K, r["status"]
    # alpha-hat of 1e6 rows: its standard error is 1 / sqrt(alpha_info) in log alpha; five of them around the truth
    for k in range(K):
        z = abs(math.log(r["alpha"][k] / alpha)) * math.sqrt(r["alpha_info"][k])
        assert z <= 5.0, (k, r["alpha"][k], z)
    # one partition's block against a pass of its own at the returned (coef, alpha)
    k = 3
    nk, ck, ok, yk = num[k::K].contiguous(), codes[k::K].contiguous(), o[k::K].contiguous(), y[k::K].contiguous()
    H, gs, ll, _, _, tt = engine.onehot_negbin_pass(plan, nk, ck, yk, r["coef"][k].contiguous(), r["alpha"][k], offset=ok, want_theta=True)
    Hn = H.cpu().numpy()
    step = float(np.max(np.abs(np.linalg.solve(Hn, gs.cpu().numpy()))))
    s_, i_ = float(tt[0].item()), float(tt[1].item())
    print("partition", k, "|H^-1 g| %.2e" % step, "|s / (i theta)| %.2e" % abs(s_ * r["alpha"][k] / i_))
    assert step <= 1e-10 * max(1.0, float(r["coef"][k].abs().max())) and abs(s_ * r["alpha"][k] / i_) <= 1e-9
    assert np.array_equal(Hn, Hn.T) and rel(Hn, r["Sig_inv"][k].cpu().numpy()) <= 1e-12
    assert abs(float(ll.item()) - r["loglik"][k]) <= 1e-12 * abs(r["loglik"][k])
