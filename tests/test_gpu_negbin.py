"""GPU: the negative-binomial (NB2) map step (csrc/negbin.hip) against the numpy / scipy reference (tests/negbin_reference.py) and
mpmath: the pass at a fixed (beta, alpha) at every Gram width class, the device digamma / trigamma, the per-partition fit and its
stationarity, the alpha = 0 and fixed-alpha branches, strided partitions, edge cases, reproducibility, the end-to-end DLSA combine,
the calibration of Sig_inv on overdispersed counts, the frame-level negbin_model and a 1e7 x 100 fit."""
import math
import warnings

import numpy as np
import pytest

import negbin_reference as nr
import newton_reference as nw
import poisson_reference as pr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WIDTHS = [1, 7, 50, 100, 130, 260, 500, 600]


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


def _dev(*arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _theta_terms_mp(y, mu, alpha):
    """(s, i, pearson) of the rows (y, mu) in 50 digits (mpmath), from the textbook forms; the special functions once per distinct y"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    th = 1 / mp.mpf(alpha)
    d1 = {v: mp.digamma(mp.mpf(v) + th) - mp.digamma(th) for v in np.unique(y)}
    d2 = {v: mp.polygamma(1, th) - mp.polygamma(1, mp.mpf(v) + th) for v in np.unique(y)}
    s = i = pe = mp.mpf(0)
    lt = mp.log(th)
    for yv, mv in zip(y, mu):
        yy, m = mp.mpf(yv), mp.mpf(mv)
        s += d1[yv] + lt + 1 - mp.log(th + m) - (yy + th) / (m + th)
        i += d2[yv] - 1 / th + 2 / (m + th) - (yy + th) / (m + th) ** 2
        pe += (yy - m) ** 2 / (m + mp.mpf(alpha) * m * m)
    return s, i, pe


def _check_pass(eng, X, y, o, beta, alpha, intercept, tol=1e-12, theta=True, Xd=None):
    """Xd: the device tensor to pass for X (a view with its own pitch / alignment); default a contiguous copy"""
    Xc, yd, od, bd = _dev(X, y, o, beta)
    H, g, ll, w, mu, tt = eng.negbin_pass(Xc if Xd is None else Xd, yd, bd, alpha, offset=od, fit_intercept=intercept, want_w=True,
                                          want_theta=True)
    llr, gr, Hr, mur, sr, ir, per = nr.terms(X, y, beta, alpha, o, intercept)
    assert abs(float(ll.item()) - llr) <= tol * abs(llr), (float(ll.item()), llr)
    assert rel(g.cpu().numpy(), gr) <= tol, rel(g.cpu().numpy(), gr)
    assert rel(mu.cpu().numpy(), mur) <= tol
    assert rel(w.cpu().numpy(), mur / (1.0 + alpha * mur)) <= tol
    Hn = H.cpu().numpy()
    assert rel(Hn, Hr) <= tol, rel(Hn, Hr)
    assert np.array_equal(Hn, Hn.T)
    if not theta:
        return
    # s, i, pearson: the scipy reference's own error against mpmath on the same (y, mu); the kernel gets 10 times that.  In one sample
    # in ten the reference happens to land within 1e-18 of the truth, which is luck and not its accuracy: any fp64 evaluation of a sum
    # whose terms cancel carries an ulp of its terms, so the measured figure is not taken below eps sum |terms| / |sum|.
    truth = [float(v) for v in _theta_terms_mp(y, mur, alpha)]
    th = 1.0 / alpha
    from scipy import special
    mag = [float(np.sum(np.abs(special.digamma(y + th) - special.digamma(th)) + np.abs(np.log1p(alpha * mur)) + np.abs((mur - y) / (mur + th)))),
           float(np.sum(np.abs(special.polygamma(1, th) - special.polygamma(1, y + th)) + 1.0 / th + 2.0 / (mur + th) + (y + th) / (mur + th) ** 2)),
           truth[2]]
    got = tt.cpu().numpy()
    for name, t, r, k, m in zip(("s", "i", "pearson"), truth, (sr, ir, per), got, mag):
        e_ref, e_k = abs(r - t) / abs(t), abs(k - t) / abs(t)
        floor = np.finfo(float).eps * m / abs(t)
        print("negbin pass p=%d alpha=%g %s: scipy %.2e kernel %.2e floor %.2e" % (X.shape[1], alpha, name, e_ref, e_k, floor))
        assert e_k <= 10 * max(e_ref, floor), (name, e_k, e_ref, floor)


def _away_from_optimum(pe):
    return np.linspace(-0.8, 0.6, pe) / max(1.0, math.sqrt(pe / 10))


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("alpha", [0.05, 0.5, 5.0])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, False), (False, True), (True, True)])
def test_pass_matches_reference(eng, p, alpha, intercept, offset):
    n = 3001
    X, y, o = nr.data(10 + p, n, p, intercept, offset, alpha)
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), alpha, intercept)


# Shapes of the row pass no 3001-row case reaches (as tests/test_gpu_poisson.py: NC = 16 with one row per wave; fewer rows than one
# batch, where every prefetch at NC = 1 is a clamped re-read of row n - 1; one full and one partial batch at NC = 2).  theta=False:
# the theta kernel is not the pass's, and at n = 1 its sums can be exactly 0.
SHORT_AND_WIDE = [(67, 1025), (67, 1030), (1, 1), (1, 2), (5, 7), (7, 8), (9, 130), (13, 128)]


@pytest.mark.parametrize("n,p", SHORT_AND_WIDE)
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_short_and_wide_shapes(eng, n, p, intercept, offset):
    X, y, o = nr.data(900 + p + n, n, p, intercept, offset, 0.5)
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), 0.5, intercept, theta=False)


@pytest.mark.parametrize("p", [8, 130, 1030])
@pytest.mark.parametrize("pad", [3, 2])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_even_width_on_the_scalar_loads(eng, p, pad, intercept, offset):
    """an even p takes the scalar loads only through the rows' pitch or base: columns 1 .. p of a buffer with p + 3 columns (an odd
    pitch) and of one with p + 2 (an even pitch, the base 8 bytes off a 16-byte boundary), passed as views, without a copy"""
    n = 67
    X, y, o = nr.data(900 + p + n, n, p, intercept, offset, 0.5)
    big = torch.zeros((n, p + pad), dtype=torch.float64, device="cuda")
    Xd = big[:, 1:1 + p]
    Xd.copy_(torch.from_numpy(X))
    assert Xd.stride(0) == p + pad and Xd.stride(1) == 1
    if pad == 2:
        assert Xd.data_ptr() % 16 == 8
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), 0.5, intercept, theta=False, Xd=Xd)


def test_special_functions(eng):
    """the device digamma, trigamma and the two cancelling differences against mpmath (50 digits); the bound is 4 times the measured
    error of scipy.special on the same grid (digamma, polygamma(1), and the differences taken from scipy's digamma / gammaln)"""
    mp = pytest.importorskip("mpmath")
    from scipy import special
    mp.mp.dps = 50
    th, yy = np.meshgrid(np.logspace(-2, 6, 33), np.array([0.0, 1.0, 2.0, 10.0, 1e3, 1e6]), indexing="ij")
    th, yy = th.ravel(), yy.ravel()
    got = eng.negbin_special(*_dev(th, yy)).cpu().numpy()
    tm = [[mp.digamma(t), mp.polygamma(1, t), mp.digamma(t + v) - mp.digamma(t), mp.loggamma(t + v) - mp.loggamma(t) - v * mp.log(t)]
          for t, v in zip(map(mp.mpf, th), map(mp.mpf, yy))]
    with np.errstate(invalid="ignore"):
        ref = np.c_[special.digamma(th), special.polygamma(1, th), special.digamma(th + yy) - special.digamma(th),
                    special.gammaln(th + yy) - special.gammaln(th) - yy * np.log(th)]

    # where the true value is 0 (y = 0; y = 1 for the log-gamma difference, lgamma(1 + t) - lgamma(t) = log t) it must be met exactly:
    # those points are left out of both relative errors
    zero = np.zeros(got.shape, dtype=bool)
    zero[:, 2] = yy == 0
    zero[:, 3] = (yy == 0) | (yy == 1)
    assert np.all(got[zero] == 0.0)

    def err(a):     # relative to the true value
        e = np.zeros(a.shape)
        for r in range(a.shape[0]):
            for c in range(4):
                if not zero[r, c]:
                    e[r, c] = float(abs(mp.mpf(a[r, c]) - tm[r][c]) / abs(tm[r][c]))
        return e
    e_ref, e_k = err(ref), err(got)
    for c, name in enumerate(("digamma", "trigamma", "psi(y+t)-psi(t)", "lgamma(y+t)-lgamma(t)-y log t")):
        print("negbin special %s: scipy max rel err %.2e, kernel %.2e (worst at theta=%g y=%g)" % (
            name, e_ref[:, c].max(), e_k[:, c].max(), th[np.argmax(e_k[:, c])], yy[np.argmax(e_k[:, c])]))
        assert np.isfinite(e_ref[:, c].max()) and e_k[:, c].max() <= 4 * e_ref[:, c].max(), (name, e_k[:, c].max(), e_ref[:, c].max())


def test_pass_eta_spanning_700(eng):
    n, p = 2000, 3
    for intercept, offset, alpha in [(False, False, 0.5), (True, True, 5.0)]:
        X, y, o = nr.data(20, n, p, intercept, offset, alpha)
        X[:, 0] = np.linspace(-1.0, 1.0, n)
        beta = np.array([699.0, 0.3, -0.2]) if not intercept else np.array([-0.4, 699.0, 0.3, -0.2])
        ll, g, H, mu, s, i, pe = nr.terms(X, y, beta, alpha, o, intercept)
        assert np.ptp(np.log(mu[mu > 0])) > 1300 and np.isfinite(ll) and np.all(np.isfinite(H))
        _check_pass(eng, X, y, o, beta, alpha, intercept, theta=False)


def test_pass_stays_finite_where_alpha_mu_overflows(eng):
    # p = 1, beta = 1: eta is x itself.  alpha mu overflows above eta = 709.78 - log(alpha) while mu is finite up to 709.78
    x = np.array([-800.0, -746.0, -700.0, 0.0, 700.0, 705.0, 709.0, 709.7])
    Xd, yd, bd = _dev(x[:, None].copy(), np.full(len(x), 3.0), np.ones(1))
    alpha = 1e3
    H, g, ll, w, mu, _ = eng.negbin_pass(Xd, yd, bd, alpha, want_w=True)
    w, mu = w.cpu().numpy(), mu.cpu().numpy()
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(mu)) and math.isfinite(float(ll.item())) and bool(torch.isfinite(g).all())
    assert np.all(w[x >= 700] == 1.0 / alpha) and np.all(w[x <= -746] == 0.0)
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    th = 1 / mp.mpf(alpha)
    want = sum(mp.loggamma(3 + th) - mp.loggamma(th) - mp.loggamma(4) + th * mp.log(th) + 3 * mp.mpf(v) - (th + 3) * mp.log(th + mp.exp(mp.mpf(v)))
               for v in x)
    assert abs(float(ll.item()) - float(want)) <= 1e-12 * abs(float(want))
    # past 709.78 mu itself is +inf: the driver's failed step
    Xd2 = _dev(np.array([[0.0], [720.0]]))[0]
    _, _, ll2, _, _, _ = eng.negbin_pass(Xd2, yd[:2], bd, alpha, want_H=False)
    assert float(ll2.item()) == -math.inf


def _fit(eng, X, y, o, offs, intercept, **kw):
    Xd, yd, od = _dev(X, y, o)
    return eng.negbin_fit_ex(Xd, yd, offs[:-1], [offs[k + 1] - offs[k] for k in range(len(offs) - 1)], offset=od,
                             fit_intercept=intercept, **kw)


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_fit_matches_reference(eng, p, alpha):
    n, K = 2 * max(3000, 20 * p), 2
    X, y, o = nr.data(40 + p, n, p, True, True, alpha)
    offs = [k * n // K for k in range(K + 1)]
    r = _fit(eng, X, y, o, offs, True)
    assert r["status"] == [0] * K, r["status"]
    for k in range(K):
        sl = slice(offs[k], offs[k + 1])
        b, H, ll, a, info, pearson = nr.fit(X[sl], y[sl], o[sl], True)
        assert a > 0 and r["alpha"][k] > 0
        print("negbin fit p=%d alpha=%g part %d: alpha_hat %.6f, %d row passes, coef %.1e H %.1e alpha %.1e" % (
            p, alpha, k, r["alpha"][k], r["n_iter"][k], rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H),
            abs(r["alpha"][k] - a) / a))
        assert rel(r["coef"][k].cpu().numpy(), b) <= 1e-10
        assert rel(r["Sig_inv"][k].cpu().numpy(), H) <= 1e-10
        assert rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b) <= 1e-10
        assert abs(r["loglik"][k] - ll) <= 1e-10 * abs(ll)
        assert abs(r["alpha"][k] - a) <= 1e-9 * a
        assert abs(r["alpha_info"][k] - info) <= 1e-6 * info and abs(r["pearson"][k] - pearson) <= 1e-9 * pearson


@pytest.mark.parametrize("p", [7, 130, 600])
@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_fit_is_stationary(eng, p, alpha):
    """a certificate that does not depend on the reference's route: both scores vanish at the returned (coef, alpha)"""
    n = max(3000, 20 * p)
    X, y, o = nr.data(140 + p, n, p, True, True, alpha)
    r = _fit(eng, X, y, o, [0, n], True)
    assert r["status"] == [0] and r["alpha"][0] > 0
    b, a = r["coef"][0].cpu().numpy(), r["alpha"][0]
    _, g, H, _, s, i, _ = nr.terms(X, y, b, a, o, True)
    db = float(np.max(np.abs(np.linalg.solve(H, g))))
    print("negbin stationarity p=%d alpha=%g: |H^-1 g| %.1e, |s/(i theta)| %.1e" % (p, alpha, db, abs(s * a / i)))
    assert db <= 1e-10 * max(1.0, float(np.max(np.abs(b))))
    assert abs(s * a / i) <= 1e-9


def _underdispersed(seed, n, p):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    mu = np.exp(0.2 + X @ np.where(np.arange(p) < 2, 0.5, 0.0))
    return X, rng.binomial(4, mu / 4).astype(np.float64)


def test_underdispersed_partition_is_the_poisson_block(eng):
    import dlsa_amd
    X, y = _underdispersed(8, 12_000, 5)
    Xd, yd = _dev(X, y)
    a = dlsa_amd.fit_negbin_partitions(Xd, yd, partition_num=3, fit_intercept=True)
    b = dlsa_amd.fit_poisson_partitions(Xd, yd, partition_num=3, fit_intercept=True)
    assert a.status == [0] * 3 and a.extra["alpha"] == [0.0] * 3 and a.extra["alpha_info"] == [0.0] * 3
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik
    assert all(0 < v < 4000 for v in a.extra["pearson"])            # Pearson below n: underdispersed
    assert dlsa_amd.combine_dispersion(a) == 0.0


def test_fixed_alpha(eng):
    import dlsa_amd
    n, p = 6000, 9
    X, y, o = nr.data(33, n, p, True, True, 0.5)
    r = _fit(eng, X, y, o, [0, 3000, n], True, alpha=0.3)
    assert r["status"] == [0, 0] and r["alpha"] == [0.3, 0.3]
    for k, sl in enumerate((slice(0, 3000), slice(3000, n))):
        b, H, ll, a, info, pearson = nr.fit(X[sl], y[sl], o[sl], True, alpha=0.3)
        assert rel(r["coef"][k].cpu().numpy(), b) <= 1e-10 and rel(r["Sig_inv"][k].cpu().numpy(), H) <= 1e-10
        assert rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b) <= 1e-10 and abs(r["loglik"][k] - ll) <= 1e-10 * abs(ll)
        assert abs(r["alpha_info"][k] - info) <= 1e-6 * abs(info) and abs(r["pearson"][k] - pearson) <= 1e-9 * pearson
    with pytest.raises(ValueError, match="Poisson"):
        _fit(eng, X, y, o, [0, n], True, alpha=0)
    with pytest.raises(ValueError, match="Poisson"):
        dlsa_amd.fit_negbin_partitions(*_dev(X, y), alpha=0.0)
    with pytest.raises(ValueError):
        _fit(eng, X, y, o, [0, n], True, alpha=-1.0)


def _poisson_mle_at_the_start(seed, n, p):
    """rows whose Poisson MLE is the Poisson fit's own start (the intercept at log(sum y / sum e^o), slopes 0): y = mu + r with
    r orthogonal to [1 | X], heteroscedastic, scaled so that y > 0.  The Poisson start then converges at its first evaluation and
    every further row pass of a fixed-alpha NB2 fit belongs to the NB2 loop, whose score differs: it weighs r by 1 / (1 + alpha mu)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    o = np.log(rng.uniform(0.5, 2.0, n))
    D = np.column_stack([np.ones(n), X])
    mu = 3.0 * np.exp(0.3 + o)
    z = rng.standard_normal(n) * mu
    r = z - D @ np.linalg.lstsq(D, z, rcond=None)[0]
    r *= 0.9 * np.min(mu / np.abs(r))
    return X, mu + r, o


# Only the host loop is under test: one partition of 600 rows, p = 3, intercept and offset on, alpha fixed.
@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_budget_counts_the_poisson_start_and_advances_after_the_last_pass(eng, max_iter):
    n, p, alpha = 600, 3, 0.5
    X, y, o = _poisson_mle_at_the_start(9, n, p)
    Xd, yd, od = _dev(X, y, o)
    rp = eng.poisson_fit_ex(Xd, yd, [0], [n], offset=od, fit_intercept=True, max_iter=max_iter)
    assert rp["status"] == [0]
    bp = rp["coef"][0].cpu().numpy()
    # Fisher scoring at the fixed alpha from the Poisson MLE, undamped: 7 evaluations, so max_iter + 1 <= 4 never suffices
    evals, bs, lls = nw.undamped(lambda b: nr.terms(X, y, b, alpha, o, True)[:3], bp, 1e-13)
    assert evals is not None and evals > max_iter + 1 and nw.monotone(lls[:max_iter + 1])       # no halving in the budget
    r = _fit(eng, X, y, o, [0, n], True, alpha=alpha, max_iter=max_iter)
    assert r["status"] == [1] and r["rc"] == 5
    # the Poisson start's passes, the pass for mu at the Poisson MLE, and max_iter + 1 evaluations of the NB2 loop
    assert r["n_iter"] == [rp["n_iter"][0] + max_iter + 2]
    # the NB2 loop advances after its last evaluation: coef is iterate max_iter + 1, one step beyond where Sig_inv was evaluated
    assert rel(r["coef"][0].cpu().numpy(), bs[max_iter + 1]) <= 1e-10
    assert rel(r["Sig_inv"][0].cpu().numpy(), nr.terms(X, y, bs[max_iter], alpha, o, True)[2]) <= 1e-10


def test_far_start_is_halved(eng):
    """the far start of the Poisson suite through the fixed-alpha fit: the undamped iteration from the same start (beta = 0, no
    intercept) DIVERGES -- the first full step of the Poisson start overflows mu, its second evaluation is -inf -- so the fit
    gets past it only by halving.  (alpha = 1e-4: at a larger one the scoring without an intercept needs more than max_iter steps.)"""
    rng = np.random.default_rng(62)
    X = rng.uniform(-0.5, 0.5, (20_000, 3))
    y = rng.poisson(np.exp(5.0 + X @ np.array([4.0, -3.0, 2.0]))).astype(np.float64)
    evals, _, lls = nw.undamped(lambda b: pr.terms(X, y, b, None, False)[:3], np.zeros(3), 1e-13)
    assert evals is None and len(lls) == 2 and lls[1] == -math.inf
    r = _fit(eng, X, y, None, [0, 20_000], False, alpha=1e-4)
    print("far start, alpha 1e-4: %d row passes, the undamped iteration diverged at its second" % r["n_iter"][0])
    assert r["status"] == [0] and r["rc"] == 0
    assert r["n_iter"][0] > len(lls)
    b = nr.fit(X, y, None, False, alpha=1e-4)[0]
    assert rel(r["coef"][0].cpu().numpy(), b) <= 1e-10


def test_strided_partitions_equal_contiguous_copies(eng):
    import dlsa_amd
    n, p, K = 30_001, 8, 5
    X, y, o = nr.data(70, n, p, True, True, 0.5)
    e = np.exp(o)
    Xd, yd, ed = _dev(X, y, e)
    a = dlsa_amd.fit_negbin_partitions(Xd, yd, partition_num=K, fit_intercept=True, exposure=ed)
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    Xc, yc, ec = _dev(X[perm], y[perm], e[perm])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    b = dlsa_amd.fit_negbin_partitions(Xc, yc, part_offsets=offs, fit_intercept=True, exposure=ec)
    assert a.status == [0] * K and b.status == [0] * K
    assert a.names == ["intercept"] + ["x%d" % i for i in range(p)]
    assert rel(a.coef.cpu().numpy(), b.coef.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_inv.cpu().numpy(), b.Sig_inv.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_invMcoef.cpu().numpy(), b.Sig_invMcoef.cpu().numpy()) <= 1e-13
    assert rel(a.extra["alpha"], b.extra["alpha"]) <= 1e-11 and min(a.extra["alpha"]) > 0


def test_fit_empty_and_all_zero_partitions(eng):
    n, p = 6000, 4
    X, y, o = nr.data(50, n, p, True, True, 0.5)
    y[2000:4000] = 0.0
    offs = [0, 2000, 4000, 4000, n]
    r = _fit(eng, X, y, o, offs, True)
    assert r["status"] == [0, 4, 4, 0], r["status"]
    for k in (1, 2):
        assert not r["Sig_inv"][k].any() and not r["coef"][k].any() and not r["Sig_invMcoef"][k].any()
        assert r["loglik"][k] == 0.0 and r["alpha"][k] == 0.0 and r["alpha_info"][k] == 0.0
    b, H, _, a, _, _ = nr.fit(X[4000:], y[4000:], o[4000:], True)
    assert rel(r["coef"][3].cpu().numpy(), b) <= 1e-10 and abs(r["alpha"][3] - a) <= 1e-9 * a


def test_collinear_column_is_not_spd(eng):
    X, y, _ = nr.data(60, 2000, 5, True, False, 0.5)
    X = np.column_stack([X, X[:, 0]])                       # duplicated column: singular information
    r = _fit(eng, X, y, None, [0, 2000], False)
    assert r["status"] == [2] and r["rc"] == 4


def test_negative_or_non_finite_counts_are_refused(eng):
    import dlsa_amd
    from dlsa_amd import _lib
    X, y, o = nr.data(61, 1000, 3, True, True, 0.5)
    y_bad = y.copy(); y_bad[700] = -1.0
    with pytest.raises(ValueError):
        dlsa_amd.fit_negbin_partitions(*_dev(X, y_bad), fit_intercept=True)
    with pytest.raises(_lib.DlsaError) as ex:       # (the C ABI's own check, below the Python one)
        _fit(eng, X, y_bad, o, [0, 500, 1000], True)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    o_bad = o.copy(); o_bad[3] = np.nan
    with pytest.raises(_lib.DlsaError) as ex:
        _fit(eng, X, y, o_bad, [0, 500, 1000], True)
    assert "partition 0" in str(ex.value)
    with pytest.raises(ValueError):
        dlsa_amd.fit_negbin_partitions(*_dev(X, y), offset=_dev(o)[0], exposure=_dev(np.exp(o))[0])
    # the pass reports an invalid count as a NaN log-likelihood
    ll = eng.negbin_pass(*_dev(X, y_bad, np.zeros(3)), 0.5)[2]
    assert math.isnan(float(ll.item()))
    with pytest.raises(ValueError):
        eng.negbin_pass(*_dev(X, y, np.zeros(3)), 0.0)


def test_fit_is_bit_reproducible(eng):
    import dlsa_amd
    X, y, o = nr.data(80, 50_000, 30, True, True, 0.5)
    Xd, yd, od = _dev(X, y, o)
    a = dlsa_amd.fit_negbin_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    b = dlsa_amd.fit_negbin_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    assert a.status == [0] * 3
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik and a.extra == b.extra and a.n_iter == b.n_iter


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K = 80_000, 10, 8
    X, y, o = nr.data(90, n, p, True, True, 0.5)
    Xd, yd, od = _dev(X, y, o)
    mb = dlsa_amd.fit_negbin_partitions(Xd, yd, partition_num=K, fit_intercept=True, offset=od)
    assert mb.status == [0] * K and min(mb.extra["alpha"]) > 0
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [nr.block(X[k::K], y[k::K], o[k::K], True) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = dlsa_amd.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


def test_sig_inv_is_calibrated(eng):
    """the reason for the feature: on overdispersed counts the NB block's Sig_inv is the information the data carry, the Poisson one
    is too large by about 1 + alpha mu"""
    import dlsa_amd
    df = dlsa_amd.simulate_negbin(2_000_000, 10, 20, alpha=0.5)
    assert list(df.columns) == ["partition_id", "y"] + ["x%d" % i for i in range(10)]
    X = torch.from_numpy(np.ascontiguousarray(df.iloc[:, 2:].to_numpy())).cuda()
    y = torch.from_numpy(df["y"].to_numpy()).cuda()
    mb = dlsa_amd.fit_negbin_partitions(X, y, partition_num=20, fit_intercept=True)
    assert mb.status == [0] * 20
    theta = dlsa_amd.dlsa_mapred(mb)["beta_byOLS"].to_numpy()
    one = dlsa_amd.fit_negbin_partitions(X, y, fit_intercept=True)
    assert one.status == [0]
    Hn = one.Sig_inv[0].cpu().numpy()
    se = np.sqrt(np.diag(np.linalg.inv(Hn)))
    gap = np.abs(theta - one.coef[0].cpu().numpy()) / se
    assert gap.max() <= 0.1, gap
    truth = np.concatenate([[0.0], np.where(np.arange(10) < 4, 0.5, 0.0)])
    assert np.all(np.abs(one.coef[0].cpu().numpy() - truth) <= 5 * se)
    a, info = one.extra["alpha"][0], one.extra["alpha_info"][0]
    assert abs(math.log(a) - math.log(0.5)) <= 5 / math.sqrt(info), (a, info)
    ac = dlsa_amd.combine_dispersion(mb)
    assert abs(math.log(ac) - math.log(a)) <= 1 / math.sqrt(info)      # the one-round combine of the 20 estimates: within one standard error
    pois = dlsa_amd.fit_poisson_partitions(X, y, fit_intercept=True)
    ratio = np.diag(pois.Sig_inv[0].cpu().numpy()) / np.diag(Hn)
    assert ratio.min() > 1.2, ratio


def test_negbin_model_frame_and_eval(eng):
    import pandas as pd
    import dlsa_amd
    df = dlsa_amd.simulate_negbin(5000, 6, 1, 0.5, seed=7, exposure=True)
    assert list(df.columns) == ["partition_id", "y", "exposure"] + ["x%d" % i for i in range(6)]
    part = df.drop(columns=["partition_id"])
    out = dlsa_amd.negbin_model(part, "y", fit_intercept=True, exposure_name="exposure")
    names = ["intercept"] + ["x%d" % i for i in range(6)]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (7, 10)
    X = part[names[1:]].to_numpy()
    Xd, yd, ed = _dev(X, part["y"].to_numpy(), part["exposure"].to_numpy())
    mb = dlsa_amd.fit_negbin_partitions(Xd, yd, fit_intercept=True, exposure=ed)
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out["Sig_invMcoef"].to_numpy(), mb.Sig_invMcoef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    ahat = out.attrs["alpha"]
    assert ahat == mb.extra["alpha"][0] == dlsa_amd.combine_dispersion(mb) and ahat > 0
    o = np.log(part["exposure"].to_numpy())
    b, H, ll, a, _, _ = nr.fit(X, part["y"].to_numpy(), o, True)
    assert rel(out["coef"].to_numpy(), b) <= 1e-10 and abs(ahat - a) <= 1e-9 * a
    # a second map step at the combined dispersion
    fixed = dlsa_amd.negbin_model(part, "y", fit_intercept=True, exposure_name="exposure", alpha=ahat)
    assert fixed.attrs["alpha"] == ahat and rel(fixed["coef"].to_numpy(), b) <= 1e-9
    # eval: the log-likelihood of each estimator column, shaped like poisson_model_eval
    par = pd.DataFrame({"mle": mb.coef[0].cpu().numpy(), "ref": b, "zero": np.zeros(7)})
    ev = dlsa_amd.negbin_model_eval(part, "y", par, ahat, fit_intercept=True, exposure_name="exposure")
    assert list(ev.columns) == ["mle", "ref", "zero"] and ev.shape == (1, 3)
    od = torch.log(ed)
    for c in par.columns:              # the tensor path: one pass per estimator column
        ll_c = eng.negbin_pass(Xd, yd, _dev(par[c].to_numpy())[0], ahat, offset=od, fit_intercept=True, want_H=False)[2]
        assert ev[c][0] == float(ll_c.item())
    assert abs(ev["mle"][0] - mb.loglik[0]) <= 1e-12 * abs(mb.loglik[0])
    refs = [nr.terms(X, part["y"].to_numpy(), par[c].to_numpy(), ahat, o, True)[0] for c in par.columns]
    assert rel(ev.to_numpy()[0], refs) <= 1e-12


def test_negbin_model_missing_dummy_level_gives_zero_block(eng):
    import pandas as pd
    import dlsa_amd
    rng = np.random.default_rng(2)
    n = 4000
    df = pd.DataFrame({"partition_id": np.zeros(n), "y": 0.0, "dist": rng.normal(5.0, 2.0, n),
                       "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2])})
    mu = np.exp(0.1 * (df["dist"] - 5) + 0.4 * (df["carrier"] == "BB"))
    df["y"] = rng.poisson(mu * rng.gamma(2.0, 0.5, n)).astype(float)
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"]}, "factor_dropped": {"carrier": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"]}}
    baseline = ["carrier_AA"]
    want = ["par_id", "coef", "Sig_invMcoef", "intercept", "dist", "carrier_BB", "carrier_CC"]
    out = dlsa_amd.negbin_model(df, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert list(out.columns) == want
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC"]).astype(float)
    b, H, _, a, _, _ = nr.fit(Xo, df["y"].to_numpy(), None, True)
    assert rel(out["coef"], b) <= 1e-10 and rel(out.iloc[:, 3:].to_numpy(), H) <= 1e-10 and abs(out.attrs["alpha"] - a) <= 1e-9 * a
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = dlsa_amd.negbin_model(sub, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert any("missing in this data chunk" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (4, 7) and float(np.abs(zero.to_numpy()).max()) == 0.0


def test_full_size_fit(eng):
    import dlsa_amd
    n, p, alpha = 10_000_000, 100, 0.5
    X, _ = eng.synth(123, 0, n, p, labels=False)
    beta = torch.zeros(p + 1, dtype=torch.float64, device="cuda")
    beta[0] = 0.2
    beta[1: 1 + int(0.4 * p)] = 0.5
    g = torch.Generator(device="cuda").manual_seed(5)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    # Gamma(shape 1 / alpha = 2, scale alpha): the sum of two exponentials, drawn on the device
    u = torch.rand((2, n), dtype=torch.float64, device="cuda", generator=g).clamp_min_(1e-300)
    mix = -alpha * (torch.log(u[0]) + torch.log(u[1]))
    y = torch.poisson(torch.exp(X @ beta[1:] + beta[0] + o) * mix, generator=g)
    del u, mix
    mb = dlsa_amd.fit_negbin_partitions(X, y, fit_intercept=True, offset=o)
    assert mb.status == [0]
    coef, ahat = mb.coef[0], mb.extra["alpha"][0]
    print("negbin full size: alpha_hat %.6f, %d row passes" % (ahat, mb.n_iter[0]))
    H, gs, ll, _, _, tt = eng.negbin_pass(X, y, coef, ahat, offset=o, fit_intercept=True, want_theta=True)
    assert float(gs.abs().max()) <= 1e-9 * float(y.sum())             # the score vanishes at the returned coef
    s, i, _ = tt.cpu().numpy()
    assert abs(s * ahat / i) <= 1e-9                                   # and so does the dispersion's
    Hn = H.cpu().numpy()
    assert np.array_equal(Hn, Hn.T) and np.all(np.linalg.eigvalsh(Hn) > 0)
    assert rel(Hn, mb.Sig_inv[0].cpu().numpy()) <= 1e-12
    assert abs(float(ll.item()) - mb.loglik[0]) <= 1e-12 * abs(mb.loglik[0])
    se = np.sqrt(np.diag(np.linalg.inv(Hn)))
    z = np.abs(coef.cpu().numpy() - beta.cpu().numpy()) / se
    assert z.max() <= 5.0, z.max()
    assert abs(math.log(ahat) - math.log(alpha)) <= 5 / math.sqrt(mb.extra["alpha_info"][0])
    # a 2e5-row slice against the reference
    m = 200_000
    _check_pass(eng, X[:m].cpu().numpy(), y[:m].cpu().numpy(), o[:m].cpu().numpy(), coef.cpu().numpy(), ahat, True, theta=False)
