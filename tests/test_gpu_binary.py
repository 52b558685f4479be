"""GPU: the probit and cloglog map steps (csrc/binary.hip) against the CPU Newton fit of tests/binary_reference.py (row terms from
mpmath, sums in longdouble, iterated to a step below 1e-15): the per-partition fit on contiguous and strided partitions, the cloglog
pass on y = 0 against the Poisson pass bit for bit, the degenerate and refused partitions, the frame-level models and the end-to-end
DLSA combine.  The tolerances are those test_gpu_poisson.py holds against poisson_reference.py."""
import functools
import math

import numpy as np
import pytest

import binary_reference as br

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K = 4000, 4


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


def _prob(link, eta):
    return -np.expm1(-np.exp(eta)) if link == "cloglog" else 0.5 * (1.0 + np.vectorize(math.erf)(eta / math.sqrt(2.0)))


@functools.lru_cache(maxsize=None)
def _data(link, seed, n, p, intercept, offset, b0=-0.3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.where(np.arange(p) < max(1, int(0.4 * p)), 1.0, 0.0) / max(1.0, math.sqrt(p / 10))
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    eta = X @ beta + (b0 if intercept else 0.0) + (0.0 if o is None else o)
    y = (rng.uniform(size=n) < _prob(link, eta)).astype(np.float64)
    return X, y, o


@functools.lru_cache(maxsize=None)
def _reference(link, p, intercept, offset):
    """the reference blocks of the K contiguous partitions, computed once"""
    X, y, o = _data(link, 40 + p, N, p, intercept, offset)
    offs = [k * N // K for k in range(K + 1)]
    return [br.newton_fit(link, X[offs[k]:offs[k + 1]], y[offs[k]:offs[k + 1]], None if o is None else o[offs[k]:offs[k + 1]], intercept)
            for k in range(K)]


def _fit_ex(eng, link):
    return eng.probit_fit_ex if link == "probit" else eng.cloglog_fit_ex


def _pass(eng, link):
    return eng.probit_pass if link == "probit" else eng.cloglog_pass


def _fit_partitions(link):
    import dlsa_amd
    return dlsa_amd.fit_probit_partitions if link == "probit" else dlsa_amd.fit_cloglog_partitions


def _away_from_optimum(pe):
    return np.linspace(-0.8, 0.6, pe) / max(1.0, math.sqrt(pe / 10))


def _check_pass(eng, link, X, y, o, beta, intercept, tol=1e-12):
    """the pass on dense rows against model_terms at the same eta, summed in longdouble (the bar of test_gpu_poisson.py's pass check)"""
    Xd, yd, od, bd = _dev(X, y, o, beta)
    H, g, ll, w = _pass(eng, link)(Xd, yd, bd, offset=od, fit_intercept=intercept, want_w=True)
    D = (np.concatenate([np.ones((len(y), 1)), X], 1) if intercept else X).astype(np.longdouble)
    eta = (D @ beta.astype(np.longdouble) + (0 if o is None else o.astype(np.longdouble))).astype(np.float64)
    t = {key: np.where(y == 1, br.model_terms(link, eta, 1)[key], br.model_terms(link, eta, 0)[key]).astype(np.longdouble) for key in br.KEYS}
    llr, gr, Hr = float(np.sum(t["l"])), (D.T @ t["r"]).astype(np.float64), (D.T @ (D * t["w"][:, None])).astype(np.float64)
    figs = (abs(float(ll.item()) - llr) / abs(llr), rel(g.cpu().numpy(), gr), rel(w.cpu().numpy(), t["w"].astype(np.float64)), rel(H.cpu().numpy(), Hr))
    assert max(figs) <= tol, figs
    Hn = H.cpu().numpy()
    assert np.array_equal(Hn, Hn.T)
    return figs


@pytest.mark.parametrize("p", [1, 7, 130, 260, 600, 1030])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
@pytest.mark.parametrize("link", br.LINKS)
def test_pass_matches_reference(eng, link, p, intercept, offset):
    """dense rows at every column-chunk count of the row pass (NC = 1, 2, 4, 8, 16), n not a multiple of the batch"""
    X, y, o = _data(link, 10 + p, 1003, p, intercept, offset)
    figs = _check_pass(eng, link, X, y, o, _away_from_optimum(p + intercept), intercept)
    print("%s pass p=%d: ll %.1e g %.1e w %.1e H %.1e" % ((link, p) + figs))


@pytest.mark.parametrize("p", [1, 5, 129])
@pytest.mark.parametrize("intercept,offset", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("link", br.LINKS)
def test_fit_matches_reference(eng, link, p, intercept, offset):
    X, y, o = _data(link, 40 + p, N, p, intercept, offset)
    offs = [k * N // K for k in range(K + 1)]
    Xd, yd, od = _dev(X, y, o)
    r = _fit_ex(eng, link)(Xd, yd, offs[:-1], [offs[k + 1] - offs[k] for k in range(K)], offset=od, fit_intercept=intercept)
    assert r["status"] == [0] * K and r["rc"] == 0, r["status"]
    ref = _reference(link, p, intercept, offset)
    worst = 0.0
    for k in range(K):
        b, H, Hb, ll = ref[k]
        figs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H), rel(r["Sig_invMcoef"][k].cpu().numpy(), Hb),
                abs(r["loglik"][k] - ll) / abs(ll))
        worst = max(worst, *figs)
        assert max(figs) <= 1e-10, (k, figs)
    print("%s p=%d intercept=%r offset=%r: worst relative error %.2e" % (link, p, intercept, offset, worst))
    # the same partitions as strided views of the interleaved rows
    perm = np.empty(N, dtype=np.int64)
    for k in range(K):
        perm[k::K] = np.arange(offs[k], offs[k + 1])
    Xs, ys, os_ = _dev(X[perm], y[perm], None if o is None else o[perm])
    s = _fit_ex(eng, link)(Xs, ys, list(range(K)), [N // K] * K, row_step=K, offset=os_, fit_intercept=intercept)
    assert s["status"] == [0] * K
    for name in ("coef", "Sig_inv", "Sig_invMcoef"):
        assert rel(s[name].cpu().numpy(), r[name].cpu().numpy()) <= 1e-13, name
    assert rel(s["loglik"], r["loglik"]) <= 1e-13


@pytest.mark.parametrize("seed", [700, 701, 702])
@pytest.mark.parametrize("link,b0", [("probit", -2.95), ("cloglog", -6.4)])
def test_fit_of_rare_events(eng, link, b0, seed):
    """a response share of 1e-3 to 3e-3 -- 5 to 12 ones among 4000 rows -- with p + 1 = 21 coefficients, more than there are ones: the
    start value of the intercept has to be the link of that share (from a start in the far tail every row of the majority has w = 0 and
    H has the rank of the ones).  The fit reaches the reference's MLE in at most two evaluations more than the reference's start needs."""
    n, p = 4000, 20
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.zeros(p)
    beta[:3] = 0.6
    y = (rng.uniform(size=n) < _prob(link, X @ beta + b0)).astype(np.float64)
    ones = int(y.sum())
    assert 1 <= ones < p + 1
    r = _fit_ex(eng, link)(*_dev(X, y), [0], [n], fit_intercept=True)
    assert r["status"] == [0] and r["rc"] == 0, r["status"]
    b, H, Hb, ll = br.newton_fit(link, X, y, None, True)
    figs = (rel(r["coef"][0].cpu().numpy(), b), rel(r["Sig_inv"][0].cpu().numpy(), H), rel(r["Sig_invMcoef"][0].cpu().numpy(), Hb),
            abs(r["loglik"][0] - ll) / abs(ll))
    print("%s rare events: %d ones of %d, %d evaluations, worst relative error %.2e" % (link, ones, n, r["n_iter"][0], max(figs)))
    assert max(figs) <= 1e-10, figs
    assert r["n_iter"][0] <= 12, r["n_iter"]


@pytest.mark.parametrize("p", [3, 4, 130])
@pytest.mark.parametrize("intercept", [False, True])
def test_cloglog_pass_on_zeros_is_the_poisson_pass_bit_for_bit(eng, p, intercept):
    X, _, o = _data("cloglog", 7, 1003, p, intercept, True)
    beta = np.linspace(-0.8, 0.6, p + intercept)
    Xd, od, bd = _dev(X, o, beta)
    yd = torch.zeros(1003, dtype=torch.float64, device="cuda")
    a = eng.cloglog_pass(Xd, yd, bd, offset=od, fit_intercept=intercept, want_w=True)
    b = eng.poisson_pass(Xd, yd, bd, offset=od, fit_intercept=intercept, want_w=True)
    for u, v, what in zip(a, b, ("H", "g", "loglik", "w")):
        assert torch.equal(u, v), what


@pytest.mark.parametrize("link", br.LINKS)
def test_degenerate_and_empty_partitions(eng, link):
    """with an intercept, all-0 and all-1 partitions and a partition without rows are EMPTY with the zero block; without an intercept
    an all-equal response can have a finite MLE, and the loop runs"""
    n, p = 4000, 3
    X, y, o = _data(link, 50, n, p, True, True)
    y = y.copy()
    y[1000:2000] = 0.0
    y[2000:3000] = 1.0
    first, rows = [0, 1000, 2000, 3000, 3000], [1000, 1000, 1000, 0, 1000]
    Xd, yd, od = _dev(X, y, o)
    r = _fit_ex(eng, link)(Xd, yd, first, rows, offset=od, fit_intercept=True)
    assert r["status"] == [0, 4, 4, 4, 0], r["status"]
    for k in (1, 2, 3):
        assert not r["Sig_inv"][k].any() and not r["coef"][k].any() and not r["Sig_invMcoef"][k].any() and r["loglik"][k] == 0.0
    b, H, _, _ = br.newton_fit(link, X[3000:], y[3000:], o[3000:], True)
    assert rel(r["coef"][4].cpu().numpy(), b) <= 1e-10 and rel(r["Sig_inv"][4].cpu().numpy(), H) <= 1e-10
    # a finite MLE without an intercept: the responses all 1, one column of both signs: l = sum log F(x b) has its maximum where the
    # score sum r x = 0 balances the two signs
    x = np.concatenate([np.full(600, 1.0), np.full(400, -1.0)])[:, None]
    ones = np.ones(1000)
    r1 = _fit_ex(eng, link)(*_dev(x, ones), [0], [1000], fit_intercept=False)
    b1, H1, _, ll1 = br.newton_fit(link, x, ones, None, False)
    assert r1["status"] == [0] and rel(r1["coef"][0].cpu().numpy(), b1) <= 1e-10 and abs(r1["loglik"][0] - ll1) <= 1e-10 * abs(ll1)


@pytest.mark.parametrize("link", br.LINKS)
def test_invalid_responses_and_offsets_are_refused(eng, link):
    from dlsa_amd import _lib
    X, y, o = _data(link, 61, 1000, 3, True, True)
    fit = _fit_partitions(link)
    for bad in (2.0, 0.5, math.nan, -1.0):
        y_bad = y.copy(); y_bad[700] = bad
        with pytest.raises(ValueError, match="the response must be 0 or 1"):
            fit(*_dev(X, y_bad), fit_intercept=True)
        with pytest.raises(_lib.DlsaError) as ex:          # (the C ABI's own check, below the Python one)
            _fit_ex(eng, link)(*_dev(X, y_bad), [0, 500], [500, 500], offset=_dev(o)[0], fit_intercept=True)
        assert ex.value.code == 1 and "partition 1" in str(ex.value) and "not 0 or 1" in str(ex.value)
        _, _, ll, _ = _pass(eng, link)(*_dev(X, y_bad, np.zeros(3)))
        assert math.isnan(float(ll.item()))
    o_bad = o.copy(); o_bad[3] = math.inf
    with pytest.raises(_lib.DlsaError) as ex:
        _fit_ex(eng, link)(*_dev(X, y), [0, 500], [500, 500], offset=_dev(o_bad)[0], fit_intercept=True)
    assert ex.value.code == 1 and "partition 0" in str(ex.value)
    with pytest.raises(ValueError, match="not both"):
        fit(*_dev(X, y), offset=_dev(o)[0], exposure=_dev(np.exp(o))[0])
    with pytest.raises(ValueError):
        fit(*_dev(X, y[:-1]))
    with pytest.raises(ValueError):
        fit(*_dev(X, y), offset=_dev(o[:-1])[0])
    _, _, ll, _ = _pass(eng, link)(*_dev(X, y, np.zeros(3)))
    assert math.isfinite(float(ll.item()))


def test_collinear_column_is_not_spd(eng):
    X, y, _ = _data("probit", 60, 2000, 5, True, False)
    X = np.column_stack([X, X[:, 0]])
    r = eng.probit_fit_ex(*_dev(X, y), [0], [2000])
    assert r["status"] == [2] and r["rc"] == 4


@pytest.mark.parametrize("link", br.LINKS)
def test_model_frame_and_eval(eng, link):
    """<link>_model on a frame with a dummy factor and an exposure column against fit_<link>_partitions on the design it builds;
    <link>_model_eval at the fitted coefficients returns the fit's loglik"""
    import pandas as pd
    import dlsa_amd
    rng = np.random.default_rng(3)
    n = 4000
    df = pd.DataFrame({"y": 0.0, "exposure": rng.uniform(0.5, 2.0, n), "dist": rng.normal(0.0, 1.0, n),
                       "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2])})
    eta = -0.4 + 0.5 * df["dist"].to_numpy() + 0.4 * (df["carrier"] == "BB").to_numpy() - 0.3 * (df["carrier"] == "CC").to_numpy() \
        + np.log(df["exposure"].to_numpy())
    df["y"] = (rng.uniform(size=n) < _prob(link, eta)).astype(float)
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"]}, "factor_dropped": {"carrier": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"]}}
    baseline = ["carrier_AA"]
    model = dlsa_amd.probit_model if link == "probit" else dlsa_amd.cloglog_model
    model_eval = dlsa_amd.probit_model_eval if link == "probit" else dlsa_amd.cloglog_model_eval
    names = ["intercept", "dist", "carrier_BB", "carrier_CC"]
    out = model(df, "y", fit_intercept=True, exposure_name="exposure", dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (4, 7)
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC"]).astype(float)
    Xd, yd, ed = _dev(Xo, df["y"].to_numpy(), df["exposure"].to_numpy())
    mb = _fit_partitions(link)(Xd, yd, fit_intercept=True, exposure=ed)
    assert mb.status == [0]
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out["Sig_invMcoef"].to_numpy(), mb.Sig_invMcoef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    b, H, _, ll = br.newton_fit(link, Xo, df["y"].to_numpy(), np.log(df["exposure"].to_numpy()), True)
    assert rel(out["coef"].to_numpy(), b) <= 1e-10 and rel(out[names].to_numpy(), H) <= 1e-10
    par = pd.DataFrame({"mle": mb.coef[0].cpu().numpy(), "zero": np.zeros(4)})
    ev = model_eval(df, "y", par, fit_intercept=True, exposure_name="exposure", dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert list(ev.columns) == ["mle", "zero"] and ev.shape == (1, 2)
    assert abs(ev["mle"][0] - mb.loglik[0]) <= 1e-13 * abs(mb.loglik[0])
    assert abs(ev["mle"][0] - ll) <= 1e-10 * abs(ll) and ev["zero"][0] < ev["mle"][0]
    # an offset column instead of the exposure column: the same model
    df2 = df.assign(logexp=np.log(df["exposure"])).drop(columns=["exposure"])
    out2 = model(df2, "y", fit_intercept=True, offset_name="logexp", dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert rel(out2["coef"].to_numpy(), out["coef"].to_numpy()) <= 1e-12


@pytest.mark.parametrize("link", br.LINKS)
def test_end_to_end_dlsa_recovers_the_simulated_coefficients(eng, link):
    """simulate_binary (fixed seed), K = 8: dlsa_mapred's WLS estimate within 5 standard errors (from the combined Sig_inv) of the
    simulated coefficients, and dlsa's path with unpenalized="intercepts" keeps the intercept"""
    import dlsa_amd
    n, p, Kp = 40_000, 10, 8
    df = dlsa_amd.simulate_binary(n, p, Kp, link, seed=20260101, intercept=-0.5, coef_value=0.5, exposure=True)
    assert list(df.columns) == ["partition_id", "y", "exposure"] + ["x%d" % i for i in range(p)]
    assert set(np.unique(df["y"])) == {0.0, 1.0}
    X = torch.from_numpy(np.ascontiguousarray(df.iloc[:, 3:].to_numpy())).cuda()
    y = torch.from_numpy(df["y"].to_numpy()).cuda()
    e = torch.from_numpy(df["exposure"].to_numpy()).cuda()
    mb = _fit_partitions(link)(X, y, partition_num=Kp, fit_intercept=True, exposure=e)
    assert mb.status == [0] * Kp
    out = dlsa_amd.dlsa_mapred(mb)
    theta = out["beta_byOLS"].to_numpy()
    S = out.iloc[:, 2:].to_numpy()
    se = np.sqrt(np.diag(np.linalg.inv(S)))
    truth = np.concatenate([[-0.5], np.where(np.arange(p) < int(0.4 * p), 0.5, 0.0)])
    gap = np.abs(theta - truth) / se
    print("%s: |theta - truth| / se = %s" % (link, np.round(gap, 2)))
    assert np.all(gap <= 5.0), gap
    # the combine reproduces its own blocks: Sig_inv is the sum of the partitions'
    assert rel(S, mb.Sig_inv.sum(0).cpu().numpy()) <= 1e-12
    res = dlsa_amd.dlsa(out.iloc[:, 2:], out["beta_byOLS"], n, unpenalized="intercepts")
    assert list(res.columns) == ["beta_byAIC", "beta_byBIC"] and res.shape == (p + 1, 2)
    bic = res["beta_byBIC"].to_numpy()
    assert bic[0] != 0.0 and abs(bic[0] - theta[0]) <= 5 * se[0]
    assert np.all(bic[1:1 + int(0.4 * p)] != 0.0)
    with pytest.raises(ValueError):
        dlsa_amd.simulate_binary(10, 2, 1, "logit")
