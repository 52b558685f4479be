"""GPU: the Gamma regression map step (csrc/gamma.hip) against the numpy reference (tests/gamma_reference.py): the pass at a fixed
beta and dispersion (loglik, score, r, information, Pearson and deviance sums) at every class the count pass and the Gram dispatch
distinguish, the per-partition fit with estimated and fixed dispersion, strided partitions, reproducibility, edge cases, the
calibration of the block that the dispersion is there for, the end-to-end DLSA combine and the frame-level gamma_model.

The tolerances are the project's parity bars of the Poisson tests (1e-12 for a pass, 1e-10 for a fit): on the CPU the fp64 numpy
reference agrees with a longdouble run of itself to <= 6e-16 on coef and H at the widths used here."""
import math
import warnings

import numpy as np
import pytest

import gamma_reference as gr
import newton_reference as nw

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


def _data(seed, n, p, intercept, offset, b0=0.3, shape=2.0):
    """X ~ U(-0.5, 0.5), beta* as test_gpu_poisson._data, y ~ Gamma(shape, mu / shape), offsets log U(0.5, 2)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.where(np.arange(p) < max(1, int(0.4 * p)), 0.5, 0.0) / max(1.0, math.sqrt(p / 10))
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    eta = X @ beta + (b0 if intercept else 0.0) + (0.0 if o is None else o)
    y = rng.gamma(shape, np.exp(eta) / shape)
    return X, y, o


def _check_pass(eng, X, y, o, beta, intercept, dispersion=1.0, tol=1e-12, Xd=None):
    """Xd: the device tensor to pass for X (a view with its own pitch / alignment); default a contiguous copy"""
    Xc, yd, od, bd = _dev(X, y, o, beta)
    H, g, ll, w, st = eng.gamma_pass(Xc if Xd is None else Xd, yd, bd, dispersion, offset=od, fit_intercept=intercept, want_w=True,
                                     want_stats=True)
    llr, gr_, Hr, rr, Pr, devr = gr.terms(X, y, beta, o, intercept, dispersion)
    Hn, P, dev = H.cpu().numpy(), float(st[0].item()), float(st[1].item())
    errs = {"ll": abs(float(ll.item()) - llr) / abs(llr), "g": rel(g.cpu().numpy(), gr_), "w": rel(w.cpu().numpy(), rr), "H": rel(Hn, Hr),
            "P": abs(P - Pr) / Pr, "Dev": abs(dev - devr) / devr}
    print("gamma pass n=%d p=%d: %s" % (X.shape[0], X.shape[1], " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= tol for v in errs.values()), errs
    assert np.array_equal(Hn, Hn.T)


def _away_from_optimum(pe):
    return np.linspace(-0.8, 0.6, pe) / max(1.0, math.sqrt(pe / 10))


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("dispersion", [1.0, 0.37])
def test_pass_matches_reference(eng, p, intercept, offset, dispersion):
    n = 3 * p + 37
    X, y, o = _data(10 + p, n, p, intercept, offset)
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), intercept, dispersion)


# fewer rows than one batch of 8 (or a single row): at NC = 1 every prefetch of the second register set is a clamped re-read of row
# n - 1; p = 1030 is NC = 16 with one row per wave
@pytest.mark.parametrize("n", [1, 5, 9])
@pytest.mark.parametrize("p", [3, 130, 1030])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_short_and_wide_shapes(eng, n, p, intercept, offset):
    X, y, o = _data(900 + p + n, n, p, intercept, offset)
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), intercept, 0.37)


@pytest.mark.parametrize("p", [8, 130, 1030])
@pytest.mark.parametrize("pad", [3, 2])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_even_width_on_the_scalar_loads(eng, p, pad, intercept, offset):
    """an even p takes the scalar loads only through the rows' pitch or base: columns 1 .. p of a buffer with p + 3 columns (an odd
    pitch) and of one with p + 2 (an even pitch, the base 8 bytes off a 16-byte boundary), passed as views, without a copy"""
    n = 67
    X, y, o = _data(900 + p + n, n, p, intercept, offset)
    big = torch.zeros((n, p + pad), dtype=torch.float64, device="cuda")
    Xd = big[:, 1:1 + p]
    Xd.copy_(torch.from_numpy(X))
    assert Xd.stride(0) == p + pad and Xd.stride(1) == 1
    if pad == 2:
        assert Xd.data_ptr() % 16 == 8
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), intercept, Xd=Xd)


def test_pass_eta_spanning_600(eng):
    n, p = 2000, 3
    X, y, o = _data(20, n, p, True, True)
    X[:, 0] = np.linspace(-1.0, 1.0, n)
    beta = np.array([-0.4, 300.0, 0.3, -0.2])
    ll, g, H, r, P, dev = gr.terms(X, y, beta, o, True)
    assert np.ptp(np.log(r)) > 590 and all(np.isfinite(v).all() for v in (ll, g, H, r, P, dev))
    _check_pass(eng, X, y, o, beta, True)


def _fit(eng, X, y, o, offs, intercept, **kw):
    Xd, yd, od = _dev(X, y, o)
    return eng.gamma_fit_ex(Xd, yd, offs[:-1], [offs[k + 1] - offs[k] for k in range(len(offs) - 1)], offset=od,
                            fit_intercept=intercept, **kw)


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("intercept,offset", [(True, True), (False, False)])
def test_fit_matches_reference(eng, p, intercept, offset):
    n, K = max(2000, 10 * p), 3
    X, y, o = _data(40 + p, n, p, intercept, offset)
    offs = [0, int(0.30 * n), int(0.62 * n), n]                 # unequal sizes
    est = _fit(eng, X, y, o, offs, intercept)
    fix = _fit(eng, X, y, o, offs, intercept, dispersion=0.5)
    assert est["status"] == [0] * K and fix["status"] == [0] * K, (est["status"], fix["status"])
    assert est["df"] == [offs[k + 1] - offs[k] - p - intercept for k in range(K)]
    worst = {}
    for k in range(K):
        sl = slice(offs[k], offs[k + 1])
        ok = None if o is None else o[sl]
        b, S, ll, phi, P, dev = gr.fit(X[sl], y[sl], ok, intercept)
        _, S5, ll5, _, _, _ = gr.fit(X[sl], y[sl], ok, intercept, dispersion=0.5)
        for r, Sr, llr, phir in ((est, S, ll, phi), (fix, S5, ll5, 0.5)):
            errs = {"coef": rel(r["coef"][k].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][k].cpu().numpy(), Sr),
                    "Sig_invMcoef": rel(r["Sig_invMcoef"][k].cpu().numpy(), Sr @ b), "ll": abs(r["loglik"][k] - llr) / abs(llr),
                    "phi": abs(r["dispersion"][k] - phir) / phir, "P": abs(r["pearson"][k] - P) / P, "Dev": abs(r["deviance"][k] - dev) / dev}
            worst = {key: max(v, worst.get(key, 0.0)) for key, v in errs.items()}
        assert fix["dispersion"][k] == 0.5
        # the dispersion is one scalar on the information: the block at 0.5 is twice the unit block
        unit = _fit(eng, X[sl], y[sl], ok, [0, offs[k + 1] - offs[k]], intercept, dispersion=1.0)
        assert rel(fix["Sig_inv"][k].cpu().numpy(), 2.0 * unit["Sig_inv"][0].cpu().numpy()) <= 1e-13
    print("gamma fit p=%d (%d evaluations): %s" % (p, max(est["n_iter"]), " ".join("%s %.1e" % kv for kv in worst.items())))
    assert all(v <= 1e-10 for v in worst.values()), worst


def test_strided_partitions_equal_contiguous_copies(eng):
    import dlsa_amd
    n, p, K = 3001, 8, 5
    X, y, o = _data(70, n, p, True, True)
    e = np.exp(o)
    Xd, yd, ed = _dev(X, y, e)
    a = dlsa_amd.fit_gamma_partitions(Xd, yd, partition_num=K, fit_intercept=True, exposure=ed)
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    Xc, yc, ec = _dev(X[perm], y[perm], e[perm])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    b = dlsa_amd.fit_gamma_partitions(Xc, yc, part_offsets=offs, fit_intercept=True, exposure=ec)
    assert a.status == [0] * K and b.status == [0] * K
    assert a.names == ["intercept"] + ["x%d" % i for i in range(p)]
    assert rel(a.coef.cpu().numpy(), b.coef.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_inv.cpu().numpy(), b.Sig_inv.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_invMcoef.cpu().numpy(), b.Sig_invMcoef.cpu().numpy()) <= 1e-13
    assert rel(a.extra["dispersion"], b.extra["dispersion"]) <= 1e-13 and a.extra["df"] == b.extra["df"]


def test_fit_is_bit_reproducible(eng):
    import dlsa_amd
    X, y, o = _data(80, 20_000, 30, True, True)
    Xd, yd, od = _dev(X, y, o)
    a = dlsa_amd.fit_gamma_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    b = dlsa_amd.fit_gamma_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik and a.extra == b.extra and all(v > 0 for v in a.extra["dispersion"])


def test_fit_empty_partition(eng):
    n, p = 3000, 4
    X, y, o = _data(50, n, p, True, True)
    offs = [0, 1000, 1000, n]
    r = _fit(eng, X, y, o, offs, True)
    assert r["status"] == [0, 4, 0] and r["rc"] == 0
    assert not r["Sig_inv"][1].any() and not r["coef"][1].any() and not r["Sig_invMcoef"][1].any()
    assert r["loglik"][1] == 0.0 and r["dispersion"][1] == 0.0 and r["pearson"][1] == 0.0 and r["deviance"][1] == 0.0
    b, S = gr.fit(X[1000:], y[1000:], o[1000:], True)[:2]
    assert rel(r["coef"][2].cpu().numpy(), b) <= 1e-10 and rel(r["Sig_inv"][2].cpu().numpy(), S) <= 1e-10


def test_partition_without_degrees_of_freedom(eng):
    from dlsa_amd import _lib
    n, p = 1000, 3
    X, y, o = _data(51, n, p, True, True)
    for rows1 in (4, 2):                                     # n = pe and n < pe
        offs = [0, 500, 500 + rows1, n]
        with pytest.raises(_lib.DlsaError) as ex:            # estimated dispersion: P / (n - pe) has no degrees of freedom
            _fit(eng, X, y, o, offs, True)
        assert ex.value.code == 1 and "partition 1" in str(ex.value) and "degrees of freedom" in str(ex.value)
    # fixed dispersion, n = pe: the four rows are fitted exactly (r = 1: D beta = log y - o)
    offs = [0, 500, 504, n]
    r = _fit(eng, X, y, o, offs, True, dispersion=0.5)
    assert r["status"] == [0, 0, 0] and r["df"][1] == 0
    sl = slice(500, 504)
    exact = np.linalg.solve(gr.design(X[sl], True), np.log(y[sl]) - o[sl])
    assert rel(r["coef"][1].cpu().numpy(), exact) <= 1e-9 and r["pearson"][1] <= 1e-18
    # fixed dispersion, n < pe: the information is singular, as the data say
    r = _fit(eng, X, y, o, [0, 500, 502, n], True, dispersion=0.5)
    print("two rows for four coefficients: status %d" % r["status"][1])
    assert r["status"][0] == 0 and r["status"][2] == 0 and r["status"][1] != 0 and r["rc"] != 0


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_invalid_responses_are_refused(eng, bad):
    import dlsa_amd
    from dlsa_amd import _lib
    X, y, o = _data(61, 1000, 3, True, True)
    y_bad = y.copy(); y_bad[700] = bad
    with pytest.raises(ValueError):
        dlsa_amd.fit_gamma_partitions(*_dev(X, y_bad), fit_intercept=True)
    with pytest.raises(_lib.DlsaError) as ex:       # (the C ABI's own check, below the Python one)
        _fit(eng, X, y_bad, o, [0, 500, 1000], True)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    # the pass reports an invalid response as a NaN log-likelihood
    ll = eng.gamma_pass(*_dev(X, y_bad, np.zeros(3)))[2]
    assert math.isnan(float(ll.item()))


def test_non_finite_offset_is_refused(eng):
    from dlsa_amd import _lib
    X, y, o = _data(61, 1000, 3, True, True)
    for bad in (float("nan"), float("inf"), -float("inf")):
        o_bad = o.copy(); o_bad[3] = bad
        with pytest.raises(_lib.DlsaError) as ex:
            _fit(eng, X, y, o_bad, [0, 500, 1000], True)
        assert ex.value.code == 1 and "partition 0" in str(ex.value)


def test_collinear_column_is_not_spd(eng):
    X, y, _ = _data(60, 2000, 5, True, False)
    X = np.column_stack([X, X[:, 0]])                       # duplicated column: singular information
    r = _fit(eng, X, y, None, [0, 2000], False)
    assert r["status"] == [2] and r["rc"] == 4


@pytest.mark.parametrize("max_iter", [1, 2])
def test_budget_stops_at_the_evaluated_iterate(eng, max_iter):
    n, p = 600, 3
    X, y, o = _data(303, n, p, True, True)
    evals, bs, lls = nw.undamped(lambda b: gr.terms(X, y, b, o, True)[:3], gr.start(X, y, o, True), 1e-13)
    assert evals is not None and evals > max_iter + 1 and nw.monotone(lls[:max_iter + 1])       # no halving in the budget
    r = _fit(eng, X, y, o, [0, n], True, max_iter=max_iter)
    assert r["status"] == [1] and r["rc"] == 5 and r["n_iter"] == [max_iter + 1]
    # max_iter steps were taken; the last evaluation's step was not: coef is where H and the dispersion were evaluated
    coef = r["coef"][0]
    assert rel(coef.cpu().numpy(), bs[max_iter]) <= 1e-10
    _, _, Hr, _, Pr, devr = gr.terms(X, y, bs[max_iter], o, True)
    phi = Pr / (n - p - 1)
    assert abs(r["dispersion"][0] - phi) <= 1e-10 * phi and abs(r["pearson"][0] - Pr) <= 1e-10 * Pr
    assert abs(r["deviance"][0] - devr) <= 1e-10 * devr
    llr = gr.terms(X, y, bs[max_iter], o, True, phi)[0]
    assert abs(r["loglik"][0] - llr) <= 1e-10 * abs(llr)
    Xd, yd, od = _dev(X, y, o)
    H = eng.gamma_pass(Xd, yd, coef, r["dispersion"][0], offset=od, fit_intercept=True)[0].cpu().numpy()
    assert rel(r["Sig_inv"][0].cpu().numpy(), H) <= 1e-12 and rel(H, Hr / phi) <= 1e-10
    assert rel(r["Sig_invMcoef"][0].cpu().numpy(), H @ coef.cpu().numpy()) <= 1e-12


def test_block_is_calibrated(eng):
    """What the dispersion is for.  K = 40 partitions of 2000 rows, 5 features + intercept, shape 4 (phi = 0.25): the sum over the
    partitions of (b_k - b*)' Sig_inv_k (b_k - b*) is chi-square with 240 degrees of freedom, so it lies in 240 +- 5 sqrt(480) =
    [130, 350]; a Sig_inv left unscaled gives about 60, one scaled the wrong way about 960.  The pooled Pearson estimate has standard
    deviation sqrt((2 phi^2 + 6 phi^3) / 80000): 5 of them are 0.0083.  (On the CPU reference four seeds of this design gave 221 - 273
    and 0.2477 - 0.2500.)"""
    import dlsa_amd
    K, m, p, shape = 40, 2000, 5, 4.0
    rng = np.random.default_rng(2026)
    X = rng.uniform(-0.5, 0.5, (K * m, p))
    truth = np.array([0.3, 0.5, -0.5, 0.25, 0.0, -0.25])
    y = rng.gamma(shape, np.exp(truth[0] + X @ truth[1:]) / shape)
    Xd, yd = _dev(X, y)
    mb = dlsa_amd.fit_gamma_partitions(Xd, yd, part_offsets=[k * m for k in range(K + 1)], fit_intercept=True)
    assert mb.status == [0] * K
    d = mb.coef.cpu().numpy() - truth
    S = mb.Sig_inv.cpu().numpy()
    chi2 = float(np.einsum("ki,kij,kj->", d, S, d))
    phi = dlsa_amd.combine_gamma_dispersion(mb)
    print("calibration: chi-square %.1f on 240 degrees of freedom, pooled dispersion %.4f" % (chi2, phi))
    assert 130.0 <= chi2 <= 350.0
    assert abs(phi - 0.25) <= 0.0083


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K = 40_000, 10, 8
    X, y, o = _data(90, n, p, True, True)
    Xd, yd, od = _dev(X, y, o)
    mb = dlsa_amd.fit_gamma_partitions(Xd, yd, partition_num=K, fit_intercept=True, offset=od)
    assert mb.status == [0] * K
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [gr.block(X[k::K], y[k::K], o[k::K], True) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = dlsa_amd.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


def test_gamma_model_frame_and_eval(eng):
    import pandas as pd
    import dlsa_amd
    df = dlsa_amd.simulate_gamma(5000, 6, 1, 2.0, seed=7, exposure=True)
    assert list(df.columns) == ["partition_id", "y", "exposure"] + ["x%d" % i for i in range(6)] and bool((df["y"] > 0).all())
    part = df.drop(columns=["partition_id"])
    out = dlsa_amd.gamma_model(part, "y", fit_intercept=True, exposure_name="exposure")
    names = ["intercept"] + ["x%d" % i for i in range(6)]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (7, 10)
    X = part[names[1:]].to_numpy()
    Xd, yd, ed = _dev(X, part["y"].to_numpy(), part["exposure"].to_numpy())
    mb = dlsa_amd.fit_gamma_partitions(Xd, yd, fit_intercept=True, exposure=ed)
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out["Sig_invMcoef"].to_numpy(), mb.Sig_invMcoef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    phi = out.attrs["dispersion"]
    assert phi == mb.extra["dispersion"][0] and 0.4 < phi < 0.6            # shape 2
    o = np.log(part["exposure"].to_numpy())
    b, S, ll, phir = gr.fit(X, part["y"].to_numpy(), o, True)[:4]
    assert rel(out["coef"].to_numpy(), b) <= 1e-10 and rel(out[names].to_numpy(), S) <= 1e-10 and abs(phi - phir) <= 1e-10 * phir
    # eval: the log-likelihood of each estimator column at the fit's dispersion, shaped like poisson_model_eval
    par = pd.DataFrame({"mle": mb.coef[0].cpu().numpy(), "ref": b, "zero": np.zeros(7)})
    ev = dlsa_amd.gamma_model_eval(part, "y", par, phi, fit_intercept=True, exposure_name="exposure")
    assert list(ev.columns) == ["mle", "ref", "zero"] and ev.shape == (1, 3)
    assert abs(ev["mle"][0] - mb.loglik[0]) <= 1e-13 * abs(mb.loglik[0])
    refs = [gr.terms(X, part["y"].to_numpy(), par[c].to_numpy(), o, True, phi)[0] for c in par.columns]
    assert rel(ev.to_numpy()[0], refs) <= 1e-12
    with pytest.raises(ValueError):
        dlsa_amd.gamma_model(part, "y", fit_intercept=True, exposure_name="exposure", dispersion=0.0)
    fixed = dlsa_amd.gamma_model(part, "y", fit_intercept=True, exposure_name="exposure", dispersion=0.5)
    assert fixed.attrs["dispersion"] == 0.5 and np.array_equal(fixed["coef"].to_numpy(), out["coef"].to_numpy())


def test_gamma_model_dummy_factor_and_missing_level(eng):
    import pandas as pd
    import dlsa_amd
    rng = np.random.default_rng(2)
    n = 4000
    df = pd.DataFrame({"partition_id": np.zeros(n), "y": 0.0, "dist": rng.normal(5.0, 2.0, n),
                       "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2])})
    df["y"] = rng.gamma(2.0, np.exp(0.1 * (df["dist"] - 5) + 0.4 * (df["carrier"] == "BB")) / 2.0)
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"]}, "factor_dropped": {"carrier": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"]}}
    baseline = ["carrier_AA"]
    want = ["par_id", "coef", "Sig_invMcoef", "intercept", "dist", "carrier_BB", "carrier_CC"]
    out = dlsa_amd.gamma_model(df, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert list(out.columns) == want
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC"]).astype(float)
    b, S, _, phi = gr.fit(Xo, df["y"].to_numpy(), None, True)[:4]
    assert rel(out["coef"], b) <= 1e-10 and rel(out.iloc[:, 3:].to_numpy(), S) <= 1e-10
    assert abs(out.attrs["dispersion"] - phi) <= 1e-10 * phi
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = dlsa_amd.gamma_model(sub, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert any("missing in this data chunk" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (4, 7) and float(np.abs(zero.to_numpy()).max()) == 0.0
    assert zero.attrs["dispersion"] == 0.0
