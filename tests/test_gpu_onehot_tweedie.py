"""GPU: the structured one-hot Tweedie map step (csrc/onehot_tweedie.hip) -- the Tweedie pass and fit on raw numerics + level codes
-- against the dense Tweedie entries and the numpy reference (tests/tweedie_reference.py) on the matrix
oracle.dlsa_oracle.design_matrix builds, at the designs and bars of test_gpu_onehot_gamma.py: the pass at a fixed beta, power and
dispersion (plans with and without a constant column, with and without an offset, rows with y = 0 in every case), the
per-partition fit with estimated and fixed dispersion on strided and contiguous partitions, the refusals and the frame-level
tweedie_model."""
import warnings

import numpy as np
import pytest

import tweedie_reference as tr
from test_gpu_onehot import _plan, _random_design
from test_gpu_onehot_poisson import SHAPES, TOL_FIT, TOL_PASS, _frame, _spec, _zipf_design

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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


def _check_pass(plan, num, codes, y, o, beta, X, power, dispersion, tag=None):
    """structured pass == the dense pass on X == the reference on X, every figure printed before it is asserted"""
    from dlsa_amd import engine
    q = num.shape[1]
    H, g, ll, w, st = engine.onehot_tweedie_pass(plan, dev(num) if q else None, dev(codes), dev(y), dev(beta), power, dispersion,
                                                 offset=dev(o), want_w=True, want_stats=True)
    Hd, gd, lld, wd, std = engine.tweedie_pass(dev(X), dev(y), dev(beta), power, dispersion, offset=dev(o), want_w=True, want_stats=True)
    llr, gr_, Hr, wr, Pr, devr = tr.terms(X, y, beta, power, o, False, dispersion)
    Hn = H.cpu().numpy()
    figs = (abs(float(ll.item()) - llr) / abs(llr), rel(g.cpu().numpy(), gr_), rel(w.cpu().numpy(), wr), rel(Hn, Hr),
            abs(float(st[0].item()) - Pr) / Pr, abs(float(st[1].item()) - devr) / devr)
    dense = (abs(float(ll.item()) - float(lld.item())) / abs(llr), rel(g.cpu().numpy(), gd.cpu().numpy()), rel(w.cpu().numpy(), wd.cpu().numpy()),
             rel(Hn, Hd.cpu().numpy()), rel(st.cpu().numpy(), std.cpu().numpy()))
    print("pass", tag, "vs reference: ll %.2e g %.2e w %.2e H %.2e P %.2e Dev %.2e" % figs, "vs dense: ll %.2e g %.2e w %.2e H %.2e stats %.2e" % dense)
    assert np.isfinite(llr) and np.all(np.isfinite(Hr))
    assert max(figs) <= TOL_PASS and max(dense) <= TOL_PASS, (figs, dense)
    assert np.array_equal(Hn, Hn.T)


@pytest.mark.parametrize("offset,power,dispersion", [(False, 1.5, 1.0), (True, 1.2, 0.37)])
@pytest.mark.parametrize("intercept,baseline", [(True, True), (False, False)])
@pytest.mark.parametrize("n,q,nlevels", SHAPES)
def test_pass_matches_dense_and_reference(api, orc, n, q, nlevels, intercept, baseline, offset, power, dispersion):
    rng = np.random.default_rng(n + q)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels, intercept=intercept, baseline=baseline)
    codes[rng.integers(0, n, max(1, n // 50)), 0] = -1          # unknown level: no column
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.4                             # eta spans a few units
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    y = tr.draw(rng, np.exp(np.clip(0.5 * (X @ beta), -20, 4)), power, 1.0)     # the pass is checked away from the MLE
    y[0] = 0.0                                                  # (the one-row shape is a zero row alone: the pass takes it)
    _check_pass(plan, num, codes, y, o, beta, X, power, dispersion, (n, q, nlevels, intercept, baseline, offset, "%d zero rows" % (y == 0).sum()))


def _fit_case(orc, n, q, nlevels, seed, power):
    rng = np.random.default_rng(seed)
    p, num, codes, desc, nl, level_col = _zipf_design(rng, n, q, nlevels)
    X, _ = orc.design_matrix(num, codes, *desc)
    bt = rng.normal(size=p) * 0.3
    bt[0] = -0.5
    e = rng.uniform(0.5, 2.0, n)
    y = tr.draw(rng, e * np.exp(X @ bt), power, 1.0)
    return p, num, codes, desc, nl, level_col, X, y, e


def _assert_rows(X, y, parts, least=5):
    """the test's own inputs: a level needs rows -- positive ones -- in every partition (else its column is zero there, or its
    coefficient runs off to minus infinity)"""
    for k, sl in enumerate(parts):
        cnt = ((X[sl] != 0) & (y[sl] > 0)[:, None]).sum(0)
        print("partition", k, "min positive rows per column", cnt.min(), "zero rows %.2f" % (y[sl] == 0).mean())
        assert cnt.min() >= least, (k, cnt.min())
        assert (y[sl] == 0).any()


@pytest.mark.parametrize("n,q,nlevels,K,strided,seed,power", [(60_000, 7, (11, 6, 20, 110, 110), 4, True, 60_007, 1.5),
                                                              (24_000, 2, (40, 5), 6, False, 24_002, 1.3)])
def test_fit_matches_dense_and_reference(api, orc, n, q, nlevels, K, strided, seed, power):
    from dlsa_amd import engine
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, seed, power)
    o = np.log(e)
    if strided:
        parts = [slice(k, n, K) for k in range(K)]
        first, rows, step = list(range(K)), [len(range(k, n, K)) for k in range(K)], K
    else:
        parts = [slice(k * n // K, (k + 1) * n // K) for k in range(K)]
        first, rows, step = [s.start for s in parts], [s.stop - s.start for s in parts], 1
    _assert_rows(X, y, parts)
    plan = _plan(api, p, desc, nl, level_col)
    for dispersion in (None, 0.5):
        r = engine.onehot_tweedie_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step, offset=dev(o), power=power,
                                         dispersion=dispersion)
        d = engine.tweedie_fit_ex(dev(X), dev(y), first, rows, row_step=step, offset=dev(o), power=power, dispersion=dispersion)
        assert r["status"] == [0] * K and d["status"] == [0] * K and r["df"] == d["df"] == [m - p for m in rows]
        for k, sl in enumerate(parts):
            b, S, ll, phi, P, dv = tr.fit(X[sl], y[sl], power, o[sl], False, dispersion)
            figs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), S), rel(r["Sig_invMcoef"][k].cpu().numpy(), S @ b),
                    abs(r["loglik"][k] - ll) / abs(ll), abs(r["dispersion"][k] - phi) / phi, abs(r["pearson"][k] - P) / P,
                    abs(r["deviance"][k] - dv) / dv)
            dense = (rel(r["coef"][k].cpu().numpy(), d["coef"][k].cpu().numpy()), rel(r["Sig_inv"][k].cpu().numpy(), d["Sig_inv"][k].cpu().numpy()),
                     abs(r["dispersion"][k] - d["dispersion"][k]) / phi)
            print("fit partition", k, "dispersion", dispersion, "vs reference: coef %.2e Sig_inv %.2e Sig_invMcoef %.2e loglik %.2e phi %.2e "
                  "P %.2e Dev %.2e" % figs, "vs dense: coef %.2e Sig_inv %.2e phi %.2e" % dense, "iters", r["n_iter"][k])
            assert max(figs) <= TOL_FIT and max(dense) <= TOL_FIT, (k, figs, dense)


def test_structured_equals_dense_strided_equals_contiguous(api, orc):
    n, q, nlevels, K, power = 30_001, 3, (7, 4, 12), 5, 1.6
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 41, power)
    _assert_rows(X, y, [slice(k, n, K) for k in range(K)])
    spec = _spec(api, q, nlevels, desc)
    assert spec.onehot_plan() is not None
    dn, dc, dy, de = dev(num), dev(codes), dev(y), dev(e)
    a = api.fit_tweedie_design(dn, dc, dy, spec, partition_num=K, exposure=de, power=power)
    d = api.fit_tweedie_design(dn, dc, dy, spec, partition_num=K, exposure=de, power=power, structured=False)
    assert a.status == [0] * K and d.status == [0] * K and a.names == spec.names and d.names == spec.names
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(d, f).cpu().numpy())
        print("structured vs dense", f, "%.2e" % err)
        assert err <= TOL_FIT
    assert rel(a.loglik, d.loglik) <= TOL_FIT and rel(a.extra["dispersion"], d.extra["dispersion"]) <= TOL_FIT
    assert a.extra["df"] == d.extra["df"] == [len(range(k, n, K)) - p for k in range(K)]
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    c = api.fit_tweedie_design(dev(num[perm]), dev(codes[perm]), dev(y[perm]), spec, part_offsets=offs, offset=dev(np.log(e[perm])), power=power)
    assert c.status == [0] * K
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(c, f).cpu().numpy())
        print("strided vs contiguous", f, "%.2e" % err)
        assert err <= 1e-13
    assert rel(a.extra["dispersion"], c.extra["dispersion"]) <= 1e-13
    # bit-reproducible, the dispersion included
    a2 = api.fit_tweedie_design(dn, dc, dy, spec, partition_num=K, exposure=de, power=power)
    assert torch.equal(a.coef, a2.coef) and torch.equal(a.Sig_inv, a2.Sig_inv) and a.loglik == a2.loglik and a.extra == a2.extra
    with pytest.raises(ValueError):
        api.fit_tweedie_design(dn, dc, dy, spec, offset=torch.log(de), exposure=de)
    with pytest.raises(ValueError):
        api.fit_tweedie_design(dn, dc, dy - dy, spec)           # no positive response
    with pytest.raises(ValueError):
        api.fit_tweedie_design(dn, dc, dy, spec, dispersion=-0.5)
    with pytest.raises(ValueError):
        api.fit_tweedie_design(dn, dc, dy, spec, power=2.0)


def test_invalid_rows_are_refused_naming_the_partition(api, orc):
    from dlsa_amd import _lib, engine
    n, q, nlevels = 2000, 2, (4, 3)
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 9, 1.5)
    plan = _plan(api, p, desc, nl, level_col)
    for bad in (-2.0, float("nan"), float("inf")):
        yb = y.copy(); yb[1500] = bad
        with pytest.raises(_lib.DlsaError) as ex:
            engine.onehot_tweedie_fit_ex(plan, dev(num), dev(codes), dev(yb), [0, 1000], [1000, 1000])
        assert ex.value.code == 1 and "partition 1" in str(ex.value)
    y0 = y.copy(); y0[1000:] = 0.0                           # rows, none positive
    with pytest.raises(_lib.DlsaError) as ex:
        engine.onehot_tweedie_fit_ex(plan, dev(num), dev(codes), dev(y0), [0, 1000], [1000, 1000])
    assert ex.value.code == 1 and "partition 1" in str(ex.value) and "no positive response" in str(ex.value)
    with pytest.raises(_lib.DlsaError) as ex:                # 0 < n <= p rows under an estimated dispersion
        engine.onehot_tweedie_fit_ex(plan, dev(num), dev(codes), dev(y), [0, 1000], [1000, p])
    assert ex.value.code == 1 and "partition 1" in str(ex.value) and "degrees of freedom" in str(ex.value)
    for power in (1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match="power must lie strictly between 1 and 2"):
            engine.onehot_tweedie_fit_ex(plan, dev(num), dev(codes), dev(y), [0, 1000], [1000, 1000], power=power)
    r = engine.onehot_tweedie_fit_ex(plan, dev(num), dev(codes), dev(y), [0, 1000, 1000], [1000, 0, 1000])
    assert r["status"] == [0, 4, 0] and not r["Sig_inv"][1].any() and r["dispersion"][1] == 0.0


def _tweedie_frame(seed, n, power):
    df, dummy_info, baseline, names, Xo = _frame(seed, n)
    rng = np.random.default_rng(seed + 1)
    eta = -0.3 + 0.1 * (df["dist"] - 5) - 0.02 * (df["age"] - 40) + 0.4 * (df["carrier"] == "BB") - 0.3 * (df["carrier"] == "CC") \
        + 0.2 * (df["region"] == "s") - 0.25 * (df["region"] == "w")
    df["y"] = tr.draw(rng, (df["expo"] * np.exp(eta)).to_numpy(), power, 1.0)
    return df, dummy_info, baseline, names, Xo


def test_tweedie_model_structured_equals_the_dense_call(api):
    import pandas as pd
    power = 1.5
    df, dummy_info, baseline, names, Xo = _tweedie_frame(2, 6000, power)
    assert 0.05 < float((df["y"] == 0).mean()) < 0.6
    kw = dict(fit_intercept=True, exposure_name="expo", power=power, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    out = api.tweedie_model(df, "y", structured=True, **kw)
    dense = api.tweedie_model(df, "y", structured=False, **kw)
    default = api.tweedie_model(df, "y", **kw)
    want = ["par_id", "coef", "Sig_invMcoef"] + names
    assert list(out.columns) == want and list(dense.columns) == want
    assert default.equals(dense) and default.to_numpy().tobytes() == dense.to_numpy().tobytes()      # the default is the dense path
    o = np.log(df["expo"].to_numpy())
    b, S, ll, phi = tr.fit(Xo, df["y"].to_numpy(), power, o, True)[:4]
    figs = (rel(out["coef"], b), rel(out[names].to_numpy(), S), rel(out["Sig_invMcoef"], S @ b), abs(out.attrs["dispersion"] - phi) / phi)
    print("tweedie_model structured vs reference", figs)
    assert max(figs) <= TOL_FIT and out.attrs["power"] == power
    assert rel(out["coef"], dense["coef"]) <= TOL_FIT and rel(out[names].to_numpy(), dense[names].to_numpy()) <= TOL_FIT
    assert rel(out["Sig_invMcoef"], dense["Sig_invMcoef"]) <= TOL_FIT
    assert abs(out.attrs["dispersion"] - dense.attrs["dispersion"]) <= TOL_FIT * phi
    # a missing level: the zero block and the reference's warning, from the codes
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = api.tweedie_model(sub, "y", structured=True, **kw)
    assert any("missing in this data chunk" in str(w.message) and "Skip modeling" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (8, 11) and float(np.abs(zero.to_numpy()).max()) == 0.0
    # eval: the quasi-log-likelihood of each estimator column at the fit's dispersion
    par = pd.DataFrame({"mle": out["coef"].to_numpy(), "ref": b, "zero": np.zeros(8)})
    ekw = {k: v for k, v in kw.items() if k != "power"}
    ev = api.tweedie_model_eval(df, "y", par, power, phi, structured=True, **ekw)
    refs = [tr.terms(Xo, df["y"].to_numpy(), par[c].to_numpy(), power, o, True, phi)[0] for c in par.columns]
    print("tweedie_model_eval structured vs reference %.2e" % rel(ev.to_numpy()[0], refs))
    assert list(ev.columns) == ["mle", "ref", "zero"] and rel(ev.to_numpy()[0], refs) <= 1e-12
    evd = api.tweedie_model_eval(df, "y", par, power, phi, structured=False, **ekw)
    assert rel(ev.to_numpy()[0], evd.to_numpy()[0]) <= 1e-12
