"""GPU: the Poisson regression map step (csrc/poisson.hip) against the numpy reference (tests/poisson_reference.py): the pass at a
fixed beta (loglik, score, mu, information) at every Gram width class, the per-partition fit, strided partitions, edge cases,
reproducibility, the end-to-end DLSA combine, the statistics of the combine, the frame-level poisson_model and a 1e7 x 100 fit."""
import math
import warnings

import numpy as np
import pytest

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


def _data(seed, n, p, intercept, offset, b0=0.3, scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.where(np.arange(p) < max(1, int(0.4 * p)), 0.5, 0.0) * scale / max(1.0, math.sqrt(p / 10))
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    eta = X @ beta + (b0 if intercept else 0.0) + (0.0 if o is None else o)
    y = rng.poisson(np.exp(eta)).astype(np.float64)
    return X, y, o


def _check_pass(eng, X, y, o, beta, intercept, tol=1e-12, Xd=None):
    """Xd: the device tensor to pass for X (a view with its own pitch / alignment); default a contiguous copy"""
    Xc, yd, od, bd = _dev(X, y, o, beta)
    H, g, ll, w = eng.poisson_pass(Xc if Xd is None else Xd, yd, bd, offset=od, fit_intercept=intercept, want_w=True)
    llr, gr, Hr, mur = pr.terms(X, y, beta, o, intercept)
    assert abs(float(ll.item()) - llr) <= tol * abs(llr), (float(ll.item()), llr)
    assert rel(g.cpu().numpy(), gr) <= tol, rel(g.cpu().numpy(), gr)
    assert rel(w.cpu().numpy(), mur) <= tol
    Hn = H.cpu().numpy()
    assert rel(Hn, Hr) <= tol, rel(Hn, Hr)
    assert np.array_equal(Hn, Hn.T)


def _away_from_optimum(pe):
    return np.linspace(-0.8, 0.6, pe) / max(1.0, math.sqrt(pe / 10))


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, False), (False, True), (True, True)])
def test_pass_matches_reference(eng, p, intercept, offset):
    n = 3001
    X, y, o = _data(10 + p, n, p, intercept, offset)
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), intercept)


# Shapes of the row pass no 3001-row case reaches.  p > 1024 is NC = 16 with one row per wave (1025: the scalar loads, 1030: the
# 16-byte ones); the short ones have fewer rows than one batch of 8 (or a single row), so at NC = 1 every prefetch of the second
# register set is a clamped re-read of row n - 1 and most waves process nothing, and at NC = 2 there is one full and one partial batch.
SHORT_AND_WIDE = [(67, 1025), (67, 1030), (1, 1), (1, 2), (5, 7), (7, 8), (9, 130), (13, 128)]


@pytest.mark.parametrize("n,p", SHORT_AND_WIDE)
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_short_and_wide_shapes(eng, n, p, intercept, offset):
    X, y, o = _data(900 + p + n, n, p, intercept, offset)
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), intercept)


# Edge shapes of the shared row-pass skeleton (csrc/row_pass.h) that neither list above reaches: n = 1003 at p = 3 is several batches
# per wave on the NC = 1 two-set loop with a last prefetched batch past the end, and a pair that straddles p; n = 300 001 at p = 3
# meets the cap on the block count (37 501 batches of 8 ask for 2344 blocks of 16); 129, 257 and 513 are the scalar loads at
# NC = 2, 4 and 8 with one column in the last chunk.
SKELETON_EDGES = [(1003, 3), (300001, 3), (67, 129), (67, 257), (67, 513)]


@pytest.mark.parametrize("n,p", SKELETON_EDGES)
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_edge_shapes_of_the_row_pass_skeleton(eng, n, p, intercept, offset):
    X, y, o = _data(700 + p + n % 1000, n, p, intercept, offset)
    _check_pass(eng, X, y, o, _away_from_optimum(p + intercept), intercept)


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


def test_pass_exp_is_exact_to_two_ulp_over_the_range(eng):
    # p = 1, beta = 1, no intercept, no offset: eta is x itself, so w = exp(x) of the kernel's exp
    x = np.concatenate([np.linspace(-745.0, 709.7, 20001), [-746.0, -800.0, -1e6, 709.78, 709.79, 720.0, 1e6]])
    X = x[:, None].copy()
    Xd, yd, bd = _dev(X, np.zeros(len(x)), np.ones(1))
    _, _, ll, w = eng.poisson_pass(Xd, yd, bd, want_H=False, want_w=True)
    w = w.cpu().numpy()
    with np.errstate(over="ignore"):
        ref = np.exp(x)
    fin = np.isfinite(ref)
    assert np.all(np.abs(w[fin] - ref[fin]) <= 2 * np.spacing(ref[fin]))
    assert np.all(w[x <= -746.0] == 0.0)
    assert np.all(np.isinf(w[x >= 709.79]) & (w[x >= 709.79] > 0))
    assert np.isfinite(w[x == 709.78]).all()
    assert float(ll.item()) == -math.inf                    # mu overflowed: the driver's failed step


@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_eta_spanning_700(eng, intercept, offset):
    n, p = 2000, 3
    X, y, o = _data(20, n, p, intercept, offset)
    X[:, 0] = np.linspace(-1.0, 1.0, n)
    beta = np.array([699.0, 0.3, -0.2]) if not intercept else np.array([-0.4, 699.0, 0.3, -0.2])
    ll, g, H, mu = pr.terms(X, y, beta, o, intercept)
    assert np.ptp(np.log(mu[mu > 0])) > 1300 and np.isfinite(ll) and np.all(np.isfinite(H))
    _check_pass(eng, X, y, o, beta, intercept)


def _fit(eng, X, y, o, offs, intercept, **kw):
    Xd, yd, od = _dev(X, y, o)
    return eng.poisson_fit_ex(Xd, yd, offs[:-1], [offs[k + 1] - offs[k] for k in range(len(offs) - 1)], offset=od,
                              fit_intercept=intercept, **kw)


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("intercept,offset", [(True, True), (False, False)])
def test_fit_matches_reference(eng, p, intercept, offset):
    n, K = 2 * max(3000, 6 * p), 2
    X, y, o = _data(40 + p, n, p, intercept, offset)
    offs = [k * n // K for k in range(K + 1)]
    r = _fit(eng, X, y, o, offs, intercept)
    assert r["status"] == [0] * K, r["status"]
    for k in range(K):
        sl = slice(offs[k], offs[k + 1])
        b, H, ll = pr.fit(X[sl], y[sl], None if o is None else o[sl], intercept)
        assert rel(r["coef"][k].cpu().numpy(), b) <= 1e-10
        assert rel(r["Sig_inv"][k].cpu().numpy(), H) <= 1e-10
        assert rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b) <= 1e-10
        assert abs(r["loglik"][k] - ll) <= 1e-10 * abs(ll)


def test_strided_partitions_equal_contiguous_copies(eng):
    import dlsa_amd
    n, p, K = 30_001, 8, 5
    X, y, o = _data(70, n, p, True, True)
    e = np.exp(o)
    Xd, yd, ed = _dev(X, y, e)
    a = dlsa_amd.fit_poisson_partitions(Xd, yd, partition_num=K, fit_intercept=True, exposure=ed)
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    Xc, yc, ec = _dev(X[perm], y[perm], e[perm])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    b = dlsa_amd.fit_poisson_partitions(Xc, yc, part_offsets=offs, fit_intercept=True, exposure=ec)
    assert a.status == [0] * K and b.status == [0] * K
    assert a.names == ["intercept"] + ["x%d" % i for i in range(p)]
    assert rel(a.coef.cpu().numpy(), b.coef.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_inv.cpu().numpy(), b.Sig_inv.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_invMcoef.cpu().numpy(), b.Sig_invMcoef.cpu().numpy()) <= 1e-13


def test_fit_empty_and_all_zero_partitions(eng):
    n, p = 6000, 4
    X, y, o = _data(50, n, p, True, True)
    y[2000:4000] = 0.0
    offs = [0, 2000, 4000, 4000, n]
    r = _fit(eng, X, y, o, offs, True)
    assert r["status"] == [0, 4, 4, 0], r["status"]
    for k in (1, 2):
        assert not r["Sig_inv"][k].any() and not r["coef"][k].any() and not r["Sig_invMcoef"][k].any()
        assert r["loglik"][k] == 0.0
    b, H, _ = pr.fit(X[4000:], y[4000:], o[4000:], True)
    assert rel(r["coef"][3].cpu().numpy(), b) <= 1e-10


def test_collinear_column_is_not_spd(eng):
    X, y, _ = _data(60, 2000, 5, True, False)
    X = np.column_stack([X, X[:, 0]])                       # duplicated column: singular information
    r = _fit(eng, X, y, None, [0, 2000], False)
    assert r["status"] == [2] and r["rc"] == 4


def test_negative_or_non_finite_counts_are_refused(eng):
    import dlsa_amd
    from dlsa_amd import _lib
    X, y, o = _data(61, 1000, 3, True, True)
    y_bad = y.copy(); y_bad[700] = -1.0
    with pytest.raises(ValueError):
        dlsa_amd.fit_poisson_partitions(*_dev(X, y_bad), fit_intercept=True)
    with pytest.raises(_lib.DlsaError) as ex:       # (the C ABI's own check, below the Python one)
        _fit(eng, X, y_bad, o, [0, 500, 1000], True)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    o_bad = o.copy(); o_bad[3] = np.nan
    with pytest.raises(_lib.DlsaError) as ex:
        _fit(eng, X, y, o_bad, [0, 500, 1000], True)
    assert "partition 0" in str(ex.value)
    with pytest.raises(ValueError):
        dlsa_amd.fit_poisson_partitions(*_dev(X, y), offset=_dev(o)[0], exposure=_dev(np.exp(o))[0])
    # the pass reports an invalid count as a NaN log-likelihood
    _, _, ll, _ = eng.poisson_pass(*_dev(X, y_bad, np.zeros(3)))
    assert math.isnan(float(ll.item()))


def _far_start():
    rng = np.random.default_rng(62)
    X = rng.uniform(-0.5, 0.5, (20_000, 3))
    y = rng.poisson(np.exp(5.0 + X @ np.array([4.0, -3.0, 2.0]))).astype(np.float64)
    return X, y


def test_far_start_with_large_counts_converges(eng):
    X, y = _far_start()
    # no intercept: beta = 0 is far from the MLE (the counts ask for eta ~ 5), the first full steps overshoot
    r = _fit(eng, X, y, None, [0, 20_000], False)
    assert r["status"] == [0]
    b, H, ll = pr.fit(X, y, None, False)
    assert rel(r["coef"][0].cpu().numpy(), b) <= 1e-10 and rel(r["Sig_inv"][0].cpu().numpy(), H) <= 1e-10


def test_far_start_is_halved(eng):
    """the host loop's safeguard: the undamped iteration from the same start DIVERGES (its first full step overflows mu: the second
    evaluation is -inf), so every evaluation the fit makes beyond those two is the halvings' doing"""
    X, y = _far_start()
    evals, _, lls = nw.undamped(lambda b: pr.terms(X, y, b, None, False)[:3], np.zeros(3), 1e-13)
    assert evals is None and len(lls) == 2 and lls[1] == -math.inf
    r = _fit(eng, X, y, None, [0, 20_000], False)
    print("far start: %d evaluations, the undamped iteration diverged at its second" % r["n_iter"][0])
    assert r["status"] == [0] and r["rc"] == 0
    assert r["n_iter"][0] > len(lls)


# Only the host loop is under test: one partition of 600 rows, intercept and offset on; p = 64 (the row pass's widest register
# tier) once.  The undamped reference needs 5 evaluations at p = 3 and 6 at p = 64, so max_iter + 1 <= 4 never suffices.
@pytest.mark.parametrize("p,max_iter", [(3, 1), (3, 2), (3, 3), (64, 2)])
def test_budget_stops_at_the_evaluated_iterate(eng, p, max_iter):
    n = 600
    X, y, o = _data(300 + p, n, p, True, True)
    start = np.zeros(p + 1)
    start[0] = np.log(y.sum() / np.exp(o).sum())
    evals, bs, lls = nw.undamped(lambda b: pr.terms(X, y, b, o, True)[:3], start, 1e-13)
    assert evals is not None and evals > max_iter + 1 and nw.monotone(lls[:max_iter + 1])       # no halving in the budget
    r = _fit(eng, X, y, o, [0, n], True, max_iter=max_iter)
    assert r["status"] == [1] and r["rc"] == 5
    assert r["n_iter"] == [max_iter + 1]
    # max_iter steps were taken; the last evaluation's step was not: coef is where H, g and loglik were evaluated
    coef = r["coef"][0]
    assert rel(coef.cpu().numpy(), bs[max_iter]) <= 1e-10
    assert abs(r["loglik"][0] - lls[max_iter]) <= 1e-10 * abs(lls[max_iter])
    Xd, yd, od = _dev(X, y, o)
    H, _, _, _ = eng.poisson_pass(Xd, yd, coef, offset=od, fit_intercept=True)
    assert rel(r["Sig_inv"][0].cpu().numpy(), H.cpu().numpy()) <= 1e-12
    assert rel(r["Sig_invMcoef"][0].cpu().numpy(), H.cpu().numpy() @ coef.cpu().numpy()) <= 1e-12


def test_fit_is_bit_reproducible(eng):
    import dlsa_amd
    X, y, o = _data(80, 50_000, 30, True, True)
    Xd, yd, od = _dev(X, y, o)
    a = dlsa_amd.fit_poisson_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    b = dlsa_amd.fit_poisson_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K = 80_000, 10, 8
    X, y, o = _data(90, n, p, True, True)
    Xd, yd, od = _dev(X, y, o)
    mb = dlsa_amd.fit_poisson_partitions(Xd, yd, partition_num=K, fit_intercept=True, offset=od)
    assert mb.status == [0] * K
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [pr.block(X[k::K], y[k::K], o[k::K], True) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = dlsa_amd.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


def test_dlsa_estimate_is_close_to_the_global_mle(eng):
    import dlsa_amd
    df = dlsa_amd.simulate_poisson(2_000_000, 10, 20)
    assert list(df.columns) == ["partition_id", "y"] + ["x%d" % i for i in range(10)]
    X = torch.from_numpy(np.ascontiguousarray(df.iloc[:, 2:].to_numpy())).cuda()
    y = torch.from_numpy(df["y"].to_numpy()).cuda()
    mb = dlsa_amd.fit_poisson_partitions(X, y, partition_num=20, fit_intercept=True)
    assert mb.status == [0] * 20
    theta = dlsa_amd.dlsa_mapred(mb)["beta_byOLS"].to_numpy()
    one = dlsa_amd.fit_poisson_partitions(X, y, fit_intercept=True)
    assert one.status == [0]
    se = np.sqrt(np.diag(np.linalg.inv(one.Sig_inv[0].cpu().numpy())))
    gap = np.abs(theta - one.coef[0].cpu().numpy()) / se
    assert gap.max() <= 0.1, gap
    # and the MLE itself sits where the simulator put beta*: intercept log(1) = 0, 0.5 on the first 4 columns
    truth = np.concatenate([[0.0], np.where(np.arange(10) < 4, 0.5, 0.0)])
    assert np.all(np.abs(one.coef[0].cpu().numpy() - truth) <= 5 * se)


def test_poisson_model_frame_and_eval(eng):
    import pandas as pd
    import dlsa_amd
    df = dlsa_amd.simulate_poisson(5000, 6, 1, seed=7, exposure=True)
    assert list(df.columns) == ["partition_id", "y", "exposure"] + ["x%d" % i for i in range(6)]
    part = df.drop(columns=["partition_id"])
    out = dlsa_amd.poisson_model(part, "y", fit_intercept=True, exposure_name="exposure")
    names = ["intercept"] + ["x%d" % i for i in range(6)]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (7, 10)
    X = part[names[1:]].to_numpy()
    Xd, yd, ed = _dev(X, part["y"].to_numpy(), part["exposure"].to_numpy())
    mb = dlsa_amd.fit_poisson_partitions(Xd, yd, fit_intercept=True, exposure=ed)
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out["Sig_invMcoef"].to_numpy(), mb.Sig_invMcoef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    o = np.log(part["exposure"].to_numpy())
    b, H, ll = pr.fit(X, part["y"].to_numpy(), o, True)
    assert rel(out["coef"].to_numpy(), b) <= 1e-10
    # eval: the log-likelihood of each estimator column, shaped like logistic_model_eval
    par = pd.DataFrame({"mle": mb.coef[0].cpu().numpy(), "ref": b, "zero": np.zeros(7)})
    ev = dlsa_amd.poisson_model_eval(part, "y", par, fit_intercept=True, exposure_name="exposure")
    assert list(ev.columns) == ["mle", "ref", "zero"] and ev.shape == (1, 3)
    od = torch.log(ed)
    for c in par.columns:              # the tensor path: one pass per estimator column
        _, _, ll, _ = eng.poisson_pass(Xd, yd, _dev(par[c].to_numpy())[0], offset=od, fit_intercept=True, want_H=False)
        assert ev[c][0] == float(ll.item())
    assert abs(ev["mle"][0] - mb.loglik[0]) <= 1e-13 * abs(mb.loglik[0])
    refs = [pr.terms(X, part["y"].to_numpy(), par[c].to_numpy(), o, True)[0] for c in par.columns]
    assert rel(ev.to_numpy()[0], refs) <= 1e-12


def test_poisson_model_missing_dummy_level_gives_zero_block(eng):
    import pandas as pd
    import dlsa_amd
    rng = np.random.default_rng(2)
    n = 4000
    df = pd.DataFrame({"partition_id": np.zeros(n), "y": 0.0, "dist": rng.normal(5.0, 2.0, n),
                       "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2])})
    df["y"] = rng.poisson(np.exp(0.1 * (df["dist"] - 5) + 0.4 * (df["carrier"] == "BB"))).astype(float)
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"]}, "factor_dropped": {"carrier": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"]}}
    baseline = ["carrier_AA"]
    want = ["par_id", "coef", "Sig_invMcoef", "intercept", "dist", "carrier_BB", "carrier_CC"]
    out = dlsa_amd.poisson_model(df, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert list(out.columns) == want
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC"]).astype(float)
    b, H, _ = pr.fit(Xo, df["y"].to_numpy(), None, True)
    assert rel(out["coef"], b) <= 1e-10 and rel(out.iloc[:, 3:].to_numpy(), H) <= 1e-10
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = dlsa_amd.poisson_model(sub, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert any("missing in this data chunk" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (4, 7) and float(np.abs(zero.to_numpy()).max()) == 0.0


def test_full_size_fit_with_intercept_and_offset(eng):
    import dlsa_amd
    n, p = 10_000_000, 100
    X, _ = eng.synth(123, 0, n, p, labels=False)
    beta = torch.zeros(p + 1, dtype=torch.float64, device="cuda")
    beta[0] = 0.2
    beta[1: 1 + int(0.4 * p)] = 0.5
    g = torch.Generator(device="cuda").manual_seed(5)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    y = torch.poisson(torch.exp(X @ beta[1:] + beta[0] + o), generator=g)
    mb = dlsa_amd.fit_poisson_partitions(X, y, fit_intercept=True, offset=o)
    assert mb.status == [0]
    coef = mb.coef[0]
    H, gs, ll, _ = eng.poisson_pass(X, y, coef, offset=o, fit_intercept=True)
    assert float(gs.abs().max()) <= 1e-9 * float(y.sum())             # the score vanishes at the returned coef
    Hn = H.cpu().numpy()
    assert np.array_equal(Hn, Hn.T) and np.all(np.linalg.eigvalsh(Hn) > 0)
    assert rel(Hn, mb.Sig_inv[0].cpu().numpy()) <= 1e-12
    assert abs(float(ll.item()) - mb.loglik[0]) <= 1e-12 * abs(mb.loglik[0])
    se = np.sqrt(np.diag(np.linalg.inv(Hn)))
    z = np.abs(coef.cpu().numpy() - beta.cpu().numpy()) / se
    assert z.max() <= 5.0, z.max()
    # a 2e5-row slice against the reference
    m = 200_000
    _check_pass(eng, X[:m].cpu().numpy(), y[:m].cpu().numpy(), o[:m].cpu().numpy(), coef.cpu().numpy(), True)
