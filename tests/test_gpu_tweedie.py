"""GPU: the Tweedie map step (csrc/tweedie.hip) against the numpy reference (tests/tweedie_reference.py): the pass at a fixed beta,
power and dispersion (quasi-log-likelihood, score, weights, information, Pearson and deviance sums) at every class the count pass
and the Gram dispatch distinguish, the per-partition fit with estimated and fixed dispersion, strided partitions, reproducibility,
edge cases and refusals, the calibration of the block that the dispersion is there for, the end-to-end DLSA combine and the
frame-level tweedie_model.  Every pass case has a row with y = 0.

The tolerances are the project's parity bars of the Poisson and Gamma tests (1e-12 for a pass, 1e-10 for a fit): on the CPU the fp64
reference agrees with a longdouble run of itself to <= 2e-15 on these inputs and to <= 2.7e-14 in the eta-span cases
(test_tweedie_cpu.py asserts 1e-13)."""
import math
import warnings

import numpy as np
import pytest

import newton_reference as nw
import tweedie_reference as tr

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


def _check_pass(eng, X, y, o, beta, intercept, power=1.5, dispersion=1.0, tol=1e-12, Xd=None):
    """Xd: the device tensor to pass for X (a view with its own pitch / alignment); default a contiguous copy"""
    Xc, yd, od, bd = _dev(X, y, o, beta)
    H, g, ll, w, st = eng.tweedie_pass(Xc if Xd is None else Xd, yd, bd, power, dispersion, offset=od, fit_intercept=intercept,
                                       want_w=True, want_stats=True)
    llr, gr_, Hr, wr, Pr, devr = tr.terms(X, y, beta, power, o, intercept, dispersion)
    Hn, P, dev = H.cpu().numpy(), float(st[0].item()), float(st[1].item())
    errs = {"ll": abs(float(ll.item()) - llr) / abs(llr), "g": rel(g.cpu().numpy(), gr_), "w": rel(w.cpu().numpy(), wr), "H": rel(Hn, Hr),
            "P": abs(P - Pr) / Pr, "Dev": abs(dev - devr) / devr}
    print("tweedie pass n=%d p=%d power=%g (%d zero rows): %s" % (X.shape[0], X.shape[1], power, int((y == 0).sum()),
                                                                 " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= tol for v in errs.values()), errs
    assert np.array_equal(Hn, Hn.T)


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("dispersion", [1.0, 0.37])
def test_pass_matches_reference(eng, p, intercept, offset, dispersion):
    n = 3 * p + 37
    X, y, o = tr.data(10 + p, n, p, intercept, offset)
    assert y[0] == 0.0 and (y > 0).any()
    _check_pass(eng, X, y, o, tr.away_from_optimum(p + intercept), intercept, 1.5, dispersion)


@pytest.mark.parametrize("p", [7, 130, 600])
@pytest.mark.parametrize("power", [1.2, 1.8])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_other_powers(eng, p, power, intercept, offset):
    n = 3 * p + 37
    X, y, o = tr.data(10 + p, n, p, intercept, offset, power)
    assert (y == 0).any() and (y > 0).any()
    _check_pass(eng, X, y, o, tr.away_from_optimum(p + intercept), intercept, power, 0.37)


# fewer rows than one batch of 8 (or a single row): at NC = 1 every prefetch of the second register set is a clamped re-read of row
# n - 1; p = 1030 is NC = 16 with one row per wave.  The single row is once zero (data() makes row 0 one) and once positive.
@pytest.mark.parametrize("n", [1, 5, 9])
@pytest.mark.parametrize("p", [3, 130, 1030])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_short_and_wide_shapes(eng, n, p, intercept, offset):
    X, y, o = tr.data(900 + p + n, n, p, intercept, offset)
    assert y[0] == 0.0
    _check_pass(eng, X, y, o, tr.away_from_optimum(p + intercept), intercept, 1.5, 0.37)
    if n == 1:
        _check_pass(eng, X, np.array([1.7]), o, tr.away_from_optimum(p + intercept), intercept, 1.5, 0.37)


@pytest.mark.parametrize("p", [8, 130, 1030])
@pytest.mark.parametrize("pad", [3, 2])
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_pass_even_width_on_the_scalar_loads(eng, p, pad, intercept, offset):
    """an even p takes the scalar loads only through the rows' pitch or base: columns 1 .. p of a buffer with p + 3 columns (an odd
    pitch) and of one with p + 2 (an even pitch, the base 8 bytes off a 16-byte boundary), passed as views, without a copy"""
    n = 67
    X, y, o = tr.data(900 + p + n, n, p, intercept, offset)
    big = torch.zeros((n, p + pad), dtype=torch.float64, device="cuda")
    Xd = big[:, 1:1 + p]
    Xd.copy_(torch.from_numpy(X))
    assert Xd.stride(0) == p + pad and Xd.stride(1) == 1
    if pad == 2:
        assert Xd.data_ptr() % 16 == 8
    _check_pass(eng, X, y, o, tr.away_from_optimum(p + intercept), intercept, Xd=Xd)


@pytest.mark.parametrize("power", [1.5, 1.2])
def test_pass_eta_spanning_600(eng, power):
    X, y, o, beta = tr.eta_span_case(power)
    ll, g, H, w, P, dev = tr.terms(X, y, beta, power, o, True)
    eta = tr.design(X, True) @ beta + o
    assert np.ptp(eta) > 590 and (y == 0).any() and all(np.isfinite(v).all() for v in (ll, g, H, w, P, dev))
    _check_pass(eng, X, y, o, beta, True, power)


def _fit(eng, X, y, o, offs, intercept, **kw):
    Xd, yd, od = _dev(X, y, o)
    return eng.tweedie_fit_ex(Xd, yd, offs[:-1], [offs[k + 1] - offs[k] for k in range(len(offs) - 1)], offset=od,
                              fit_intercept=intercept, **kw)


@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("intercept,offset", [(True, True), (False, False)])
def test_fit_matches_reference(eng, p, intercept, offset):
    n, K, power = max(2000, 10 * p), 3, 1.5
    X, y, o = tr.data(40 + p, n, p, intercept, offset)
    offs = [0, int(0.30 * n), int(0.62 * n), n]                 # unequal sizes
    est = _fit(eng, X, y, o, offs, intercept, power=power)
    fix = _fit(eng, X, y, o, offs, intercept, power=power, dispersion=0.5)
    assert est["status"] == [0] * K and fix["status"] == [0] * K, (est["status"], fix["status"])
    assert est["df"] == [offs[k + 1] - offs[k] - p - intercept for k in range(K)]
    worst = {}
    for k in range(K):
        sl = slice(offs[k], offs[k + 1])
        ok = None if o is None else o[sl]
        b, S, ll, phi, P, dev = tr.fit(X[sl], y[sl], power, ok, intercept)
        ll5 = tr.terms(X[sl], y[sl], b, power, ok, intercept, 0.5)[0]
        for r, Sr, llr, phir in ((est, S, ll, phi), (fix, S * (phi / 0.5), ll5, 0.5)):
            errs = {"coef": rel(r["coef"][k].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][k].cpu().numpy(), Sr),
                    "Sig_invMcoef": rel(r["Sig_invMcoef"][k].cpu().numpy(), Sr @ b), "ll": abs(r["loglik"][k] - llr) / abs(llr),
                    "phi": abs(r["dispersion"][k] - phir) / phir, "P": abs(r["pearson"][k] - P) / P, "Dev": abs(r["deviance"][k] - dev) / dev}
            worst = {key: max(v, worst.get(key, 0.0)) for key, v in errs.items()}
        assert fix["dispersion"][k] == 0.5
        # the dispersion is one scalar on the information: the block at 0.5 is twice the unit block
        unit = _fit(eng, X[sl], y[sl], ok, [0, offs[k + 1] - offs[k]], intercept, power=power, dispersion=1.0)
        assert rel(fix["Sig_inv"][k].cpu().numpy(), 2.0 * unit["Sig_inv"][0].cpu().numpy()) <= 1e-13
    print("tweedie fit p=%d (%d evaluations): %s" % (p, max(est["n_iter"]), " ".join("%s %.1e" % kv for kv in worst.items())))
    assert all(v <= 1e-10 for v in worst.values()), worst


@pytest.mark.parametrize("power", [1.2, 1.8])
def test_fit_other_powers(eng, power):
    n, p = 3000, 7
    X, y, o = tr.data(47, n, p, True, True, power)
    r = _fit(eng, X, y, o, [0, 1300, n], True, power=power)
    assert r["status"] == [0, 0]
    for k, sl in enumerate((slice(0, 1300), slice(1300, n))):
        b, S, ll, phi, P, dev = tr.fit(X[sl], y[sl], power, o[sl], True)
        errs = {"coef": rel(r["coef"][k].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][k].cpu().numpy(), S),
                "ll": abs(r["loglik"][k] - ll) / abs(ll), "phi": abs(r["dispersion"][k] - phi) / phi, "Dev": abs(r["deviance"][k] - dev) / dev}
        print("tweedie fit power=%g partition %d: %s" % (power, k, " ".join("%s %.1e" % kv for kv in errs.items())))
        assert all(v <= 1e-10 for v in errs.values()), errs


def test_strided_partitions_equal_contiguous_copies(eng):
    import dlsa_amd
    n, p, K = 3001, 8, 5
    X, y, o = tr.data(70, n, p, True, True)
    e = np.exp(o)
    Xd, yd, ed = _dev(X, y, e)
    a = dlsa_amd.fit_tweedie_partitions(Xd, yd, partition_num=K, fit_intercept=True, exposure=ed, power=1.5)
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    Xc, yc, ec = _dev(X[perm], y[perm], e[perm])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    b = dlsa_amd.fit_tweedie_partitions(Xc, yc, part_offsets=offs, fit_intercept=True, exposure=ec, power=1.5)
    assert a.status == [0] * K and b.status == [0] * K
    assert a.names == ["intercept"] + ["x%d" % i for i in range(p)]
    assert rel(a.coef.cpu().numpy(), b.coef.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_inv.cpu().numpy(), b.Sig_inv.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_invMcoef.cpu().numpy(), b.Sig_invMcoef.cpu().numpy()) <= 1e-13
    assert rel(a.extra["dispersion"], b.extra["dispersion"]) <= 1e-13 and a.extra["df"] == b.extra["df"]


def test_fit_is_bit_reproducible(eng):
    import dlsa_amd
    X, y, o = tr.data(80, 20_000, 30, True, True)
    Xd, yd, od = _dev(X, y, o)
    a = dlsa_amd.fit_tweedie_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    b = dlsa_amd.fit_tweedie_partitions(Xd, yd, partition_num=3, fit_intercept=True, offset=od)
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik and a.extra == b.extra and all(v > 0 for v in a.extra["dispersion"])


def test_fit_empty_partition(eng):
    n, p = 3000, 4
    X, y, o = tr.data(50, n, p, True, True)
    offs = [0, 1000, 1000, n]
    r = _fit(eng, X, y, o, offs, True)
    assert r["status"] == [0, 4, 0] and r["rc"] == 0
    assert not r["Sig_inv"][1].any() and not r["coef"][1].any() and not r["Sig_invMcoef"][1].any()
    assert r["loglik"][1] == 0.0 and r["dispersion"][1] == 0.0 and r["pearson"][1] == 0.0 and r["deviance"][1] == 0.0
    b, S = tr.fit(X[1000:], y[1000:], 1.5, o[1000:], True)[:2]
    assert rel(r["coef"][2].cpu().numpy(), b) <= 1e-10 and rel(r["Sig_inv"][2].cpu().numpy(), S) <= 1e-10


def test_partition_without_degrees_of_freedom(eng):
    from dlsa_amd import _lib
    n, p = 1000, 3
    X, y, o = tr.data(51, n, p, True, True)
    y[500:504] = [0.7, 1.9, 0.4, 2.6]                        # (positive: the four rows below can be fitted exactly)
    for rows1 in (4, 2):                                     # n = pe and n < pe
        offs = [0, 500, 500 + rows1, n]
        with pytest.raises(_lib.DlsaError) as ex:            # estimated dispersion: P / (n - pe) has no degrees of freedom
            _fit(eng, X, y, o, offs, True)
        assert ex.value.code == 1 and "partition 1" in str(ex.value) and "degrees of freedom" in str(ex.value)
    # fixed dispersion, n = pe: the four rows are fitted exactly (y = mu: D beta = log y - o)
    offs = [0, 500, 504, n]
    r = _fit(eng, X, y, o, offs, True, dispersion=0.5)
    assert r["status"] == [0, 0, 0] and r["df"][1] == 0
    sl = slice(500, 504)
    exact = np.linalg.solve(tr.design(X[sl], True), np.log(y[sl]) - o[sl])
    assert rel(r["coef"][1].cpu().numpy(), exact) <= 1e-9 and r["pearson"][1] <= 1e-18
    # fixed dispersion, n < pe: the information is singular, as the data say
    r = _fit(eng, X, y, o, [0, 500, 502, n], True, dispersion=0.5)
    print("two rows for four coefficients: status %d" % r["status"][1])
    assert r["status"][0] == 0 and r["status"][2] == 0 and r["status"][1] != 0 and r["rc"] != 0


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_invalid_responses_are_refused(eng, bad):
    import dlsa_amd
    from dlsa_amd import _lib
    X, y, o = tr.data(61, 1000, 3, True, True)
    y_bad = y.copy(); y_bad[700] = bad
    with pytest.raises(ValueError):
        dlsa_amd.fit_tweedie_partitions(*_dev(X, y_bad), fit_intercept=True)
    with pytest.raises(_lib.DlsaError) as ex:       # (the C ABI's own check, below the Python one)
        _fit(eng, X, y_bad, o, [0, 500, 1000], True)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    # the pass reports an invalid response as a NaN quasi-log-likelihood
    ll = eng.tweedie_pass(*_dev(X, y_bad, np.zeros(3)), 1.5)[2]
    assert math.isnan(float(ll.item()))


def test_non_finite_offset_is_refused(eng):
    from dlsa_amd import _lib
    X, y, o = tr.data(61, 1000, 3, True, True)
    for bad in (float("nan"), float("inf"), -float("inf")):
        o_bad = o.copy(); o_bad[3] = bad
        with pytest.raises(_lib.DlsaError) as ex:
            _fit(eng, X, y, o_bad, [0, 500, 1000], True)
        assert ex.value.code == 1 and "partition 0" in str(ex.value)


def test_all_zero_partition_is_refused(eng):
    import dlsa_amd
    from dlsa_amd import _lib
    X, y, o = tr.data(61, 1000, 3, True, True)
    y0 = y.copy(); y0[500:] = 0.0
    with pytest.raises(_lib.DlsaError) as ex:
        _fit(eng, X, y0, o, [0, 500, 1000], True)
    assert ex.value.code == 1 and "partition 1" in str(ex.value) and "no positive response" in str(ex.value)
    with pytest.raises(ValueError, match="no response is positive"):
        dlsa_amd.fit_tweedie_partitions(*_dev(X, np.zeros(1000)), fit_intercept=True)
    # zeros as such are data: the first partition alone fits
    assert _fit(eng, X, y0, o, [0, 500], True)["status"] == [0]


@pytest.mark.parametrize("power", [1.0, 2.0, 0.5, 2.5, float("nan")])
def test_power_outside_the_family_is_refused(eng, power):
    import ctypes
    from dlsa_amd import _lib
    X, y, o = tr.data(61, 200, 3, True, True)
    Xd, yd, bd = _dev(X, y, np.zeros(3))
    with pytest.raises(ValueError, match="power must lie strictly between 1 and 2"):
        eng.tweedie_pass(Xd, yd, bd, power)
    with pytest.raises(ValueError, match="power must lie strictly between 1 and 2"):
        _fit(eng, X, y, o, [0, 200], True, power=power)
    # the C ABI's own check, below the Python one
    lib = _lib.load()
    ws = torch.empty(lib.dlsa_tweedie_workspace_bytes(200, 3, 0, 1), dtype=torch.uint8, device="cuda")
    g = torch.empty(3, dtype=torch.float64, device="cuda")
    rc = lib.dlsa_tweedie_pass_f64(Xd.data_ptr(), 3, yd.data_ptr(), None, bd.data_ptr(), power, 1.0, 200, 3, 0, None, 0, g.data_ptr(), None,
                                   None, None, ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and "power" in _lib.last_error()
    first, rows = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(200)
    out = torch.empty(3 + 9 + 3, dtype=torch.float64, device="cuda")
    rc = lib.dlsa_tweedie_fit_f64(Xd.data_ptr(), 3, yd.data_ptr(), None, first, rows, 1, 1, 3, 0, power, 0.0, 1e-13, 100, out.data_ptr(),
                                  out[3:].data_ptr(), out[12:].data_ptr(), None, None, None, None, None, None, ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and "power" in _lib.last_error()


def test_collinear_column_is_not_spd(eng):
    """a column that is exactly dependent on the others -- here all zeros -- leaves an exactly zero pivot: NOT_SPD at the first
    evaluation.  (The solver declares NOT_SPD at a pivot <= 0.  A duplicated column leaves a last pivot of rounding noise of either
    sign, so whether it is caught depends on the data: over the seeds 60 .. 67 of this design the Tweedie fit caught 7 of 8, the Gamma
    fit 7 of 8 and the Poisson fit 8 of 8, the zero column 24 of 24.)"""
    X, y, _ = tr.data(60, 2000, 5, True, False)
    X = np.column_stack([X, np.zeros(2000)])                # singular information
    r = _fit(eng, X, y, None, [0, 2000], False)
    assert r["status"] == [2] and r["rc"] == 4


@pytest.mark.parametrize("max_iter", [1, 2])
def test_budget_stops_at_the_evaluated_iterate(eng, max_iter):
    n, p, power = 600, 3, 1.5
    X, y, o = tr.data(303, n, p, True, True)
    evals, bs, lls = nw.undamped(lambda b: tr.terms(X, y, b, power, o, True)[:3], tr.start(X, y, power, o, True), 1e-13)
    assert evals is not None and evals > max_iter + 1 and nw.monotone(lls[:max_iter + 1])       # no halving in the budget
    r = _fit(eng, X, y, o, [0, n], True, max_iter=max_iter)
    assert r["status"] == [1] and r["rc"] == 5 and r["n_iter"] == [max_iter + 1]
    # max_iter steps were taken; the last evaluation's step was not: coef is where H and the dispersion were evaluated
    coef = r["coef"][0]
    assert rel(coef.cpu().numpy(), bs[max_iter]) <= 1e-10
    _, _, Hr, _, Pr, devr = tr.terms(X, y, bs[max_iter], power, o, True)
    phi = Pr / (n - p - 1)
    assert abs(r["dispersion"][0] - phi) <= 1e-10 * phi and abs(r["pearson"][0] - Pr) <= 1e-10 * Pr
    assert abs(r["deviance"][0] - devr) <= 1e-10 * devr
    llr = tr.terms(X, y, bs[max_iter], power, o, True, phi)[0]
    assert abs(r["loglik"][0] - llr) <= 1e-10 * abs(llr)
    Xd, yd, od = _dev(X, y, o)
    H = eng.tweedie_pass(Xd, yd, coef, power, r["dispersion"][0], offset=od, fit_intercept=True)[0].cpu().numpy()
    assert rel(r["Sig_inv"][0].cpu().numpy(), H) <= 1e-12 and rel(H, Hr / phi) <= 1e-10
    assert rel(r["Sig_invMcoef"][0].cpu().numpy(), H @ coef.cpu().numpy()) <= 1e-12


@pytest.mark.parametrize("power,dispersion", tr.CALIBRATION)
def test_block_is_calibrated(eng, power, dispersion):
    """What the dispersion is for.  K = 40 partitions of 1500 rows, 5 features + intercept, offsets: Q = the sum over the partitions
    of (b_k - b*)' Sig_inv_k (b_k - b*) is chi-square with 240 degrees of freedom, so it lies in 240 +- 3 sqrt(480) = [174, 306].  A
    Sig_inv left unscaled is off by the dispersion: on the CPU reference with this seed Q is 229.5 at (1.8, 0.3) and 249.2 at (1.2, 2.0),
    unscaled 69.0 and 491.8 (test_tweedie_cpu.py asserts both).  The pooled Pearson dispersion has relative variance (2 + the
    excess kurtosis xi (2 xi - 1) phi mu^(xi - 2)) / 59760: a standard deviation below 0.9 % in both cases, so 4 % is more than four of
    them (the CPU reference gives 0.3001 and 1.9700)."""
    import dlsa_amd
    K, m = 40, 1500
    X, y, o = tr.calibration_case(power, dispersion, K, m)
    Xd, yd, od = _dev(X, y, o)
    mb = dlsa_amd.fit_tweedie_partitions(Xd, yd, part_offsets=[k * m for k in range(K + 1)], fit_intercept=True, offset=od, power=power)
    assert mb.status == [0] * K
    q = tr.calibration_q(mb.coef.cpu().numpy(), mb.Sig_inv.cpu().numpy())
    phi = dlsa_amd.combine_tweedie_dispersion(mb)
    print("calibration at (%g, %g): Q %.1f on 240 degrees of freedom, pooled dispersion %.4f" % (power, dispersion, q, phi))
    assert 174.0 <= q <= 306.0
    assert abs(phi - dispersion) <= 0.04 * dispersion


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K, power = 40_000, 10, 8, 1.5
    X, y, o = tr.data(90, n, p, True, True)
    Xd, yd, od = _dev(X, y, o)
    mb = dlsa_amd.fit_tweedie_partitions(Xd, yd, partition_num=K, fit_intercept=True, offset=od, power=power)
    assert mb.status == [0] * K
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [tr.block(X[k::K], y[k::K], power, o[k::K], True) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = dlsa_amd.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


def test_tweedie_model_frame_and_eval(eng):
    import pandas as pd
    import dlsa_amd
    power = 1.4
    df = dlsa_amd.simulate_tweedie(5000, 6, 1, power, 1.5, seed=7, exposure=True)
    assert list(df.columns) == ["partition_id", "y", "exposure"] + ["x%d" % i for i in range(6)]
    assert bool((df["y"] >= 0).all()) and 0.05 < float((df["y"] == 0).mean()) < 0.6
    part = df.drop(columns=["partition_id"])
    out = dlsa_amd.tweedie_model(part, "y", fit_intercept=True, exposure_name="exposure", power=power)
    names = ["intercept"] + ["x%d" % i for i in range(6)]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (7, 10)
    X = part[names[1:]].to_numpy()
    Xd, yd, ed = _dev(X, part["y"].to_numpy(), part["exposure"].to_numpy())
    mb = dlsa_amd.fit_tweedie_partitions(Xd, yd, fit_intercept=True, exposure=ed, power=power)
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out["Sig_invMcoef"].to_numpy(), mb.Sig_invMcoef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    phi = out.attrs["dispersion"]
    assert out.attrs["power"] == power and phi == mb.extra["dispersion"][0] and 1.2 < phi < 1.8
    o = np.log(part["exposure"].to_numpy())
    b, S, ll, phir = tr.fit(X, part["y"].to_numpy(), power, o, True)[:4]
    assert rel(out["coef"].to_numpy(), b) <= 1e-10 and rel(out[names].to_numpy(), S) <= 1e-10 and abs(phi - phir) <= 1e-10 * phir
    # eval: the quasi-log-likelihood of each estimator column at the fit's dispersion, shaped like poisson_model_eval
    par = pd.DataFrame({"mle": mb.coef[0].cpu().numpy(), "ref": b, "zero": np.zeros(7)})
    ev = dlsa_amd.tweedie_model_eval(part, "y", par, power, phi, fit_intercept=True, exposure_name="exposure")
    assert list(ev.columns) == ["mle", "ref", "zero"] and ev.shape == (1, 3)
    assert abs(ev["mle"][0] - mb.loglik[0]) <= 1e-13 * abs(mb.loglik[0])
    refs = [tr.terms(X, part["y"].to_numpy(), par[c].to_numpy(), power, o, True, phi)[0] for c in par.columns]
    assert rel(ev.to_numpy()[0], refs) <= 1e-12
    with pytest.raises(ValueError):
        dlsa_amd.tweedie_model(part, "y", fit_intercept=True, exposure_name="exposure", power=power, dispersion=0.0)
    with pytest.raises(ValueError):
        dlsa_amd.tweedie_model(part, "y", fit_intercept=True, exposure_name="exposure", power=2.0)
    fixed = dlsa_amd.tweedie_model(part, "y", fit_intercept=True, exposure_name="exposure", power=power, dispersion=0.5)
    assert fixed.attrs["dispersion"] == 0.5 and np.array_equal(fixed["coef"].to_numpy(), out["coef"].to_numpy())
    # the default power is 1.5
    assert dlsa_amd.tweedie_model(part, "y", fit_intercept=True, exposure_name="exposure").attrs["power"] == 1.5


def test_tweedie_model_dummy_factor_and_missing_level(eng):
    import pandas as pd
    import dlsa_amd
    rng = np.random.default_rng(2)
    n, power = 4000, 1.5
    df = pd.DataFrame({"partition_id": np.zeros(n), "y": 0.0, "dist": rng.normal(5.0, 2.0, n),
                       "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2])})
    df["y"] = tr.draw(rng, np.exp(0.1 * (df["dist"].to_numpy() - 5) + 0.4 * (df["carrier"] == "BB").to_numpy()), power, 1.0)
    assert 0.05 < float((df["y"] == 0).mean()) < 0.5
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"]}, "factor_dropped": {"carrier": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"]}}
    baseline = ["carrier_AA"]
    want = ["par_id", "coef", "Sig_invMcoef", "intercept", "dist", "carrier_BB", "carrier_CC"]
    out = dlsa_amd.tweedie_model(df, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert list(out.columns) == want
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC"]).astype(float)
    b, S, _, phi = tr.fit(Xo, df["y"].to_numpy(), power, None, True)[:4]
    assert rel(out["coef"], b) <= 1e-10 and rel(out.iloc[:, 3:].to_numpy(), S) <= 1e-10
    assert abs(out.attrs["dispersion"] - phi) <= 1e-10 * phi and out.attrs["power"] == 1.5
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = dlsa_amd.tweedie_model(sub, "y", fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert any("missing in this data chunk" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (4, 7) and float(np.abs(zero.to_numpy()).max()) == 0.0
    assert zero.attrs["dispersion"] == 0.0
