"""GPU: the ordinal (proportional-odds) map step (csrc/ordinal.hip, include/dlsa_hip_ordinal.h) against the numpy reference
(tests/ordinal_reference.py): the pass at a fixed theta (log-likelihood, score, observed information, weights) at every shape at
which the row pass takes another path -- odd and even p, the column-chunk boundaries, the in-pass borders, the budget boundary
C NC = 16 and the masked X'v route beyond it --, fewer rows than a batch, a padded pitch, each nullable output, the extreme case,
unordered cutpoints and bad responses; the per-partition fit, C = 2 against the logistic fit, strided and empty partitions, the
refusals; the frame-level ordinal_model, the end-to-end DLSA combine with unpenalised cutpoints and the calibration of the block.

The tolerances are the project's parity bars (1e-12 relative l-inf for a pass, 1e-10 for a fit).  On the CPU the fp64 reference
agrees with a longdouble run of itself to <= 1.8e-15 on these inputs and to 8.7e-15 (the weights; 3.4e-16 for g and H) in the
extreme case (test_ordinal_cpu.py asserts 1e-13), so the extreme case is held to the same 1e-12 against the longdouble run."""
import ctypes
import functools

import numpy as np
import pytest

import lars_unpenalized_reference as ur
import ordinal_reference as orf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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


@functools.lru_cache(maxsize=None)
def _pass_case(n, p, C):
    X, y = orf.data(10 + p, n, p, C)
    theta = orf.away_from_optimum(p, C)
    return X, y, theta, orf.terms(X, y, theta, C)


def _check_pass(eng, X, y, theta, C, ref, tol=1e-12, Xd=None, what="pass"):
    """Xd: the device tensor to pass for X (a view with its own pitch); default a contiguous copy"""
    Xc, yd, td = _dev(X, y, theta)
    H, g, ll, w = eng.ordinal_pass(Xc if Xd is None else Xd, yd, td, C, want_w=True)
    llr, gr_, Hr, wr = [np.asarray(v, float) for v in ref]
    Hn = H.cpu().numpy()
    errs = {"ll": abs(float(ll.item()) - llr) / abs(llr), "g": rel(g.cpu().numpy(), gr_), "H": rel(Hn, Hr), "w": rel(w.cpu().numpy(), wr)}
    print("ordinal %s n=%d p=%d C=%d: %s" % (what, X.shape[0], X.shape[1], C, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(np.isfinite(v) and v <= tol for v in errs.values()), errs
    assert np.array_equal(Hn, Hn.T)
    return H, g, ll, w


@pytest.mark.parametrize("n,p,C", orf.PASS_SHAPES)
def test_pass_matches_reference(eng, n, p, C):
    """odd and even p (the scalar and the vector loads), p = 127 / 128 / 129 and 257 (the chunk counts 1, 2 and 4), the in-pass borders
    (C NC <= 16, with (4001, 130, 8) on the boundary) and the masked X'v route ((3001, 257, 5) and (2001, 600, 3)); H bitwise
    symmetric, g and loglik bit-identical over two runs"""
    X, y, theta, ref = _pass_case(n, p, C)
    assert set(range(C)) <= set(y.astype(int))
    H, g, ll, w = _check_pass(eng, X, y, theta, C, ref)
    Xd, yd, td = _dev(X, y, theta)
    H2, g2, ll2, w2 = eng.ordinal_pass(Xd, yd, td, C, want_w=True)
    assert torch.equal(g, g2) and torch.equal(ll, ll2) and torch.equal(w, w2) and torch.equal(H, H2)


@pytest.mark.parametrize("p,C", [(5, 3), (5, 8), (130, 8), (257, 5)])
def test_pass_fewer_rows_than_one_batch(eng, p, C):
    """n = C rows: at NC = 1 every prefetch of the second register set is a clamped re-read of the last row"""
    X, y = orf.data(900 + p, C, p, C)
    theta = orf.away_from_optimum(p, C)
    _check_pass(eng, X, y, theta, C, orf.terms(X, y, theta, C), what="short pass")


# Edge shapes of the shared row-pass skeleton (csrc/row_pass.h) that no list above reaches: n = 1, 7 and 9 are a batch of 8 that is
# all clamp but one row, one with a single clamped row, and a second batch with one row; n = 1003 at p = 3 is several batches per
# wave on the NC = 1 two-set loop with a last prefetched batch past the end, and a pair that straddles p; n = 300 001 at p = 3 meets
# the cap on the block count (37 501 batches of 8 ask for 2344 blocks of 16); p = 1025 is NC = 16 on the scalar loads; (257, 8) is
# the masked route at the most classes (C NC = 32 > 16) beside the in-pass borders of the others.
SKELETON_EDGES = [(1, 5, 3), (7, 5, 3), (9, 5, 3), (9, 130, 8), (1003, 3, 4), (300001, 3, 3), (67, 1025, 2), (1003, 257, 8)]


@pytest.mark.parametrize("n,p,C", SKELETON_EDGES)
def test_pass_edge_shapes_of_the_row_pass_skeleton(eng, n, p, C):
    X, y = orf.data(700 + p + n % 1000, n, p, C)
    theta = orf.away_from_optimum(p, C)
    _check_pass(eng, X, y, theta, C, orf.terms(X, y, theta, C), what="edge pass")


@pytest.mark.parametrize("p,C,pad", [(5, 3, 3), (130, 8, 2), (257, 5, 3)])
def test_pass_on_a_padded_pitch(eng, p, C, pad):
    """columns 1 .. p of a buffer with p + pad columns, passed as a view: an odd pitch, or an even one with the base 8 bytes off a
    16-byte boundary -- the scalar loads either way"""
    n = 1003
    X, y = orf.data(950 + p, n, p, C)
    theta = orf.away_from_optimum(p, C)
    big = torch.zeros((n, p + pad), dtype=torch.float64, device="cuda")
    Xd = big[:, 1:1 + p]
    Xd.copy_(torch.from_numpy(X))
    assert Xd.stride(0) == p + pad and Xd.stride(1) == 1
    _check_pass(eng, X, y, theta, C, orf.terms(X, y, theta, C), Xd=Xd, what="padded pass")


@pytest.mark.parametrize("n,p,C", [(6001, 5, 3), (3001, 257, 5)])
def test_each_nullable_output_left_out_in_turn(eng, n, p, C):
    """straight on the C ABI: H, g, loglik and w_out each null in turn; the others keep their bits"""
    from dlsa_amd import _lib
    lib = _lib.load()
    X, y, theta, _ = _pass_case(n, p, C)
    Xd, yd, td = _dev(X, y, theta)
    d = C - 1 + p
    ws = torch.empty(lib.dlsa_ordinal_workspace_bytes(n, p, C, 1), dtype=torch.uint8, device="cuda")

    def run(skip):
        out = {"H": torch.full((d, d), 7.0, dtype=torch.float64, device="cuda"), "g": torch.full((d,), 7.0, dtype=torch.float64, device="cuda"),
               "ll": torch.full((1,), 7.0, dtype=torch.float64, device="cuda"), "w": torch.full((n,), 7.0, dtype=torch.float64, device="cuda")}
        ptr = {k: (None if k == skip else v.data_ptr()) for k, v in out.items()}
        rc = lib.dlsa_ordinal_pass_f64(Xd.data_ptr(), p, yd.data_ptr(), td.data_ptr(), C, n, p, ptr["H"], d, ptr["g"], ptr["ll"], ptr["w"],
                                       ws.data_ptr(), ws.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        return out
    full = run(None)
    for skip in ("H", "g", "ll", "w"):
        part = run(skip)
        for k in full:
            if k == skip:
                assert bool((part[k] == 7.0).all()), (skip, k)
            else:
                assert torch.equal(part[k], full[k]), (skip, k)


def test_pass_extreme_case(eng):
    """|u| and |l| up to 600, one pair of cutpoints 1e-6 apart: against the longdouble run of the reference.  On the CPU the fp64
    reference differs from it by (ll, g, H, w) = (1.9e-16, 3.4e-16, 3.3e-16, 8.7e-15)."""
    X, y, theta = orf.extreme_case()
    ref = orf.terms(X, y, theta, orf.EXTREME_CLASSES, np.longdouble)
    assert all(np.isfinite(np.asarray(v, float)).all() for v in ref)
    _check_pass(eng, X, y, theta, orf.EXTREME_CLASSES, ref, what="extreme pass")


@pytest.mark.parametrize("n,p,C", [(6001, 5, 8), (3001, 257, 5)])
def test_unordered_cutpoints_give_nan_and_no_fault(eng, n, p, C):
    X, y, _, _ = _pass_case(n, p, C)
    Xd, yd, td = _dev(X, y, orf.unordered(p, C))
    H, g, ll, w = eng.ordinal_pass(Xd, yd, td, C, want_w=True)          # (rc 0: the wrapper raises otherwise)
    torch.cuda.synchronize()
    assert np.isnan(ll.item())
    td = td.clone()
    td[0] = float("nan")
    assert np.isnan(eng.ordinal_pass(Xd, yd, td, C, want_H=False)[2].item())


@pytest.mark.parametrize("bad", [float("nan"), 7.5])
def test_a_bad_response_gives_nan_loglik_in_the_pass(eng, bad):
    n, p, C = 6001, 5, 8
    X, y, theta, _ = _pass_case(n, p, C)
    y = y.copy()
    y[[250, 3100]] = bad
    Xd, yd, td = _dev(X, y, theta)
    H, g, ll, _ = eng.ordinal_pass(Xd, yd, td, C)
    torch.cuda.synchronize()
    assert np.isnan(ll.item())


# ---- the fit --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit_case(n, p, C):
    X, y = orf.data(40 + p, n, p, C)
    return X, y, orf.fit(X, y, C)


def _fit(eng, X, y, offs, C, **kw):
    Xd, yd = _dev(X, y)
    return eng.ordinal_fit_ex(Xd, yd, offs[:-1], [offs[k + 1] - offs[k] for k in range(len(offs) - 1)], classes=C, **kw)


@pytest.mark.parametrize("n,p,C", orf.FIT_SHAPES)
def test_fit_matches_reference(eng, n, p, C):
    """the evaluations: the stopping rule compares the NEXT step with tol; at convergence that step is rounding noise of the solve, so
    either side of the comparison may see it land on the other side of 1e-13 once -- the counts agree to one evaluation"""
    X, y, (b, S, ll, n_iter) = _fit_case(n, p, C)
    assert set(range(C)) <= set(y.astype(int)) and 5 <= n_iter <= 6
    r = _fit(eng, X, y, [0, n], C)
    assert r["status"] == [0] and r["rc"] == 0
    errs = {"coef": rel(r["coef"][0].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][0].cpu().numpy(), S),
            "Sig_invMcoef": rel(r["Sig_invMcoef"][0].cpu().numpy(), S @ b), "ll": abs(r["loglik"][0] - ll) / abs(ll)}
    print("ordinal fit n=%d p=%d C=%d: %d evaluations (reference %d) %s" % (n, p, C, r["n_iter"][0], n_iter,
                                                                            " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-10 for v in errs.values()), errs
    assert abs(r["n_iter"][0] - n_iter) <= 1
    Sn = r["Sig_inv"][0].cpu().numpy()
    assert np.array_equal(Sn, Sn.T)


@pytest.mark.parametrize("p", [7, 50])
def test_two_classes_equal_the_logistic_fit(eng, p):
    """C = 2 is the logistic model with theta = [-intercept | beta]: coef, Sig_inv (rows and columns of the cutpoint change sign)
    and Sig_inv coef after the sign map"""
    n, K = 3001, 3
    X, y = orf.data(90 + p, n, p, 2)
    Xd, yd = _dev(X, y)
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    a = eng.ordinal_fit_ex(Xd, yd, first, rows, row_step=K, classes=2)
    b = eng.irls_fit_ex(Xd, yd, first, rows, row_step=K, fit_intercept=True)
    assert a["status"] == [0] * K and b["status"] == [0] * K
    sgn = np.ones(p + 1)
    sgn[0] = -1.0
    got = {"coef": a["coef"].cpu().numpy() * sgn, "Sig_invMcoef": a["Sig_invMcoef"].cpu().numpy() * sgn,
           "Sig_inv": a["Sig_inv"].cpu().numpy() * sgn[None, :, None] * sgn[None, None, :]}
    errs = {key: rel(got[key], b[key].cpu().numpy()) for key in got}
    errs["ll"] = rel(a["loglik"], b["loglik"])
    print("ordinal C = 2 against irls_fit_ex p=%d: %s" % (p, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-10 for v in errs.values()), errs


@pytest.mark.parametrize("p,C", [(10, 4), (258, 5)])
def test_strided_partitions_equal_gathered_ones_bit_for_bit(eng, p, C):
    """K = 4 strided partitions, read in place with the pitch 4 p, against the contiguous fits of the gathered rows: the same bits.
    p is even, so both layouts have an even pitch and 16-byte aligned rows and the Gram dispatch stages them alike (an odd pitch takes
    another staging and other last bits, as the frame-level test of the multinomial family notes); the in-pass borders (10, 4) and the
    masked X'v route (258, 5)."""
    n, K = 4 * 1203 + 3, 4                               # 1204, 1204, 1204, 1203 rows
    X, y = orf.data(55 + p, n, p, C)
    Xd, yd = _dev(X, y)
    rows = [len(range(k, n, K)) for k in range(K)]
    assert len(set(rows)) > 1
    s = eng.ordinal_fit_ex(Xd, yd, list(range(K)), rows, row_step=K, classes=C)
    assert s["status"] == [0] * K
    for k in range(K):
        c = _fit(eng, X[k::K], y[k::K], [0, rows[k]], C)
        assert c["status"] == [0] and c["n_iter"][0] == s["n_iter"][k] and c["loglik"][0] == s["loglik"][k]
        for key in ("coef", "Sig_inv", "Sig_invMcoef"):
            assert torch.equal(s[key][k], c[key][0]), (k, key)


def test_empty_partition_is_the_zero_block(eng):
    X, y = orf.data(57, 600, 5, 3)
    r = _fit(eng, X, y, [0, 300, 300, 600], 3)
    assert r["status"] == [0, 4, 0] and r["rc"] == 0 and r["n_iter"][1] == 0 and r["loglik"][1] == 0.0
    for key in ("coef", "Sig_inv", "Sig_invMcoef"):
        assert float(r[key][1].abs().max()) == 0.0
    one = _fit(eng, X[300:], y[300:], [0, 300], 3)
    assert torch.equal(one["coef"][0], r["coef"][2])


def test_a_constant_column_is_not_spd(eng):
    """the cutpoints are the intercepts: an all-zero column leaves an exactly zero pivot at the first evaluation"""
    X, y = orf.data(60, 2000, 5, 3)
    X = np.column_stack([X, np.zeros(2000)])
    r = _fit(eng, X, y, [0, 2000], 3)
    assert r["status"] == [2] and r["rc"] == 4


def _raw_fit(lib, Xd, yd, offs, p, C, poison=7.0):
    K, d = len(offs) - 1, C - 1 + p
    first = (ctypes.c_int64 * K)(*offs[:-1])
    rows = (ctypes.c_int64 * K)(*[offs[k + 1] - offs[k] for k in range(K)])
    out = [torch.full(shape, poison, dtype=torch.float64, device="cuda") for shape in ((K, d), (K, d, d), (K, d))]
    host = ((ctypes.c_int * K)(*([-9] * K)), (ctypes.c_int * K)(*([-9] * K)), (ctypes.c_double * K)(*([poison] * K)))
    ws = torch.empty(lib.dlsa_ordinal_workspace_bytes(max(rows), p, C, 1), dtype=torch.uint8, device="cuda")
    rc = lib.dlsa_ordinal_fit_f64(Xd.data_ptr(), p, yd.data_ptr(), first, rows, 1, K, p, C, 1e-13, 100, out[0].data_ptr(), out[1].data_ptr(),
                                  out[2].data_ptr(), *host, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    untouched = all(bool((o == poison).all()) for o in out) and list(host[0]) == [-9] * K and list(host[1]) == [-9] * K \
        and list(host[2]) == [poison] * K
    return rc, untouched


@pytest.mark.parametrize("bad", [1.5, -1.0, 3.0, float("nan")])
def test_a_response_that_is_no_class_code_is_refused(eng, bad):
    from dlsa_amd import _lib
    C = 3
    X, y = orf.data(62, 400, 4, C)
    y[[250, 310]] = bad
    with pytest.raises(_lib.DlsaError) as ex:
        _fit(eng, X, y, [0, 200, 400], C)
    assert ex.value.code == 1 and "partition 1 has 2 rows whose response is not a class code 0 .. 2" in str(ex.value)
    Xd, yd = _dev(X, y)
    rc, untouched = _raw_fit(_lib.load(), Xd, yd, [0, 200, 400], 4, C)
    assert rc == 1 and untouched
    assert _fit(eng, X, y, [0, 200], C)["status"] == [0]              # the first partition alone fits


def test_a_partition_that_lacks_a_class_is_refused(eng):
    from dlsa_amd import _lib
    C = 4
    X, y = orf.data(63, 900, 4, C)
    y[300:600][y[300:600] == 2] = 1.0
    with pytest.raises(_lib.DlsaError) as ex:
        _fit(eng, X, y, [0, 300, 600, 900], C)
    assert ex.value.code == 1 and "partition 1 has no row of class 2" in str(ex.value)
    Xd, yd = _dev(X, y)
    rc, untouched = _raw_fit(_lib.load(), Xd, yd, [0, 300, 600, 900], 4, C)
    assert rc == 1 and untouched
    assert _fit(eng, X, y, [0, 300], C)["status"] == [0]


# ---- frames, end to end, calibration ---------------------------------------------------------------------------------------------------
def test_ordinal_model_frame_and_eval(eng):
    import pandas as pd
    import dlsa_amd
    labels = ["low", "medium", "high", "severe"]
    df = dlsa_amd.simulate_ordinal(4000, 6, 1, 4, seed=7)
    assert list(df.columns) == ["partition_id", "y"] + ["x%d" % i for i in range(6)] and set(df["y"]) == {0.0, 1.0, 2.0, 3.0}
    codes = df["y"].to_numpy()
    part = df.drop(columns=["partition_id"]).assign(y=[labels[int(c)] for c in codes])
    out = dlsa_amd.ordinal_model(part, "y", labels)
    xs = ["x%d" % i for i in range(6)]
    names = ["intercept:1", "intercept:2", "intercept:3"] + xs
    assert dlsa_amd.ordinal_column_names(xs, 4) == names and dlsa_amd.intercept_columns(names) == [0, 1, 2]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (9, 12)
    X = part[xs].to_numpy()
    Xd, yd = _dev(X, codes)
    mb = dlsa_amd.fit_ordinal_partitions(Xd, yd, 4)
    assert mb.names == names
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    b, S, ll, _ = orf.fit(X, codes, 4)
    assert rel(out["coef"].to_numpy(), b) <= 1e-10 and rel(out[names].to_numpy(), S) <= 1e-10
    assert rel(out["Sig_invMcoef"].to_numpy(), S @ b) <= 1e-10
    par = pd.DataFrame({"mle": mb.coef[0].cpu().numpy(), "away": orf.away_from_optimum(6, 4)})
    ev = dlsa_amd.ordinal_model_eval(part, "y", par, labels)
    assert list(ev.columns) == ["mle", "away"] and ev.shape == (1, 2)
    refs = [orf.terms(X, codes, par[c].to_numpy(), 4)[0] for c in par.columns]
    assert rel(ev.to_numpy()[0], refs) <= 1e-12
    with pytest.raises(ValueError, match="not among classes"):
        dlsa_amd.ordinal_model(part, "y", labels[:2])


def test_end_to_end_dlsa_with_unpenalised_cutpoints(eng):
    """fit_ordinal_partitions -> dlsa_mapred -> dlsa(unpenalized="intercepts") against the oracle on the reference's blocks, at the
    bars of the multinomial end-to-end test (1e-10 for the combine, 1e-8 for the path); the J cutpoints are never shrunk"""
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K, C = 24_000, 6, 8, 4
    X, y = orf.data(90, n, p, C)
    Xd, yd = _dev(X, y)
    mb = dlsa_amd.fit_ordinal_partitions(Xd, yd, C, partition_num=K)
    assert mb.status == [0] * K
    names = ["intercept:%d" % j for j in range(1, C)] + ["x%d" % i for i in range(p)]
    assert mb.names == names
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [orf.block(X[k::K], y[k::K], C) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    # the path of the combined problem with the J cutpoints unpenalised: the oracle's path of the host-reduced problem
    U = dlsa_amd.intercept_columns(names)
    assert U == list(range(C - 1))
    res = dlsa_amd.dlsa(out.iloc[:, 2:], out["beta_byOLS"], n, unpenalized="intercepts")
    assert list(res.columns) == ["beta_byAIC", "beta_byBIC"] and res.shape == (C - 1 + p, 2)
    r = ur.path(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), U, n, "lar")
    by_aic, by_bic = r["theta"][int(np.argmin(r["AIC"]))], r["theta"][int(np.argmin(r["BIC"]))]
    ea, eb = rel(res["beta_byAIC"].to_numpy(), by_aic), rel(res["beta_byBIC"].to_numpy(), by_bic)
    bic = res["beta_byBIC"].to_numpy()
    pen = np.delete(bic, U)
    print("ordinal end to end: OLS, one-shot and Sigma within 1e-10; AIC point %.1e BIC point %.1e; %d of %d penalised coefficients "
          "are zero at the BIC point" % (ea, eb, int((pen == 0).sum()), pen.size))
    assert ea <= 1e-8 and eb <= 1e-8
    assert np.all(bic[U] != 0) and np.all(res["beta_byAIC"].to_numpy()[U] != 0) and np.any(pen == 0)


def test_block_is_calibrated(eng):
    """24 strided partitions of 1500 rows, p = 4, C = 4 (d = 7): Q = sum_k (theta_k - theta*)' Sig_inv_k (theta_k - theta*) is
    chi-square on 168 degrees of freedom, so it lies in 168 +- 4 sqrt(336) = 168 +- 73.3.  The reference alone gives 169.59 for this
    seed (test_ordinal_cpu.py asserts 168 +- 36.7)."""
    import dlsa_amd
    X, y = orf.calibration_case()
    Xd, yd = _dev(X, y)
    mb = dlsa_amd.fit_ordinal_partitions(Xd, yd, orf.CALIBRATION_CLASSES, partition_num=orf.CALIBRATION_K)
    assert mb.status == [0] * orf.CALIBRATION_K
    q = orf.calibration_q(mb.coef.cpu().numpy(), mb.Sig_inv.cpu().numpy())
    print("ordinal calibration: Q %.2f on 168 degrees of freedom (reference %.2f)" % (q, orf.CALIBRATION_Q_REFERENCE))
    assert abs(q - 168.0) <= 73.3
