"""GPU: the multinomial logistic (softmax) map step (csrc/multinomial.hip) against the numpy reference
(tests/multinomial_reference.py): the pass at a fixed theta (log-likelihood, score, information, probabilities) at every class the
row pass and the Gram dispatch distinguish, the sub-block output of the Gram kernels at their row floors, the per-partition fit,
C = 2 against the logistic fit, strided partitions, reproducibility, degenerate inputs and refusals, the calibration of the block,
the end-to-end DLSA combine and the frame-level multinomial_model.

The tolerances are the project's parity bars (1e-12 relative l-inf for a pass, 1e-10 for a fit): on the CPU the fp64 reference
agrees with a longdouble run of itself to <= 1.5e-15 on these inputs and to <= 2.6e-15 in the eta-span case
(test_multinomial_cpu.py asserts 1e-13)."""
import ctypes
import functools
import re
import warnings
from pathlib import Path

import numpy as np
import pytest

import multinomial_reference as mr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CSRC = Path(__file__).resolve().parents[1] / "dlsa_amd" / "csrc"


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


def _check_pass(eng, X, y, theta, C, intercept, tol=1e-12, Xd=None, ref=None):
    """Xd: the device tensor to pass for X (a view with its own pitch / alignment); default a contiguous copy"""
    Xc, yd, td = _dev(X, y, theta)
    H, g, ll, P = eng.multinomial_pass(Xc if Xd is None else Xd, yd, td, C, fit_intercept=intercept, want_prob=True)
    llr, gr_, Hr, Pr = mr.terms(X, y, theta, C, intercept) if ref is None else ref
    Hn = H.cpu().numpy()
    errs = {"ll": abs(float(ll.item()) - llr) / abs(llr), "g": rel(g.cpu().numpy(), gr_), "H": rel(Hn, Hr), "P": rel(P.cpu().numpy(), Pr)}
    print("multinomial pass n=%d p=%d C=%d icpt=%d: %s" % (X.shape[0], X.shape[1], C, intercept, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(np.isfinite(v) and v <= tol for v in errs.values()), errs
    assert np.array_equal(Hn, Hn.T)
    return errs


PASS_CASES = [(p, C) for C in (2, 3, 5, 8) for p in (1, 7, 50, 100, 128, 129, 130, 256, 257, 260) if (C - 1) * (p + 1) <= 2048]
PASS_CASES += [(p, C) for C in (2, 3) for p in (500, 600)] + [(1030, 2)]          # (1030: 9 chunks, NC = 16)


@pytest.mark.parametrize("p,C", PASS_CASES)
@pytest.mark.parametrize("intercept", [False, True])
def test_pass_matches_reference(eng, p, C, intercept):
    n = 3 * p + 37
    X, y = mr.data(10 + p, n, p, C, intercept)
    assert set(range(C)) <= set(y.astype(int))
    _check_pass(eng, X, y, mr.away_from_optimum((C - 1) * (p + intercept)), C, intercept)


# fewer rows than one batch of 8 (or a single row): at NC = 1 every prefetch of the second register set is a clamped re-read of row
# n - 1; p = 1030 is NC = 16 with one row per wave.  Classes without a row are legal in a pass (n = 1 and n = 5 lack some at C = 8).
@pytest.mark.parametrize("n", [1, 5, 9])
@pytest.mark.parametrize("p,C", [(3, 3), (3, 8), (130, 4), (1030, 2)])
@pytest.mark.parametrize("intercept", [False, True])
def test_pass_short_and_wide_shapes(eng, n, p, C, intercept):
    X, y = mr.data(900 + p + n, n, p, C, intercept)
    _check_pass(eng, X, y, mr.away_from_optimum((C - 1) * (p + intercept)), C, intercept)


# Edge shapes of the shared row-pass skeleton (csrc/row_pass.h) that neither list above reaches: n = 7 is one batch of 8 with one
# clamped row; n = 1003 at p = 3 is several batches per wave on the NC = 1 two-set loop with a last prefetched batch past the end;
# n = 300 001 at p = 3 meets the cap on the block count (37 501 batches of 8 ask for 2344 blocks of 16); p = 2 is the 16-byte loads at
# the smallest width; p = 513 at C = 4 is NC = 8 (two rows per batch) with the most classes that have it, p = 1025 at C = 2 is NC = 16
# on the scalar loads.
SKELETON_EDGES = [(7, 3, 3), (7, 130, 4), (1003, 3, 3), (300001, 3, 3), (67, 2, 5), (67, 513, 4), (67, 1025, 2)]


@pytest.mark.parametrize("n,p,C", SKELETON_EDGES)
@pytest.mark.parametrize("intercept", [False, True])
def test_pass_edge_shapes_of_the_row_pass_skeleton(eng, n, p, C, intercept):
    X, y = mr.data(700 + p + n % 1000, n, p, C, intercept)
    _check_pass(eng, X, y, mr.away_from_optimum((C - 1) * (p + intercept)), C, intercept)


def test_pass_with_an_absent_class_is_legal(eng):
    X, y = mr.data(31, 200, 7, 4, True)
    y[y == 2] = 0.0
    assert 2 not in set(y.astype(int))
    _check_pass(eng, X, y, mr.away_from_optimum(3 * 8), 4, True)


@pytest.mark.parametrize("p,C", [(8, 3), (130, 5), (1030, 2)])
@pytest.mark.parametrize("pad", [3, 2])
@pytest.mark.parametrize("intercept", [False, True])
def test_pass_even_width_on_the_scalar_loads(eng, p, C, pad, intercept):
    """an even p takes the scalar loads only through the rows' pitch or base: columns 1 .. p of a buffer with p + 3 columns (an odd
    pitch) and of one with p + 2 (an even pitch, the base 8 bytes off a 16-byte boundary), passed as views, without a copy"""
    n = 67
    X, y = mr.data(900 + p + n, n, p, C, intercept)
    big = torch.zeros((n, p + pad), dtype=torch.float64, device="cuda")
    Xd = big[:, 1:1 + p]
    Xd.copy_(torch.from_numpy(X))
    assert Xd.stride(0) == p + pad and Xd.stride(1) == 1
    if pad == 2:
        assert Xd.data_ptr() % 16 == 8
    _check_pass(eng, X, y, mr.away_from_optimum((C - 1) * (p + intercept)), C, intercept, Xd=Xd)


def test_pass_eta_spanning_600(eng):
    X, y, theta = mr.eta_span_case()
    C = mr.ETA_SPAN_CLASSES
    ref = mr.terms(X, y, theta, C, True)
    eta = mr.design(X, True) @ theta.reshape(C - 1, -1).T
    assert np.ptp(np.concatenate([np.zeros((len(X), 1)), eta], 1), axis=1).max() > 590 and all(np.isfinite(v).all() for v in ref)
    _check_pass(eng, X, y, theta, C, True, ref=ref)


# ---- the sub-block output of the Gram kernels at their row floors ------------------------------------------------------------------
def _source_constant(file, name):
    m = re.search(r"constexpr\s+int64_t\s+%s\s*=\s*(\d+)\s*;" % name, (CSRC / file).read_text())
    assert m, (file, name)
    return int(m.group(1))


FLOORS = [("narrow", 100, "gram_narrow.hip", "NARROW_MIN_ROWS", "gram_narrow_kernel<true,"),
          ("plan", 260, "gram_plan.h", "PLAN_MIN_ROWS", "gram_plan_kernel<true,"),
          ("cyclic", 500, "gram_cyclic.hip", "CYC_MIN_ROWS", "gram_cyclic_kernel<true,")]


@pytest.mark.parametrize("kind,p,file,constant,kernel", FLOORS)
def test_sub_blocks_at_the_gram_kernels_row_floors(eng, kind, p, file, constant, kernel):
    """C = 3 with an intercept: pe is odd, so the blocks (1, 1), (1, 2) and (2, 2) start at H + ldh + 1, H + ldh + pe + 1 and
    H + (pe + 1) ldh + pe + 1 -- the off-diagonal one on an 8-byte boundary only.  n = the smallest the kernel class accepts.  The host
    reference is the three weighted products."""
    n, C = _source_constant(file, constant), 3
    rng = np.random.default_rng(7000 + p)
    X = rng.uniform(-0.5, 0.5, (n, p))
    y = rng.integers(0, C, n).astype(np.float64)
    theta = mr.away_from_optimum(2 * (p + 1))
    Xd, yd, td = _dev(X, y, theta)
    H, g, ll, P = eng.multinomial_pass(Xd, yd, td, C, fit_intercept=True, want_prob=True)
    name = eng.gram_last_kernel()[0]
    assert name.startswith(kernel), name
    Hn, Pn = H.cpu().numpy(), P.cpu().numpy()
    D = mr.design(X, True)
    pe = p + 1
    Hr = np.zeros((2 * pe, 2 * pe))
    for j, k in ((0, 0), (0, 1), (1, 1)):
        w = Pn[j] * ((1.0 if j == k else 0.0) - Pn[k])
        blk = (D * w[:, None]).T @ D
        Hr[j * pe:(j + 1) * pe, k * pe:(k + 1) * pe] = Hr[k * pe:(k + 1) * pe, j * pe:(j + 1) * pe] = (blk + blk.T) / 2
    B = theta.reshape(2, pe)
    full = np.concatenate([np.zeros((n, 1)), D @ B.T], 1)
    Pr = np.exp(full - np.logaddexp.reduce(full, axis=1)[:, None])[:, 1:].T
    errs = {"H": rel(Hn, Hr), "P": rel(Pn, Pr)}
    print("multinomial sub-blocks, %s floor n=%d p=%d (%s): %s" % (kind, n, p, name, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-12 for v in errs.values()), errs
    assert np.array_equal(Hn, Hn.T)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit_case(n, p, C, intercept):
    X, y = mr.data(40 + p, n, p, C, intercept)
    return X, y, mr.fit(X, y, C, bool(intercept))


def _fit(eng, X, y, offs, C, intercept, **kw):
    Xd, yd = _dev(X, y)
    return eng.multinomial_fit_ex(Xd, yd, offs[:-1], [offs[k + 1] - offs[k] for k in range(len(offs) - 1)], classes=C,
                                  fit_intercept=bool(intercept), **kw)


@pytest.mark.parametrize("n,p,C,intercept", mr.FIT_SHAPES)
def test_fit_matches_reference(eng, n, p, C, intercept):
    """the evaluations: the stopping rule compares the NEXT step with tol; at convergence that step is rounding noise of the solve
    (about 1e-16 times the condition number) after one of about its square root, so either side of the comparison may see it land on
    the other side of 1e-13 once -- the counts agree to one evaluation"""
    X, y, (b, S, ll, n_iter) = _fit_case(n, p, C, intercept)
    r = _fit(eng, X, y, [0, n], C, intercept)
    assert r["status"] == [0] and r["rc"] == 0
    errs = {"coef": rel(r["coef"][0].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][0].cpu().numpy(), S),
            "Sig_invMcoef": rel(r["Sig_invMcoef"][0].cpu().numpy(), S @ b), "ll": abs(r["loglik"][0] - ll) / abs(ll)}
    print("multinomial fit n=%d p=%d C=%d icpt=%d: %d evaluations (reference %d) %s" % (n, p, C, intercept, r["n_iter"][0], n_iter,
                                                                                     " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-10 for v in errs.values()), errs
    assert abs(r["n_iter"][0] - n_iter) <= 1
    Sn = r["Sig_inv"][0].cpu().numpy()
    assert np.array_equal(Sn, Sn.T)


@pytest.mark.parametrize("p,intercept", [(7, True), (7, False), (50, True)])
def test_two_classes_equal_the_logistic_fit(eng, p, intercept):
    n, K = 3001, 3
    X, y = mr.data(90 + p, n, p, 2, intercept)
    Xd, yd = _dev(X, y)
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    a = eng.multinomial_fit_ex(Xd, yd, first, rows, row_step=K, classes=2, fit_intercept=intercept)
    b = eng.irls_fit_ex(Xd, yd, first, rows, row_step=K, fit_intercept=intercept)
    assert a["status"] == [0] * K and b["status"] == [0] * K
    errs = {key: rel(a[key].cpu().numpy(), b[key].cpu().numpy()) for key in ("coef", "Sig_inv", "Sig_invMcoef")}
    errs["ll"] = rel(a["loglik"], b["loglik"])
    print("multinomial C = 2 against irls_fit_ex p=%d icpt=%d: %s" % (p, intercept, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-10 for v in errs.values()), errs


def test_strided_partitions_equal_gathered_ones(eng):
    n, p, C, K = 1203, 9, 4, 4                           # 301, 301, 301, 300 rows
    X, y = mr.data(55, n, p, C, True)
    Xd, yd = _dev(X, y)
    rows = [len(range(k, n, K)) for k in range(K)]
    assert len(set(rows)) > 1
    s = eng.multinomial_fit_ex(Xd, yd, list(range(K)), rows, row_step=K, classes=C, fit_intercept=True)
    order = np.concatenate([np.arange(k, n, K) for k in range(K)])
    offs = np.concatenate([[0], np.cumsum(rows)]).tolist()
    c = _fit(eng, X[order], y[order], offs, C, True)
    assert s["status"] == [0] * K and c["status"] == [0] * K and s["n_iter"] == c["n_iter"]
    for key in ("coef", "Sig_inv", "Sig_invMcoef"):
        assert rel(s[key].cpu().numpy(), c[key].cpu().numpy()) <= 1e-12, key
    assert rel(s["loglik"], c["loglik"]) <= 1e-12


def test_fit_is_reproducible(eng):
    n, p, C = 5000, 130, 3
    X, y = mr.data(56, n, p, C, True)
    a = _fit(eng, X, y, [0, 2000, n], C, True)
    b = _fit(eng, X, y, [0, 2000, n], C, True)
    assert a["status"] == [0, 0]
    for key in ("coef", "Sig_inv", "Sig_invMcoef"):
        assert torch.equal(a[key], b[key]), key
    assert a["loglik"] == b["loglik"] and a["n_iter"] == b["n_iter"]
    Xd, yd, td = _dev(X, y, mr.away_from_optimum(2 * (p + 1)))
    u, v = eng.multinomial_pass(Xd, yd, td, C, fit_intercept=True, want_prob=True), eng.multinomial_pass(Xd, yd, td, C, fit_intercept=True, want_prob=True)
    assert all(torch.equal(s, t) for s, t in zip(u, v))


def test_empty_partition_is_the_zero_block(eng):
    X, y = mr.data(57, 600, 5, 3, True)
    r = _fit(eng, X, y, [0, 300, 300, 600], 3, True)
    assert r["status"] == [0, 4, 0] and r["rc"] == 0 and r["n_iter"][1] == 0 and r["loglik"][1] == 0.0
    for key in ("coef", "Sig_inv", "Sig_invMcoef"):
        assert float(r[key][1].abs().max()) == 0.0
    one = _fit(eng, X[300:], y[300:], [0, 300], 3, True)
    assert torch.equal(one["coef"][0], r["coef"][2])


def test_collinear_column_is_not_spd(eng):
    """an all-zero column leaves an exactly zero pivot: NOT_SPD at the first evaluation (a duplicated column leaves a last pivot of
    rounding noise of either sign, which the solver's pivot <= 0 rule catches or not)"""
    X, y = mr.data(60, 2000, 5, 3, False)
    X = np.column_stack([X, np.zeros(2000)])
    r = _fit(eng, X, y, [0, 2000], 3, False)
    assert r["status"] == [2] and r["rc"] == 4


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes,p,text", [(1, 5, "classes must lie in 2 .. 8"), (9, 5, "classes must lie in 2 .. 8"),
                                            (8, 300, "exceed the solver's 2048")])
def test_class_count_and_dimension_are_refused(eng, classes, p, text):
    from dlsa_amd import _lib
    X, y = mr.data(61, 50, p, 2, False)
    Xd, yd = _dev(X, y)
    td = torch.zeros(max(1, classes - 1) * p, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=text):
        eng.multinomial_pass(Xd, yd, td, classes)
    with pytest.raises(ValueError, match=text):
        eng.multinomial_fit_ex(Xd, yd, [0], [50], classes=classes)
    # the C ABI's own check, below the Python one
    lib = _lib.load()
    assert lib.dlsa_multinomial_workspace_bytes(50, p, 0, classes, 1) == 0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    g = torch.empty(td.numel(), dtype=torch.float64, device="cuda")
    rc = lib.dlsa_multinomial_pass_f64(Xd.data_ptr(), p, yd.data_ptr(), td.data_ptr(), classes, 50, p, 0, None, 0, g.data_ptr(), None, None, 0,
                                       ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and text in _lib.last_error()
    first, rows = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(50)
    rc = lib.dlsa_multinomial_fit_f64(Xd.data_ptr(), p, yd.data_ptr(), first, rows, 1, 1, p, 0, classes, 1e-13, 100, g.data_ptr(), g.data_ptr(),
                                      g.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and text in _lib.last_error()


@pytest.mark.parametrize("bad", [1.5, -1.0, 3.0, float("nan")])
def test_a_response_that_is_no_class_code_is_refused(eng, bad):
    from dlsa_amd import _lib
    C = 3
    X, y = mr.data(62, 400, 4, C, True)
    y[[250, 310]] = bad
    with pytest.raises(_lib.DlsaError) as ex:
        _fit(eng, X, y, [0, 200, 400], C, True)
    assert ex.value.code == 1 and "partition 1 has 2 rows whose response is not a class code 0 .. 2" in str(ex.value)
    # the pass answers with loglik = NaN and checks nothing else
    Xd, yd, td = _dev(X, y, np.zeros(2 * 5))
    assert np.isnan(eng.multinomial_pass(Xd, yd, td, C, fit_intercept=True, want_H=False)[2].item())
    # the first partition alone fits
    assert _fit(eng, X, y, [0, 200], C, True)["status"] == [0]


def test_a_partition_that_lacks_a_class_is_refused(eng):
    from dlsa_amd import _lib
    C = 4
    X, y = mr.data(63, 900, 4, C, True)
    y[300:600][y[300:600] == 2] = 1.0
    with pytest.raises(_lib.DlsaError) as ex:
        _fit(eng, X, y, [0, 300, 600, 900], C, True)
    assert ex.value.code == 1 and "partition 1 has no row of class 2" in str(ex.value)
    # the other partitions hold every class: they fit
    assert _fit(eng, X, y, [0, 300], C, True)["status"] == [0]


# ---- calibration, end to end, frames ---------------------------------------------------------------------------------------------------
def test_block_is_calibrated(eng):
    """24 strided partitions of 1500 rows, 4 features + intercept, 3 classes (dimension 10): Q = sum_k (theta_k - theta*)' Sig_inv_k
    (theta_k - theta*) is chi-square on 240 degrees of freedom, so it lies in 240 +- 4 sqrt(480) = 240 +- 88.  The reference alone
    gives 246.0 for this seed (test_multinomial_cpu.py asserts 240 +- 44)."""
    import dlsa_amd
    X, y = mr.calibration_case()
    Xd, yd = _dev(X, y)
    mb = dlsa_amd.fit_multinomial_partitions(Xd, yd, mr.CALIBRATION_CLASSES, partition_num=mr.CALIBRATION_K, fit_intercept=True)
    assert mb.status == [0] * mr.CALIBRATION_K
    q = mr.calibration_q(mb.coef.cpu().numpy(), mb.Sig_inv.cpu().numpy())
    print("multinomial calibration: Q %.1f on 240 degrees of freedom" % q)
    assert abs(q - 240.0) <= 88.0


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K, C = 24_000, 6, 8, 3
    X, y = mr.data(90, n, p, C, True)
    Xd, yd = _dev(X, y)
    mb = dlsa_amd.fit_multinomial_partitions(Xd, yd, C, partition_num=K, fit_intercept=True)
    assert mb.status == [0] * K
    base = ["intercept"] + ["x%d" % i for i in range(p)]
    assert mb.names == [nm + ":1" for nm in base] + [nm + ":2" for nm in base]
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [mr.block(X[k::K], y[k::K], C, True) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    # LARS on a no-intercept design: the blocks carry no unpenalised entry
    mb0 = dlsa_amd.fit_multinomial_partitions(Xd, yd, C, partition_num=K, fit_intercept=False)
    out0 = dlsa_amd.dlsa_mapred(mb0)
    S0, ols0 = out0.iloc[:, 2:].to_numpy(), out0["beta_byOLS"].to_numpy()
    by_aic, by_bic, _ = orc.dlsa(S0, ols0, n)
    res = dlsa_amd.dlsa(S0, ols0, n, fit_intercept=False)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8
    path = eng.lars_path(torch.from_numpy(S0).cuda(), torch.from_numpy(ols0).cuda(), False, float(n))
    assert rel(path["beta"].cpu().numpy(), orc.lars_lsa(S0, ols0, False, n)["beta"]) <= 1e-8


def test_multinomial_model_frame_and_eval(eng):
    import pandas as pd
    import dlsa_amd
    labels = ["on time", "weather", "carrier"]
    # (an even p: the frame path pads the rows of an odd one to an even pitch, which is another Gram staging and other last bits)
    df = dlsa_amd.simulate_multinomial(4000, 6, 1, 3, seed=7)
    assert list(df.columns) == ["partition_id", "y"] + ["x%d" % i for i in range(6)] and set(df["y"]) == {0.0, 1.0, 2.0}
    codes = df["y"].to_numpy()
    part = df.drop(columns=["partition_id"]).assign(y=[labels[int(c)] for c in codes])
    out = dlsa_amd.multinomial_model(part, "y", labels, fit_intercept=True)
    base = ["intercept"] + ["x%d" % i for i in range(6)]
    names = [nm + ":1" for nm in base] + [nm + ":2" for nm in base]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (14, 17)
    X = part[base[1:]].to_numpy()
    Xd, yd = _dev(X, codes)
    mb = dlsa_amd.fit_multinomial_partitions(Xd, yd, 3, fit_intercept=True)
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out["Sig_invMcoef"].to_numpy(), mb.Sig_invMcoef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    b, S, ll, _ = mr.fit(X, codes, 3, True)
    assert rel(out["coef"].to_numpy(), b) <= 1e-10 and rel(out[names].to_numpy(), S) <= 1e-10
    par = pd.DataFrame({"mle": mb.coef[0].cpu().numpy(), "away": mr.away_from_optimum(14)})
    ev = dlsa_amd.multinomial_model_eval(part, "y", par, labels, fit_intercept=True)
    assert list(ev.columns) == ["mle", "away"] and ev.shape == (1, 2)
    refs = [mr.terms(X, codes, par[c].to_numpy(), 3, True)[0] for c in par.columns]
    assert rel(ev.to_numpy()[0], refs) <= 1e-12
    # the reference class is the first label: another order is another parameterisation of the same fit
    swapped = dlsa_amd.multinomial_model(part, "y", [labels[1], labels[0], labels[2]], fit_intercept=True)
    assert rel(swapped["coef"].to_numpy()[:7], -b[:7]) <= 1e-9
    with pytest.raises(ValueError, match="not among classes"):
        dlsa_amd.multinomial_model(part, "y", labels[:2], fit_intercept=True)


def test_multinomial_model_dummy_factor_and_missing_level(eng):
    import pandas as pd
    import dlsa_amd
    rng = np.random.default_rng(2)
    n, labels = 4000, ["a", "b", "c"]
    df = pd.DataFrame({"y": "a", "dist": rng.normal(5.0, 2.0, n), "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2])})
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC"]).astype(float)
    codes = mr.draw(rng, Xo, np.array([-0.3, 0.1, 0.4, 0.0, 0.3, -0.1, 0.0, 0.5]), 3, True)
    df["y"] = [labels[int(c)] for c in codes]
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"]}, "factor_dropped": {"carrier": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"]}}
    baseline = ["carrier_AA"]
    base = ["intercept", "dist", "carrier_BB", "carrier_CC"]
    want = ["par_id", "coef", "Sig_invMcoef"] + [nm + ":1" for nm in base] + [nm + ":2" for nm in base]
    out = dlsa_amd.multinomial_model(df, "y", labels, fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert list(out.columns) == want
    b, S, _, _ = mr.fit(Xo, codes, 3, True)
    assert rel(out["coef"], b) <= 1e-10 and rel(out.iloc[:, 3:].to_numpy(), S) <= 1e-10
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = dlsa_amd.multinomial_model(sub, "y", labels, fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    assert any("missing in this data chunk" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (8, 11) and float(np.abs(zero.to_numpy()).max()) == 0.0
