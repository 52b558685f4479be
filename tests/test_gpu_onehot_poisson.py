"""GPU: the structured one-hot Poisson map step (csrc/onehot_poisson.hip) -- the Poisson pass and fit on raw numerics + level
codes -- against the numpy reference (tests/poisson_reference.py) on the dense matrix oracle.dlsa_oracle.design_matrix builds:
the pass at a fixed beta, eta beyond 700, the per-partition fit, structured = dense, edge cases, reproducibility, the end-to-end
DLSA combine, the frame-level poisson_model / poisson_model_eval, and a 1.4e7-row fit with its memory bound."""
import math
import os
import sys
import warnings

import numpy as np
import pytest

import poisson_reference as pr
from test_gpu_onehot import _plan, _random_design

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL_PASS = 1e-12
TOL_FIT = 1e-10
SHAPES = [(5000, 7, (11, 6, 20)), (3001, 2, (3,)), (20000, 0, (5, 4)), (777, 7, (40, 40, 9, 2)),
          (4000, 3, (110, 110, 20, 6)), (1, 1, (2,)), (6000, 2, (1400, 5)), (3000, 0, (700, 8, 3)),
          (2000, 1, (1000,)),           # p = 1001: the row pass's residual histogram runs with two LDS copies (the others: 8, 4, 1)
          (257, 0, (3, 2))]             # one workgroup whose second round has 255 of 256 threads masked; no dense column without intercept


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


def _check_pass(plan, num, codes, y, o, beta, X, tag=None):
    """structured pass == the reference on the dense matrix X, every figure printed before it is asserted"""
    from dlsa_amd import engine
    q = num.shape[1]
    H, g, ll, w = engine.onehot_poisson_pass(plan, dev(num) if q else None, dev(codes), dev(y), dev(beta), offset=dev(o), want_w=True)
    llr, gr, Hr, mur = pr.terms(X, y, beta, o, False)
    Hn = H.cpu().numpy()
    figs = (abs(float(ll.item()) - llr) / abs(llr), rel(g.cpu().numpy(), gr), rel(w.cpu().numpy(), mur), rel(Hn, Hr))
    print("pass", tag, "rel err ll %.2e g %.2e mu %.2e H %.2e" % figs)
    assert math.isfinite(llr) and np.all(np.isfinite(Hr))
    assert figs[0] <= TOL_PASS and figs[1] <= TOL_PASS and figs[2] <= TOL_PASS and figs[3] <= TOL_PASS, figs
    assert np.array_equal(Hn, Hn.T)
    return H, g, ll, w


def _counts(rng, X, beta, o):
    eta = X @ beta + (0.0 if o is None else o)
    return rng.poisson(np.exp(np.clip(0.5 * eta, -20, 4))).astype(np.float64)       # any counts do: the pass is checked away from the MLE


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("intercept,baseline", [(True, True), (False, False)])
@pytest.mark.parametrize("n,q,nlevels", SHAPES)
def test_pass_matches_reference(api, orc, n, q, nlevels, intercept, baseline, offset):
    rng = np.random.default_rng(n + q)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels, intercept=intercept, baseline=baseline)
    codes[rng.integers(0, n, max(1, n // 50)), 0] = -1          # unknown level: no column
    plan = _plan(api, p, desc, nl, level_col)
    if nlevels[:2] == (110, 110):
        assert plan.roles >= 2                                  # several Gram roles
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.4                             # eta spans a few units
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    y = _counts(rng, X, beta, o)
    _check_pass(plan, num, codes, y, o, beta, X, (n, q, nlevels, intercept, baseline, offset))


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
        _check_pass(plan, num, codes, _counts(rng, X, beta, o), o, beta, X, (n, q, nlevels, "unordered"))


@pytest.mark.parametrize("n,q,nlevels", [(30000, 2, (300, 300)), (9000, 3, (700, 40))])
def test_pass_with_row_banded_pair_tables(api, orc, n, q, nlevels):
    rng = np.random.default_rng(n)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    assert plan.roles >= 2                                      # a pair table beyond LDS, cut into row bands
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.4
    o = np.log(rng.uniform(0.5, 2.0, n))
    _check_pass(plan, num, codes, _counts(rng, X, beta, o), o, beta, X, (n, q, nlevels))


@pytest.mark.parametrize("seed", range(20))
def test_pass_randomised_designs(api, orc, seed):
    """Seeded random designs as test_onehot_passes_randomised_designs: 0-7 numerics, 1-5 factors of 2-120 levels, a few rows with
    an unknown level, with and without intercept / baselines / offset, 1-40000 rows."""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([rng.integers(1, 300), rng.integers(300, 6000), rng.integers(6000, 40000)]))
    q = int(rng.integers(0, 8))
    nlevels = tuple(int(rng.choice([rng.integers(2, 8), rng.integers(8, 40), rng.integers(40, 121)])) for _ in range(int(rng.integers(1, 6))))
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels, intercept=bool(rng.random() < 0.7), baseline=bool(rng.random() < 0.7))
    if n > 10:
        codes[rng.integers(0, n, max(1, n // 40)), int(rng.integers(0, len(nlevels)))] = -1
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * float(rng.choice([0.05, 0.4, 1.0]))
    o = np.log(rng.uniform(0.5, 2.0, n)) if rng.random() < 0.5 else None
    _check_pass(plan, num, codes, _counts(rng, X, beta, o), o, beta, X, (seed, n, q, nlevels))


def test_pass_eta_spanning_700(api, orc):
    """Level coefficients of +-400 with a compensating offset: the gathered part of eta spans 800, and with a ramp in the offset
    log mu itself spans more than 700 -- the log-likelihood stays finite and everything equals the reference."""
    rng = np.random.default_rng(700)
    n, q, nlevels = 4000, 2, (3, 5)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.2
    c1, c2 = level_col[1], level_col[2]                         # levels 1 and 2 of factor 0
    beta[c1], beta[c2] = 400.0, -400.0
    o = -400.0 * (codes[:, 0] == 1) + 400.0 * (codes[:, 0] == 2) + np.linspace(-352.0, 352.0, n)
    y = rng.poisson(1.0, n).astype(np.float64)
    ll, g, H, mu = pr.terms(X, y, beta, o, False)
    assert np.ptp(X @ beta) > 700 and np.ptp(np.log(mu)) > 700 and np.isfinite(ll) and np.all(np.isfinite(H)) and np.all(np.isfinite(g))
    H2, g2, ll2, _ = _check_pass(plan, num, codes, y, o, beta, X, "eta>700")
    assert math.isfinite(float(ll2.item())) and bool(torch.isfinite(g2).all()) and bool(torch.isfinite(H2).all())


# ---- fit ----------------------------------------------------------------------------------------------------------------
def _zipf_design(rng, n, q, nlevels):
    """intercept, q standardised numerics (shift / scale as _random_design), baselines dropped, Zipf level frequencies (1 / rank)"""
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    for t, L in enumerate(nlevels):
        w = 1.0 / np.arange(1, L + 1)
        codes[:, t] = rng.choice(L, n, p=w / w.sum())
    return p, num, codes, desc, nl, level_col


def _fit_case(orc, n, q, nlevels, seed):
    rng = np.random.default_rng(seed)
    p, num, codes, desc, nl, level_col = _zipf_design(rng, n, q, nlevels)
    X, _ = orc.design_matrix(num, codes, *desc)
    bt = rng.normal(size=p) * 0.3
    bt[0] = -0.5
    e = rng.uniform(0.5, 2.0, n)
    y = rng.poisson(e * np.exp(X @ bt)).astype(np.float64)
    return p, num, codes, desc, nl, level_col, X, y, e


def _assert_events(X, y, parts, least=5):
    """the test's own inputs: a level without events has its MLE at -infinity, so every column needs events in every partition"""
    for k, sl in enumerate(parts):
        ev = (X[sl] != 0).T.astype(np.float64) @ y[sl]
        print("partition", k, "min events per column", ev.min())
        assert ev.min() >= least, (k, ev.min())


def _check_blocks(r, X, y, o, parts):
    assert r["status"] == [0] * len(parts), r["status"]
    for k, sl in enumerate(parts):
        b, H, ll = pr.fit(X[sl], y[sl], o[sl], False)
        figs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H),
                rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b), abs(r["loglik"][k] - ll) / abs(ll))
        print("fit partition", k, "rel err coef %.2e Sig_inv %.2e Sig_invMcoef %.2e loglik %.2e" % figs, "iters", r["n_iter"][k])
        assert max(figs) <= TOL_FIT, (k, figs)


# (seeds: n + q where every level column then has >= 5 events in every partition -- 12-38 and 8-18 for the first and the third case;
#  the second case's n + q leaves a column without events in one partition, seed 40008 gives 8-12)
@pytest.mark.parametrize("n,q,nlevels,K,strided,seed", [(60_000, 7, (11, 6, 20, 110, 110), 4, True, 60_007),
                                                        (40_000, 3, (110, 110, 20, 6), 4, False, 40_008),
                                                        (24_000, 2, (40, 5), 6, True, 24_002)])
def test_fit_matches_reference(api, orc, n, q, nlevels, K, strided, seed):
    from dlsa_amd import engine
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, seed)
    if nlevels[-1] == 110:
        assert p == 260
    o = np.log(e)
    if strided:
        parts = [slice(k, n, K) for k in range(K)]
        first, rows, step = list(range(K)), [len(range(k, n, K)) for k in range(K)], K
    else:
        parts = [slice(k * n // K, (k + 1) * n // K) for k in range(K)]
        first, rows, step = [s.start for s in parts], [s.stop - s.start for s in parts], 1
    _assert_events(X, y, parts)
    plan = _plan(api, p, desc, nl, level_col)
    r = engine.onehot_poisson_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step, offset=dev(o))
    _check_blocks(r, X, y, o, parts)


def _spec(api, q, nlevels, desc):
    """a DesignSpec for the column plan of _random_design (numeric columns n0.., factors f0.. with levels '0', '1', ...)"""
    kind, src, level, shift, scale = desc
    factors = ["f%d" % t for t in range(len(nlevels))]
    names = []
    for j in range(len(kind)):
        names.append("intercept" if kind[j] == 0 else "n%d" % src[j] if kind[j] == 1 else "f%d_%d" % (src[j], level[j]))
    return api.DesignSpec(["n%d" % a for a in range(q)], factors, {f: [str(l) for l in range(L)] for f, L in zip(factors, nlevels)},
                          names, kind, src, level, shift, scale, [j for j in range(len(kind)) if kind[j] == 2])


def test_structured_equals_dense_and_strided_equals_contiguous(api, orc):
    n, q, nlevels, K = 30_001, 3, (7, 4, 12), 5
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 41)
    _assert_events(X, y, [slice(k, n, K) for k in range(K)])
    spec = _spec(api, q, nlevels, desc)
    assert spec.onehot_plan() is not None
    dn, dc, dy, de = dev(num), dev(codes), dev(y), dev(e)
    a = api.fit_poisson_design(dn, dc, dy, spec, partition_num=K, exposure=de)
    d = api.fit_poisson_design(dn, dc, dy, spec, partition_num=K, exposure=de, structured=False)
    assert a.status == [0] * K and d.status == [0] * K and a.names == spec.names and d.names == spec.names
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(d, f).cpu().numpy())
        print("structured vs dense", f, "%.2e" % err)
        assert err <= TOL_FIT
    assert rel(a.loglik, d.loglik) <= TOL_FIT
    # (n_iter is not compared here: structured=False fits the built matrix, whose constant column is a column like any other, from
    #  beta = 0, while the structured fit starts the plan's constant column at log(sum y / sum e^o) -- [7, 7, 7, 7, 8] against
    #  [6, 6, 7, 7, 7] evaluations; test_structured_and_dense_fit_take_the_same_evaluations compares the two from one start)
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    c = api.fit_poisson_design(dev(num[perm]), dev(codes[perm]), dev(y[perm]), spec, part_offsets=offs, offset=dev(np.log(e[perm])))
    assert c.status == [0] * K
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(c, f).cpu().numpy())
        print("strided vs contiguous", f, "%.2e" % err)
        assert err <= 1e-13
    with pytest.raises(ValueError):
        api.fit_poisson_design(dn, dc, dy, spec, offset=torch.log(de), exposure=de)
    with pytest.raises(ValueError):
        api.fit_poisson_design(dn, dc, -dy - 1.0, spec)


@pytest.mark.parametrize("max_iter", [100, 2])
def test_structured_and_dense_fit_take_the_same_evaluations(api, orc, max_iter):
    """one Newton loop behind both fits: a small plan whose constant column is column 0, against the dense fit of the built matrix's
    other columns with the implicit intercept -- the same model, columns in the same order and the same start (the intercept at
    log(sum y / sum e^o), zeros elsewhere), so the same evaluations, the same status and the same log-likelihood"""
    from dlsa_amd import engine
    n, q, nlevels = 600, 2, (5, 3)
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 611)
    assert desc[0][0] == 0 and np.all(X[:, 0] == 1.0)                 # column 0 is the plan's constant column
    _assert_events(X, y, [slice(0, n)])
    o = np.log(e)
    plan = _plan(api, p, desc, nl, level_col)
    a = engine.onehot_poisson_fit_ex(plan, dev(num), dev(codes), dev(y), [0], [n], offset=dev(o), max_iter=max_iter)
    d = engine.poisson_fit_ex(dev(X[:, 1:]), dev(y), [0], [n], offset=dev(o), fit_intercept=True, max_iter=max_iter)
    print("structured / dense: n_iter", a["n_iter"], d["n_iter"], "status", a["status"], d["status"], "loglik", a["loglik"], d["loglik"])
    assert a["n_iter"] == d["n_iter"] and a["status"] == d["status"] == [0 if max_iter == 100 else 1] and a["rc"] == d["rc"]
    assert rel(a["loglik"], d["loglik"]) <= TOL_FIT
    assert rel(a["coef"][0].cpu().numpy(), d["coef"][0].cpu().numpy()) <= TOL_FIT


def test_fit_empty_and_all_zero_partitions(api, orc):
    from dlsa_amd import engine
    n, q, nlevels = 8000, 2, (4, 3)
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 50)
    y[2000:4000] = 0.0
    offs = [0, 2000, 4000, 4000, n]
    plan = _plan(api, p, desc, nl, level_col)
    r = engine.onehot_poisson_fit_ex(plan, dev(num), dev(codes), dev(y), offs[:-1], [offs[k + 1] - offs[k] for k in range(4)],
                                     offset=dev(np.log(e)))
    assert r["status"] == [0, 4, 4, 0], r["status"]
    for k in (1, 2):
        assert not r["Sig_inv"][k].any() and not r["coef"][k].any() and not r["Sig_invMcoef"][k].any()
        assert r["loglik"][k] == 0.0
    b, H, _ = pr.fit(X[4000:], y[4000:], np.log(e[4000:]), False)
    assert rel(r["coef"][3].cpu().numpy(), b) <= TOL_FIT and rel(r["Sig_inv"][3].cpu().numpy(), H) <= TOL_FIT


def test_duplicated_level_column_has_the_dense_fits_status(api, orc):
    from dlsa_amd import engine
    rng = np.random.default_rng(60)
    n = 3000
    p, num, codes, desc, nl, level_col = _random_design(rng, n, 2, (4, 4))
    codes[:, 1] = codes[:, 0]                                   # two factors with identical codes: pairs of identical columns
    X, _ = orc.design_matrix(num, codes, *desc)
    y = rng.poisson(1.5, n).astype(np.float64)
    plan = _plan(api, p, desc, nl, level_col)
    r = engine.onehot_poisson_fit_ex(plan, dev(num), dev(codes), dev(y), [0], [n])
    d = engine.poisson_fit_ex(dev(X), dev(y), [0], [n])
    print("duplicated column: structured", r["status"], r["rc"], "dense", d["status"], d["rc"])
    assert r["status"] == d["status"] and r["rc"] == d["rc"]
    assert r["status"] == [2] and r["rc"] == 4                  # NOT_SPD


def test_invalid_counts_and_offsets_are_refused_and_arguments_checked(api, orc):
    from dlsa_amd import engine, _lib
    n, q, nlevels = 1000, 2, (4, 3)
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 61)
    o = np.log(e)
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc = dev(num), dev(codes)
    fit = lambda yy, oo: engine.onehot_poisson_fit_ex(plan, dn, dc, dev(yy), [0, 500], [500, 500], offset=dev(oo))
    y_bad = y.copy(); y_bad[700] = -1.0
    with pytest.raises(_lib.DlsaError) as ex:
        fit(y_bad, o)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    y_nan = y.copy(); y_nan[3] = np.nan
    with pytest.raises(_lib.DlsaError) as ex:
        fit(y_nan, o)
    assert ex.value.code == 1 and "partition 0" in str(ex.value)
    o_bad = o.copy(); o_bad[600] = np.inf
    with pytest.raises(_lib.DlsaError) as ex:
        fit(y, o_bad)
    assert ex.value.code == 1 and "partition 1" in str(ex.value)
    # the pass reports an invalid count as a NaN log-likelihood
    _, _, ll, _ = engine.onehot_poisson_pass(plan, dn, dc, dev(y_bad), dev(np.zeros(p)), want_H=False)
    assert math.isnan(float(ll.item()))
    # argument checks that need a plan (before any launch), and the workspace query
    lib = _lib.load()
    import ctypes
    fake = ctypes.c_void_p(256)
    args = [plan._h, fake, q, fake, len(nlevels), fake, None, fake, 10, fake, p, None, None, None, fake, 1 << 30, None]
    for i, v in ((1, None), (3, None), (8, 0), (2, q - 1), (4, len(nlevels) - 1), (10, p - 1)):
        a = list(args); a[i] = v
        assert lib.dlsa_onehot_poisson_pass_f64(*a) == 1, (i, v)
    a = list(args); a[15] = 1024
    assert lib.dlsa_onehot_poisson_pass_f64(*a) == 3
    a = list(args); a[14] = ctypes.c_void_p(257)
    assert lib.dlsa_onehot_poisson_pass_f64(*a) == 3
    first, rows = (ctypes.c_int64 * 2)(0, 5), (ctypes.c_int64 * 2)(5, 5)
    fargs = [plan._h, fake, q, fake, len(nlevels), fake, None, first, rows, 1, 2, 1e-13, 100, fake, fake, fake, None, None, None, fake,
             1 << 30, None]
    for i, v in ((9, 0), (10, 0), (11, 0.0), (12, 0), (2, q - 1), (4, len(nlevels) - 1)):
        a = list(fargs); a[i] = v
        assert lib.dlsa_onehot_poisson_fit_f64(*a) == 1, (i, v)
    a = list(fargs); a[8] = (ctypes.c_int64 * 2)(5, -1)
    assert lib.dlsa_onehot_poisson_fit_f64(*a) == 1 and "partition 1" in _lib.last_error()
    a = list(fargs); a[20] = 4096
    assert lib.dlsa_onehot_poisson_fit_f64(*a) == 3
    prev = 0
    for rows_ in (0, 1, 63, 64, 65, 1000, 4096 * 64, 10 ** 6, 10 ** 7, 2 * 10 ** 7):
        for step in (1, 7):
            b = lib.dlsa_onehot_poisson_workspace_bytes(plan._h, rows_, step)
            assert b > 0 and b >= lib.dlsa_onehot_poisson_workspace_bytes(plan._h, rows_, 1)
        b = lib.dlsa_onehot_poisson_workspace_bytes(plan._h, rows_, 1)
        assert b >= prev, rows_
        prev = b
    assert lib.dlsa_onehot_poisson_workspace_bytes(plan._h, -1, 1) == 0 and lib.dlsa_onehot_poisson_workspace_bytes(plan._h, 10, 0) == 0


def test_fit_is_bit_reproducible(api, orc):
    n, q, nlevels, K = 200_000, 7, (11, 6, 20, 110, 110), 3
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 80)
    spec = _spec(api, q, nlevels, desc)
    dn, dc, dy, de = dev(num), dev(codes), dev(y), dev(e)
    a = api.fit_poisson_design(dn, dc, dy, spec, partition_num=K, exposure=de)
    b = api.fit_poisson_design(dn, dc, dy, spec, partition_num=K, exposure=de)
    assert a.status == [0] * K
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik


def test_end_to_end_dlsa(api, orc):
    n, q, nlevels, K = 80_000, 3, (6, 4, 9), 8
    p, num, codes, desc, nl, level_col, X, y, e = _fit_case(orc, n, q, nlevels, 90)
    o = np.log(e)
    _assert_events(X, y, [slice(k, n, K) for k in range(K)])
    spec = _spec(api, q, nlevels, desc)
    mb = api.fit_poisson_design(dev(num), dev(codes), dev(y), spec, partition_num=K, offset=dev(o))
    assert mb.status == [0] * K
    out = api.dlsa_mapred(mb)
    blocks = [pr.block(X[k::K], y[k::K], o[k::K], False) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = api.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


# ---- frames -------------------------------------------------------------------------------------------------------------
def _frame(seed, n):
    import pandas as pd
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({"partition_id": np.zeros(n), "y": 0.0, "expo": rng.uniform(0.5, 2.0, n), "dist": rng.normal(5.0, 2.0, n),
                       "age": rng.normal(40.0, 10.0, n), "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2]),
                       "region": rng.choice(["n", "s", "e", "w"], n)})
    eta = -0.3 + 0.1 * (df["dist"] - 5) - 0.02 * (df["age"] - 40) + 0.4 * (df["carrier"] == "BB") - 0.3 * (df["carrier"] == "CC") \
        + 0.2 * (df["region"] == "s") - 0.25 * (df["region"] == "w")
    df["y"] = rng.poisson(df["expo"] * np.exp(eta)).astype(float)
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"], "region": ["e", "n", "s", "w"]},
                  "factor_dropped": {"carrier": [], "region": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"],
                                            "region": ["region_e", "region_n", "region_s", "region_w"]}}
    baseline = ["carrier_AA", "region_e"]
    names = ["intercept", "age", "dist", "carrier_BB", "carrier_CC", "region_n", "region_s", "region_w"]
    Xo = np.column_stack([df["age"], df["dist"], df["carrier"] == "BB", df["carrier"] == "CC", df["region"] == "n", df["region"] == "s",
                          df["region"] == "w"]).astype(float)
    return df, dummy_info, baseline, names, Xo


def test_poisson_model_structured_frame_and_eval(api):
    import pandas as pd
    df, dummy_info, baseline, names, Xo = _frame(2, 6000)
    kw = dict(fit_intercept=True, exposure_name="expo", dummy_info=dummy_info, dummy_factors_baseline=baseline)
    out = api.poisson_model(df, "y", structured=True, **kw)
    dense = api.poisson_model(df, "y", structured=False, **kw)
    default = api.poisson_model(df, "y", **kw)
    want = ["par_id", "coef", "Sig_invMcoef"] + names
    assert list(out.columns) == want and list(dense.columns) == want
    assert default.equals(dense) and default.to_numpy().tobytes() == dense.to_numpy().tobytes()      # the default is the dense path
    o = np.log(df["expo"].to_numpy())
    b, H, ll = pr.fit(Xo, df["y"].to_numpy(), o, True)
    figs = (rel(out["coef"], b), rel(out[names].to_numpy(), H), rel(out["Sig_invMcoef"], H @ b))
    print("poisson_model structured vs reference", figs)
    assert max(figs) <= TOL_FIT
    assert rel(out["coef"], dense["coef"]) <= TOL_FIT and rel(out[names].to_numpy(), dense[names].to_numpy()) <= TOL_FIT
    assert rel(out["Sig_invMcoef"], dense["Sig_invMcoef"]) <= TOL_FIT
    # a missing level: the zero block and the reference's warning, from the codes
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = api.poisson_model(sub, "y", structured=True, **kw)
    assert any("missing in this data chunk" in str(w.message) and "Skip modeling" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (8, 11) and float(np.abs(zero.to_numpy()).max()) == 0.0
    # eval: the log-likelihood of each estimator column
    par = pd.DataFrame({"mle": out["coef"].to_numpy(), "ref": b, "zero": np.zeros(8)})
    ev = api.poisson_model_eval(df, "y", par, structured=True, **kw)
    assert list(ev.columns) == ["mle", "ref", "zero"] and ev.shape == (1, 3)
    refs = [pr.terms(Xo, df["y"].to_numpy(), par[c].to_numpy(), o, True)[0] for c in par.columns]
    print("poisson_model_eval structured vs reference %.2e" % rel(ev.to_numpy()[0], refs))
    assert rel(ev.to_numpy()[0], refs) <= 1e-12
    evd = api.poisson_model_eval(df, "y", par, structured=False, **kw)
    ev0 = api.poisson_model_eval(df, "y", par, **kw)
    assert ev0.to_numpy().tobytes() == evd.to_numpy().tobytes()
    assert rel(ev.to_numpy()[0], evd.to_numpy()[0]) <= 1e-12


# ---- at scale -----------------------------------------------------------------------------------------------------------
def test_at_scale_fit_on_raw_rows(api, orc):
    from conftest import need_hbm
    from dlsa_amd import engine
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench"))
    import surrogates                            # bench/surrogates.py: test / bench data, not product code
    need_hbm(8e9)
    n, K = 14_000_000, 14
    d = surrogates.airline_shaped(n, dense=False)
    num, codes, beta, plan, p = d["num"], d["codes"], d["beta"], d["plan"], d["p"]
    q, levels = num.shape[1], d["levels"]
    g = torch.Generator(device="cuda").manual_seed(5)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    eta = beta[0] + ((num - 1.5) / 3.0) @ beta[1:1 + q]
    pos = 1 + q
    for fi, L in enumerate(levels):
        tab = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), beta[pos:pos + L - 1]])
        eta = eta + tab[codes[:, fi].long()]
        pos += L - 1
    y = torch.poisson(torch.exp(eta + o), generator=g)
    del eta, tab, d["y"]
    raw = num.numel() * 8 + codes.numel() * 4 + y.numel() * 8 + o.numel() * 8
    assert abs(raw - 1.288e9) < 1e6
    torch.cuda.synchronize()
    engine.release_workspace()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    r = engine.onehot_poisson_fit_ex(plan, num, codes, y, first, rows, row_step=K, offset=o)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("at scale: peak %.3f GB, raw %.3f GB, iters %s" % (peak / 1e9, raw / 1e9, r["n_iter"]))
    assert peak < raw + 1e9, (peak, raw)
    assert r["status"] == [0] * K, r["status"]
    truth = beta.cpu().numpy()
    for k in range(K):
        nk, ck, ok = num[k::K].contiguous(), codes[k::K].contiguous(), o[k::K].contiguous()
        yk = y[k::K].contiguous()
        H, gs, ll, _ = engine.onehot_poisson_pass(plan, nk, ck, yk, r["coef"][k].contiguous(), offset=ok)
        score = float(gs.abs().max()) / float(yk.sum())
        Hn = H.cpu().numpy()
        se = np.sqrt(np.diag(np.linalg.inv(Hn)))
        z = np.abs(r["coef"][k].cpu().numpy() - truth) / se
        print("partition", k, "score / sum y %.2e" % score, "max z %.2f" % z.max())
        assert score <= 1e-9
        assert np.array_equal(Hn, Hn.T) and np.all(np.linalg.eigvalsh(Hn) > 0)
        assert rel(Hn, r["Sig_inv"][k].cpu().numpy()) <= 1e-12
        assert abs(float(ll.item()) - r["loglik"][k]) <= 1e-12 * abs(r["loglik"][k])
        assert z.max() <= 5.0, (k, z.max())
    # a 2e5-row slice of one partition against the reference pass
    m, k = 200_000, 3
    ns, cs = num[k::K][:m].cpu().numpy(), codes[k::K][:m].cpu().numpy()
    ys, os_ = y[k::K][:m].cpu().numpy(), o[k::K][:m].cpu().numpy()
    X, _ = orc.design_matrix(ns, cs, *[a.cpu().numpy() for a in d["spec"]])
    _check_pass(plan, ns, cs, ys, os_, r["coef"][k].cpu().numpy(), X, "2e5-row slice")
