"""GPU: the structured one-hot multinomial map step (csrc/onehot_multinomial.hip) -- the softmax pass and fit on raw numerics +
level codes -- against the numpy reference (tests/multinomial_reference.py, intercept=False) on the dense matrix
oracle.dlsa_oracle.design_matrix builds, whose constant column is the plan's: the pass at a fixed theta (loglik, g, H, P), eta
spanning 600 across the classes, the per-partition fit, structured = dense, strided = contiguous, two classes = the structured
logistic fit, reproducibility, the refusals, the end-to-end DLSA combine and the frame-level multinomial_model(_eval)."""
import ctypes
import math
import warnings

import numpy as np
import pytest

import multinomial_reference as mr
from test_gpu_onehot import _plan, _random_design
from test_gpu_onehot_poisson import SHAPES, _spec, _zipf_design, dev, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL_PASS = 1e-12
TOL_FIT = 1e-10
TOL_STRIDED = 1e-13
CLASSES = (2, 3, 5, 8)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import dlsa_amd
    return dlsa_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import dlsa_oracle
    return dlsa_oracle


def _shape_p(q, nlevels, intercept, baseline):
    return (1 if intercept else 0) + q + sum(nlevels) - (len(nlevels) if baseline else 0)


# every (C, shape, setting) whose (C - 1) p fits the solver's 2048
PASS_CASES = [(n, q, nl, C, ib) for (n, q, nl) in SHAPES for C in CLASSES for ib in ((True, True), (False, False))
              if (C - 1) * _shape_p(q, nl, *ib) <= 2048]


def test_the_case_list_holds_what_it_must():
    ps = {(C, _shape_p(q, nl, *ib)) for (n, q, nl, C, ib) in PASS_CASES}
    ns = {n for (n, q, nl, C, ib) in PASS_CASES}
    assert (2, 1406) in ps and (3, 1001) in ps and (3, 709) in ps and 1 in ns and 257 in ns
    smallest = sorted({_shape_p(q, nl, True, True) for (n, q, nl) in SHAPES})[:3]
    for p in smallest:
        assert {C for (C, pp) in ps if pp == p} == set(CLASSES), p


def _check_pass(plan, num, codes, y, theta, C, X, tag=None):
    """structured pass == the reference on the dense matrix X: loglik, g, H (as a whole and block by block, so every sub-block sits
    at its place; equal to its transpose bit for bit) and P, every figure printed before it is asserted"""
    from dlsa_amd import engine
    q = num.shape[1]
    J, p = C - 1, X.shape[1]
    H, g, ll, P = engine.onehot_multinomial_pass(plan, dev(num) if q else None, dev(codes), dev(y), dev(theta), C, want_prob=True)
    llr, gr, Hr, Pr = mr.terms(X, y, theta, C, False)
    Hn = H.cpu().numpy()
    blocks = max(rel(Hn[j * p:(j + 1) * p, k * p:(k + 1) * p], Hr[j * p:(j + 1) * p, k * p:(k + 1) * p]) for j in range(J) for k in range(J))
    figs = (abs(float(ll.item()) - llr) / abs(llr), rel(g.cpu().numpy(), gr), rel(P.cpu().numpy(), Pr), rel(Hn, Hr), blocks)
    print("pass", tag, "J p", J * p, "rel err ll %.2e g %.2e P %.2e H %.2e worst block of H %.2e" % figs)
    assert math.isfinite(llr) and np.all(np.isfinite(Hr)) and np.all(np.isfinite(gr))
    assert P.shape == (J, len(y)) and Hn.shape == (J * p, J * p)
    assert max(figs) <= TOL_PASS, figs
    assert np.array_equal(Hn, Hn.T)
    return H, g, ll, P


@pytest.mark.parametrize("n,q,nlevels,C,ib", PASS_CASES)
def test_pass_matches_reference(api, orc, n, q, nlevels, C, ib):
    intercept, baseline = ib
    rng = np.random.default_rng(n + q)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels, intercept=intercept, baseline=baseline)
    codes[rng.integers(0, n, max(1, n // 50)), 0] = -1          # unknown level: no column
    plan = _plan(api, p, desc, nl, level_col)
    if nlevels[:2] == (110, 110):
        assert plan.roles >= 2                                  # several Gram roles
    X, _ = orc.design_matrix(num, codes, *desc)
    theta = rng.normal(size=(C - 1) * p) * 0.4
    y = mr.draw(rng, X, theta, C, False)
    _check_pass(plan, num, codes, y, theta, C, X, (n, q, nlevels, C, intercept, baseline))


def test_pass_with_row_banded_pair_tables(api, orc):
    n, q, nlevels, C = 30000, 2, (300, 300), 3
    rng = np.random.default_rng(n)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    assert plan.roles >= 2                                      # a pair table beyond LDS, cut into row bands
    X, _ = orc.design_matrix(num, codes, *desc)
    theta = rng.normal(size=(C - 1) * p) * 0.4
    _check_pass(plan, num, codes, mr.draw(rng, X, theta, C, False), theta, C, X, (n, q, nlevels, C))


def test_pass_with_several_gram_roles(api, orc):
    n, q, nlevels, C = 4000, 3, (110, 110, 20, 6), 3
    rng = np.random.default_rng(n + 1)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    assert plan.roles >= 2
    X, _ = orc.design_matrix(num, codes, *desc)
    theta = rng.normal(size=(C - 1) * p) * 0.4
    _check_pass(plan, num, codes, mr.draw(rng, X, theta, C, False), theta, C, X, (n, q, nlevels, C, "multi-role"))


def test_pass_eta_spanning_600(api, orc):
    """One numeric running -1 .. 1 (shift 0, scale 1) with the coefficients 300, -300 and 150, one 3-level factor, an intercept,
    C = 4: the eta of a row span up to 600 across the classes and every class dominates somewhere -- everything stays finite and
    equals the reference."""
    n, C = 2000, 4
    rng = np.random.default_rng(600)
    arr = lambda v, t: np.asarray(v, dtype=t)
    desc = (arr([0, 1, 2, 2], np.int32), arr([0, 0, 0, 0], np.int32), arr([0, 0, 1, 2], np.int32), arr([0.0] * 4, np.float64),
            arr([1.0] * 4, np.float64))
    nl, level_col, p = [3], [-1, 2, 3], 4
    num = np.linspace(-1.0, 1.0, n)[:, None].copy()
    codes = rng.integers(0, 3, (n, 1)).astype(np.int32)
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    assert np.all(X[:, 0] == 1.0) and np.array_equal(X[:, 1], num[:, 0])
    theta = np.array([[-0.4, 300.0, 0.3, -0.2], [0.2, -300.0, -0.1, 0.4], [0.1, 150.0, 0.2, 0.1]]).reshape(-1)
    y = rng.integers(0, C, n).astype(np.float64)
    eta = X @ theta.reshape(3, p).T
    assert np.ptp(eta, axis=1).max() >= 599.0
    H, g, ll, P = _check_pass(plan, num, codes, y, theta, C, X, "eta span 600")
    assert math.isfinite(float(ll.item())) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(H).all()) and bool(torch.isfinite(P).all())


def test_pass_with_unordered_adds(api, orc):
    """onehot_ordered=0: all waves add at once, last bits vary from run to run -- against the reference only."""
    from dlsa_amd import engine
    n, q, nlevels, C = 777, 7, (40, 40, 9, 2), 3
    rng = np.random.default_rng(n + q)
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    theta = rng.normal(size=(C - 1) * p) * 0.4
    with engine.kernel_options(onehot_ordered=0):
        _check_pass(plan, num, codes, mr.draw(rng, X, theta, C, False), theta, C, X, (n, q, nlevels, "unordered"))


# ---- fit ----------------------------------------------------------------------------------------------------------------
def _ref_fit(X, y, C, icpt_col, tol=1e-13, max_iter=100):
    """mr.fit's loop on the dense matrix without an implicit intercept, started as the structured fit starts: theta = 0 with the
    constant column icpt_col (None: none) of class block j at log(n_j / n_0).  Returns (coef, H at coef, loglik, evaluations)."""
    J, p = C - 1, X.shape[1]
    theta = np.zeros((J, p))
    if icpt_col is not None:
        cnt = np.bincount(y.astype(np.int64), minlength=C).astype(np.float64)
        theta[:, icpt_col] = np.log(cnt[1:] / cnt[0])
    theta = theta.reshape(-1)
    prev, ll_prev, halvings, n_iter = None, None, 0, 0
    for it in range(max_iter + 1):
        ll, g, H, _ = mr.terms(X, y, theta, C, False)
        worse = (not np.isfinite(ll)) or (ll_prev is not None and ll < ll_prev - 1e-12 * abs(ll_prev))
        if ll_prev is not None and worse and halvings < 30:
            halvings += 1
            theta = prev + (theta - prev) / 2
            continue
        halvings, n_iter = 0, it + 1
        delta = np.linalg.solve(H, g)
        if np.max(np.abs(delta)) <= tol * max(1.0, np.max(np.abs(theta))):
            break
        prev, ll_prev, theta = theta, ll, theta + delta
    return theta, H, ll, n_iter


def _fit_case(orc, n, q, nlevels, seed, C):
    rng = np.random.default_rng(seed)
    p, num, codes, desc, nl, level_col = _zipf_design(rng, n, q, nlevels)
    X, _ = orc.design_matrix(num, codes, *desc)
    B = rng.normal(size=(C - 1, p)) * 0.3
    B[:, 0] = np.linspace(-0.3, 0.3, C - 1)
    y = mr.draw(rng, X, B.reshape(-1), C, False)
    return p, num, codes, desc, nl, level_col, X, y


def _assert_rows(X, y, parts, C, least=5):
    """the test's own inputs: a (column, class) pair without rows has its MLE at -infinity, so every pair needs rows in every partition"""
    worst = None
    for k, sl in enumerate(parts):
        cnt = (X[sl] != 0).T.astype(np.float64) @ (y[sl][:, None] == np.arange(C)[None, :]).astype(np.float64)
        print("partition", k, "min rows per (column, class)", cnt.min())
        worst = cnt.min() if worst is None else min(worst, cnt.min())
    assert worst >= least, worst
    return worst


def _parts(n, K, strided):
    if strided:
        return [slice(k, n, K) for k in range(K)], list(range(K)), [len(range(k, n, K)) for k in range(K)], K
    parts = [slice(k * n // K, (k + 1) * n // K) for k in range(K)]
    return parts, [s.start for s in parts], [s.stop - s.start for s in parts], 1


FIT_CASES = [(60_000, 3, (11, 6, 40), 4, True, 60_003, 3), (40_000, 2, (20, 6), 4, False, 40_002, 5),
             (120_000, 2, (110, 110), 2, True, 120_002, 3), (30_001, 3, (7, 4, 12), 5, True, 41, 4), (20_000, 1, (4, 3), 4, True, 7, 8)]


@pytest.mark.parametrize("n,q,nlevels,K,strided,seed,C", FIT_CASES)
def test_fit_matches_reference(api, orc, n, q, nlevels, K, strided, seed, C):
    from dlsa_amd import engine
    p, num, codes, desc, nl, level_col, X, y = _fit_case(orc, n, q, nlevels, seed, C)
    parts, first, rows, step = _parts(n, K, strided)
    _assert_rows(X, y, parts, C)
    assert desc[0][0] == 0 and np.all(X[:, 0] == 1.0)           # column 0 is the plan's constant column
    plan = _plan(api, p, desc, nl, level_col)
    r = engine.onehot_multinomial_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step, classes=C)
    assert r["status"] == [0] * K and r["rc"] == 0, (r["status"], r["rc"])
    for k, sl in enumerate(parts):
        b, H, ll, evals = _ref_fit(X[sl], y[sl], C, 0)
        figs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H),
                rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b), abs(r["loglik"][k] - ll) / abs(ll))
        print("fit partition", k, "rel err coef %.2e Sig_inv %.2e Sig_invMcoef %.2e loglik %.2e" % figs, "evaluations", r["n_iter"][k],
              "reference", evals)
        assert max(figs) <= TOL_FIT, (k, figs)


def test_structured_equals_dense_and_strided_equals_contiguous(api, orc):
    n, q, nlevels, K, C = 30_001, 3, (7, 4, 12), 5, 4
    p, num, codes, desc, nl, level_col, X, y = _fit_case(orc, n, q, nlevels, 41, C)
    _assert_rows(X, y, [slice(k, n, K) for k in range(K)], C)
    spec = _spec(api, q, nlevels, desc)
    assert spec.onehot_plan() is not None
    names = api.multinomial_column_names(spec.names, C)
    assert len(names) == (C - 1) * p and names[0] == "intercept:1" and names[p] == "intercept:2"
    dn, dc, dy = dev(num), dev(codes), dev(y)
    a = api.fit_multinomial_design(dn, dc, dy, spec, C, partition_num=K)
    d = api.fit_multinomial_design(dn, dc, dy, spec, C, partition_num=K, structured=False)
    assert a.status == [0] * K and d.status == [0] * K and a.names == names and d.names == names
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(d, f).cpu().numpy())
        print("structured vs dense", f, "%.2e" % err)
        assert err <= TOL_FIT
    print("structured vs dense loglik %.2e" % rel(a.loglik, d.loglik), "evaluations", a.n_iter, d.n_iter)
    assert rel(a.loglik, d.loglik) <= TOL_FIT
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    c = api.fit_multinomial_design(dev(num[perm]), dev(codes[perm]), dev(y[perm]), spec, C, part_offsets=offs)
    assert c.status == [0] * K
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(c, f).cpu().numpy())
        print("strided vs contiguous", f, "%.2e" % err)
        assert err <= TOL_STRIDED
    assert rel(a.loglik, c.loglik) <= TOL_STRIDED


def test_two_classes_equal_the_structured_logistic_fit(api, orc):
    from dlsa_amd import engine
    n, q, nlevels, K, C = 20_000, 2, (6, 4), 4, 2
    p, num, codes, desc, nl, level_col, X, y = _fit_case(orc, n, q, nlevels, 22, C)
    parts, first, rows, step = _parts(n, K, True)
    _assert_rows(X, y, parts, C)
    plan = _plan(api, p, desc, nl, level_col)
    a = engine.onehot_multinomial_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step, classes=2)
    b = engine.onehot_irls_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step)
    assert a["status"] == [0] * K and b["status"] == [0] * K
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(a[f].cpu().numpy(), b[f].cpu().numpy())
        print("two classes vs the structured logistic fit", f, "%.2e" % err)
        assert err <= TOL_FIT


def test_pass_and_fit_are_bit_reproducible(api, orc):
    from dlsa_amd import engine
    n, q, nlevels, K, C = 50_000, 3, (11, 6, 40), 3, 3
    p, num, codes, desc, nl, level_col, X, y = _fit_case(orc, n, q, nlevels, 80, C)
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc, dy = dev(num), dev(codes), dev(y)
    theta = dev(np.random.default_rng(81).normal(size=(C - 1) * p) * 0.4)
    one = engine.onehot_multinomial_pass(plan, dn, dc, dy, theta, C, want_prob=True)
    two = engine.onehot_multinomial_pass(plan, dn, dc, dy, theta, C, want_prob=True)
    assert all(torch.equal(u, v) for u, v in zip(one, two))
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    a = engine.onehot_multinomial_fit_ex(plan, dn, dc, dy, first, rows, row_step=K, classes=C)
    b = engine.onehot_multinomial_fit_ex(plan, dn, dc, dy, first, rows, row_step=K, classes=C)
    assert a["status"] == [0] * K
    assert torch.equal(a["coef"], b["coef"]) and torch.equal(a["Sig_inv"], b["Sig_inv"]) and torch.equal(a["Sig_invMcoef"], b["Sig_invMcoef"])
    assert a["loglik"] == b["loglik"] and a["n_iter"] == b["n_iter"]


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _small(api, orc, C=3, n=1200, seed=61):
    p, num, codes, desc, nl, level_col, X, y = _fit_case(orc, n, 2, (4, 3), seed, C)
    return p, num, codes, _plan(api, p, desc, nl, level_col), X, y


@pytest.mark.parametrize("bad", [1.5, -1.0, 3.0, float("nan")])
def test_a_response_that_is_no_class_code_is_refused(api, orc, bad):
    from dlsa_amd import engine, _lib
    C = 3
    p, num, codes, plan, X, y = _small(api, orc, C)
    y[[700, 900]] = bad
    dn, dc = dev(num), dev(codes)
    with pytest.raises(_lib.DlsaError) as ex:
        engine.onehot_multinomial_fit_ex(plan, dn, dc, dev(y), [0, 600], [600, 600], classes=C)
    assert ex.value.code == 1 and "partition 1 has 2 rows whose response is not a class code 0 .. 2" in str(ex.value)
    # the pass answers with loglik = NaN and checks nothing else
    assert math.isnan(float(engine.onehot_multinomial_pass(plan, dn, dc, dev(y), dev(np.zeros(2 * p)), C, want_H=False)[2].item()))
    # the first partition alone fits
    assert engine.onehot_multinomial_fit_ex(plan, dn, dc, dev(y), [0], [600], classes=C)["status"] == [0]


def test_a_partition_that_lacks_a_class_is_refused(api, orc):
    from dlsa_amd import engine, _lib
    C = 4
    p, num, codes, plan, X, y = _small(api, orc, C, n=1800, seed=63)
    y[600:1200][y[600:1200] == 2] = 1.0
    with pytest.raises(_lib.DlsaError) as ex:
        engine.onehot_multinomial_fit_ex(plan, dev(num), dev(codes), dev(y), [0, 600, 1200], [600] * 3, classes=C)
    assert ex.value.code == 1 and "partition 1 has no row of class 2" in str(ex.value)


@pytest.mark.parametrize("classes,nlevels,text", [(1, (4, 3), "classes must lie in 2 .. 8"), (9, (4, 3), "classes must lie in 2 .. 8"),
                                                  (8, (300,), "exceed the solver's 2048")])
def test_class_count_and_dimension_are_refused(api, orc, classes, nlevels, text):
    from dlsa_amd import engine, _lib
    rng = np.random.default_rng(64)
    n, q = 50, 2
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels)
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc, dy = dev(num), dev(codes), dev(np.zeros(n))
    td = torch.zeros(max(1, classes - 1) * p, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=text):
        engine.onehot_multinomial_pass(plan, dn, dc, dy, td, classes)
    with pytest.raises(ValueError, match=text):
        engine.onehot_multinomial_fit_ex(plan, dn, dc, dy, [0], [n], classes=classes)
    # the C ABI's own check, below the Python one
    lib = _lib.load()
    assert lib.dlsa_onehot_multinomial_workspace_bytes(plan._h, n, classes, 1) == 0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    g = torch.empty(td.numel(), dtype=torch.float64, device="cuda")
    rc = lib.dlsa_onehot_multinomial_pass_f64(plan._h, dn.data_ptr(), q, dc.data_ptr(), len(nlevels), dy.data_ptr(), td.data_ptr(), classes, n,
                                              None, 0, g.data_ptr(), None, None, 0, ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and text in _lib.last_error()
    first, rows = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(n)
    rc = lib.dlsa_onehot_multinomial_fit_f64(plan._h, dn.data_ptr(), q, dc.data_ptr(), len(nlevels), dy.data_ptr(), first, rows, 1, 1, classes,
                                             1e-13, 100, g.data_ptr(), g.data_ptr(), g.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(),
                                             None)
    assert rc == 1 and text in _lib.last_error()


def test_null_num_short_workspace_and_empty_partition(api, orc):
    from dlsa_amd import engine, _lib
    C = 3
    p, num, codes, plan, X, y = _small(api, orc, C)
    n = len(y)
    dn, dc, dy = dev(num), dev(codes), dev(y)
    lib = _lib.load()
    td = torch.zeros(2 * p, dtype=torch.float64, device="cuda")
    g = torch.empty(2 * p, dtype=torch.float64, device="cuda")
    need = lib.dlsa_onehot_multinomial_workspace_bytes(plan._h, n, C, 1)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    args = [plan._h, dn.data_ptr(), 2, dc.data_ptr(), 2, dy.data_ptr(), td.data_ptr(), C, n, None, 0, g.data_ptr(), None, None, 0, ws.data_ptr(),
            ws.numel(), None]
    a = list(args); a[1] = None                                  # a null num on a plan with numerics
    assert lib.dlsa_onehot_multinomial_pass_f64(*a) == 1 and "null num" in _lib.last_error()
    a = list(args); a[16] = need - 256                           # a short workspace
    assert lib.dlsa_onehot_multinomial_pass_f64(*a) == 3 and "workspace" in _lib.last_error()
    assert lib.dlsa_onehot_multinomial_pass_f64(*args) == 0
    first, rows = (ctypes.c_int64 * 2)(0, 600), (ctypes.c_int64 * 2)(600, 600)
    out = torch.empty(2 * (2 * p) * (2 * p), dtype=torch.float64, device="cuda")
    fneed = lib.dlsa_onehot_multinomial_workspace_bytes(plan._h, 600, C, 1)
    fws = torch.empty(fneed, dtype=torch.uint8, device="cuda")
    fargs = [plan._h, dn.data_ptr(), 2, dc.data_ptr(), 2, dy.data_ptr(), first, rows, 1, 2, C, 1e-13, 100, out.data_ptr(), out.data_ptr(),
             out.data_ptr(), None, None, None, fws.data_ptr(), 1024, None]
    assert lib.dlsa_onehot_multinomial_fit_f64(*fargs) == 3 and "workspace" in _lib.last_error()
    a = list(fargs); a[1] = None; a[20] = fneed
    assert lib.dlsa_onehot_multinomial_fit_f64(*a) == 1 and "null num" in _lib.last_error()
    with pytest.raises(ValueError, match="classes"):
        engine.onehot_multinomial_fit_ex(plan, dn, dc, dy, [0], [n])
    # an empty partition: the zero block and DLSA_PART_EMPTY, its neighbours fit
    r = engine.onehot_multinomial_fit_ex(plan, dn, dc, dy, [0, 600, 600], [600, 0, 600], classes=C)
    assert r["status"] == [0, 4, 0] and r["rc"] == 0 and r["n_iter"][1] == 0 and r["loglik"][1] == 0.0
    assert not r["coef"][1].any() and not r["Sig_inv"][1].any() and not r["Sig_invMcoef"][1].any()
    b, H, _, _ = _ref_fit(X[600:], y[600:], C, 0)
    assert rel(r["coef"][2].cpu().numpy(), b) <= TOL_FIT and rel(r["Sig_inv"][2].cpu().numpy(), H) <= TOL_FIT


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_end_to_end_dlsa(api, orc):
    n, q, nlevels, K, C = 40_000, 2, (6, 4), 4, 3
    p, num, codes, desc, nl, level_col, X, y = _fit_case(orc, n, q, nlevels, 90, C)
    _assert_rows(X, y, [slice(k, n, K) for k in range(K)], C)
    spec = _spec(api, q, nlevels, desc)
    mb = api.fit_multinomial_design(dev(num), dev(codes), dev(y), spec, C, partition_num=K)
    assert mb.status == [0] * K and mb.names == api.multinomial_column_names(spec.names, C)
    out = api.dlsa_mapred(mb)
    blocks = []
    for k in range(K):
        b, S, _, _ = _ref_fit(X[k::K], y[k::K], C, 0)
        blocks.append((b, S, S @ b))
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[2] for b in blocks], [b[1] for b in blocks])
    figs = (rel(out["beta_byOLS"].to_numpy(), ols), rel(out["beta_byONESHOT"].to_numpy(), oneshot), rel(out.iloc[:, 2:].to_numpy(), S))
    print("end to end: rel err WLS %.2e one-shot %.2e Sig_inv %.2e" % figs)
    assert max(figs) <= TOL_FIT


def test_multinomial_model_structured_frame_and_eval(api):
    import pandas as pd
    rng = np.random.default_rng(2)
    n, labels = 6000, ["a", "b", "c"]
    df = pd.DataFrame({"y": "a", "dist": rng.normal(5.0, 2.0, n), "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2]),
                       "region": rng.choice(["n", "s", "e", "w"], n)})
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC", df["region"] == "n", df["region"] == "s",
                          df["region"] == "w"]).astype(float)
    truth = np.array([-0.3, 0.1, 0.4, 0.0, 0.2, -0.1, 0.3, 0.3, -0.1, 0.0, 0.5, -0.2, 0.1, 0.0])
    cls = mr.draw(rng, Xo, truth, 3, True)
    df["y"] = [labels[int(c)] for c in cls]
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"], "region": ["e", "n", "s", "w"]},
                  "factor_dropped": {"carrier": [], "region": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"],
                                            "region": ["region_e", "region_n", "region_s", "region_w"]}}
    baseline = ["carrier_AA", "region_e"]
    base = ["intercept", "dist", "carrier_BB", "carrier_CC", "region_n", "region_s", "region_w"]
    names = [nm + ":1" for nm in base] + [nm + ":2" for nm in base]
    want = ["par_id", "coef", "Sig_invMcoef"] + names
    kw = dict(fit_intercept=True, dummy_info=dummy_info, dummy_factors_baseline=baseline)
    out = api.multinomial_model(df, "y", labels, structured=True, **kw)
    dense = api.multinomial_model(df, "y", labels, structured=False, **kw)
    default = api.multinomial_model(df, "y", labels, **kw)
    assert list(out.columns) == want and list(dense.columns) == want
    assert default.to_numpy().tobytes() == dense.to_numpy().tobytes()      # the default is the dense path
    figs = (rel(out["coef"], dense["coef"]), rel(out[names].to_numpy(), dense[names].to_numpy()), rel(out["Sig_invMcoef"], dense["Sig_invMcoef"]))
    print("multinomial_model structured vs dense: coef %.2e Sig_inv %.2e Sig_invMcoef %.2e" % figs)
    assert max(figs) <= TOL_FIT
    # a missing level: the zero block of J p names and the reference's warning, from the codes
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = api.multinomial_model(sub, "y", labels, structured=True, **kw)
    assert any("missing in this data chunk" in str(w.message) and "Skip modeling" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (14, 17) and float(np.abs(zero.to_numpy()).max()) == 0.0
    # eval: the log-likelihood of each estimator column against the reference
    par = pd.DataFrame({"mle": out["coef"].to_numpy(), "away": mr.away_from_optimum(14)})
    ev = api.multinomial_model_eval(df, "y", par, labels, structured=True, **kw)
    assert list(ev.columns) == ["mle", "away"] and ev.shape == (1, 2)
    refs = [mr.terms(Xo, cls, par[c].to_numpy(), 3, True)[0] for c in par.columns]
    print("multinomial_model_eval structured vs reference %.2e" % rel(ev.to_numpy()[0], refs))
    assert rel(ev.to_numpy()[0], refs) <= TOL_PASS
    evd = api.multinomial_model_eval(df, "y", par, labels, structured=False, **kw)
    ev0 = api.multinomial_model_eval(df, "y", par, labels, **kw)
    assert ev0.to_numpy().tobytes() == evd.to_numpy().tobytes()
