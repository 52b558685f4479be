"""GPU: the structured one-hot ordinal map step (csrc/onehot_ordinal.hip) -- the proportional-odds pass and fit on raw numerics +
level codes under a plan without a constant column -- against the numpy reference (tests/ordinal_reference.py) on the dense matrix
oracle.dlsa_oracle.design_matrix builds: the pass at a fixed theta (loglik, g, H as a whole and its corner, border and beta-beta
parts, w) on both border routes and with 8, 4, 2 and 1 histogram copies, nullable outputs and a padded pitch, the extreme case, the
NaN cases, the per-partition fit on both routes, structured = dense, strided = contiguous, two classes = the structured logistic
fit, reproducibility, statuses, refusals, the frame level and the end-to-end DLSA combine with unpenalised cutpoints.

Bars: relative l-inf 1e-12 for a pass and 1e-10 for a fit (tests/onehot_ordinal_cases.py), every figure printed before it is
asserted.  The masked-route fit (20000 rows, 500 uniform levels, C = 8, seed 7): for a draw of this shape the fp64 reference was
reported to differ from its longdouble run by coef 3.0e-14, Sig_inv 1.1e-15, Sig_invMcoef 4.3e-15, loglik 6.5e-17 (a ten-minute
run, quoted from the feature's issue, not a test and not repeated on this file's draw), three orders below the fit bar; this
file's draw (tests/onehot_ordinal_cases.py: 5 evaluations, at least 24 rows per column, condition 1.1e6) was seen at coef 1.3e-14,
Sig_inv 2.0e-16, Sig_invMcoef 2.0e-15 against the fp64 reference."""
import ctypes
import math
import warnings

import numpy as np
import pytest

import lars_unpenalized_reference as ur
import onehot_ordinal_cases as cs
import ordinal_reference as orf
from test_gpu_onehot import _plan
from test_gpu_onehot_poisson import _spec, dev, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL_PASS, TOL_FIT = cs.TOL_PASS, cs.TOL_FIT


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import dlsa_amd
    return dlsa_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import dlsa_oracle
    return dlsa_oracle


def _figures(out, ref, J):
    """relative errors of (loglik, g, H, corner, border, beta-beta part, w) against the reference's terms"""
    H, g, ll, w = out
    llr, gr, Hr, wr = ref
    Hn = H.cpu().numpy()
    return Hn, {"ll": abs(float(ll.item()) - llr) / abs(llr), "g": rel(g.cpu().numpy(), gr), "H": rel(Hn, Hr),
                "corner": rel(Hn[:J, :J], Hr[:J, :J]), "border": rel(Hn[:J, J:], Hr[:J, J:]), "bb": rel(Hn[J:, J:], Hr[J:, J:]),
                "w": rel(w.cpu().numpy(), wr)}


def _check_pass(plan, num, codes, y, theta, C, X, tag=None):
    """structured pass == the reference on the dense matrix X; H equal to its transpose bit for bit"""
    from dlsa_amd import engine
    q, J, p = num.shape[1], C - 1, X.shape[1]
    out = engine.onehot_ordinal_pass(plan, dev(num) if q else None, dev(codes), dev(y), dev(theta), C, want_w=True)
    ref = orf.terms(X, y, theta, C)
    Hn, figs = _figures(out, ref, J)
    print("pass", tag, "p", p, "route", cs.lds_route(p, C), " ".join("%s %.2e" % kv for kv in figs.items()))
    assert math.isfinite(ref[0]) and np.all(np.isfinite(ref[2])) and np.all(np.isfinite(ref[1]))
    assert Hn.shape == (J + p, J + p) and out[3].shape == (len(y),)
    assert all(np.isfinite(v) and v <= TOL_PASS for v in figs.values()), figs
    assert np.array_equal(Hn, Hn.T)
    return out


def _pass_inputs(api, orc, n, q, nlevels, C, baseline, seed=None):
    rng = np.random.default_rng(n + q if seed is None else seed)
    p, num, codes, desc, nl, level_col = cs.design(rng, n, q, nlevels, baseline)
    codes[rng.integers(0, n, max(1, n // 50)), 0] = -1          # unknown level: no column
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    theta = cs.pass_theta(rng, p, C)
    y = orf.draw(rng, X, theta, C)
    return plan, num, codes, y, theta, X


@pytest.mark.parametrize("n,q,nlevels,C,baseline", cs.PASS_CASES)
def test_pass_matches_reference(api, orc, n, q, nlevels, C, baseline):
    plan, num, codes, y, theta, X = _pass_inputs(api, orc, n, q, nlevels, C, baseline)
    if nlevels[:2] == (110, 110):
        assert plan.roles >= 2                                  # several Gram roles
    _check_pass(plan, num, codes, y, theta, C, X, (n, q, nlevels, C, baseline))


@pytest.mark.parametrize("n,q,nlevels", [(30000, 2, (300, 300)), (4000, 3, (110, 110, 20, 6))])
def test_pass_with_row_banded_tables_and_several_roles(api, orc, n, q, nlevels):
    C = 3
    plan, num, codes, y, theta, X = _pass_inputs(api, orc, n, q, nlevels, C, True, seed=n + 1)
    assert plan.roles >= 2
    _check_pass(plan, num, codes, y, theta, C, X, (n, q, nlevels, C))


def test_pass_with_unordered_adds(api, orc):
    """onehot_ordered=0: all waves add at once, last bits vary from run to run -- against the reference only."""
    from dlsa_amd import engine
    n, q, nlevels, C = 777, 7, (40, 40, 9, 2), 5
    plan, num, codes, y, theta, X = _pass_inputs(api, orc, n, q, nlevels, C, True)
    with engine.kernel_options(onehot_ordered=0):
        _check_pass(plan, num, codes, y, theta, C, X, (n, q, nlevels, "unordered"))


@pytest.mark.parametrize("n,q,nlevels,C", [(3001, 2, (3,), 3), (3000, 0, (700, 8, 3), 5)])     # in-pass borders, the masked route
def test_nullable_outputs_and_padded_pitch(api, orc, n, q, nlevels, C):
    """each nullable output left out in turn (direct calls: the wrapper always asks for g and loglik), then ldh = d + 3 into a
    sentinel-filled buffer: the same bits in the d x d block, the pad columns untouched"""
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _stream
    lib = _lib.load()
    plan, num, codes, y, theta, X = _pass_inputs(api, orc, n, q, nlevels, C, True)
    J, p = C - 1, X.shape[1]
    d = J + p
    assert cs.lds_route(p, C)[0] == (C == 3)
    dn, dc, dy, dt = (dev(num) if q else None), dev(codes), dev(y), dev(theta)
    ref = orf.terms(X, y, theta, C)
    ws = torch.empty(lib.dlsa_onehot_ordinal_workspace_bytes(plan._h, n, C, 1), dtype=torch.uint8, device="cuda")

    def run(want, ldh=d):
        new = lambda *s: torch.full(s, -7.25, dtype=torch.float64, device="cuda")
        H, g, ll, w = new(d, ldh), new(d), new(1), new(n)
        got = [t if k in want else None for k, t in zip("Hglw", (H, g, ll, w))]
        rc = lib.dlsa_onehot_ordinal_pass_f64(plan._h, _ptr(dn), q, _ptr(dc), len(nlevels), _ptr(dy), _ptr(dt), C, n, _ptr(got[0]), ldh,
                                              _ptr(got[1]), _ptr(got[2]), _ptr(got[3]), _ptr(ws), ws.numel(), _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        return got
    full = run("Hglw")
    Hn, figs = _figures(full, ref, J)
    print("all outputs", (n, q, nlevels, C), figs)
    assert max(figs.values()) <= TOL_PASS
    for left_out in "Hglw":
        got = run("Hglw".replace(left_out, ""))
        for k, t, r, scale in zip("Hglw", got, (ref[2], ref[1], ref[0], ref[3]), (ref[2], ref[1], ref[0], ref[3])):
            if t is not None:
                err = rel(t.cpu().numpy().reshape(np.shape(r)), r)
                print("without", left_out, k, "%.2e" % err)
                assert err <= TOL_PASS, (left_out, k, err)
    # (with H the g set's histogram copies differ from a pass without: g agrees to rounding, not to the bit; with H both times it does)
    again = run("Hglw")
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    padded = run("Hglw", ldh=d + 3)
    assert torch.equal(padded[0][:, :d], full[0]) and bool((padded[0][:, d:] == -7.25).all())
    assert torch.equal(padded[1], full[1]) and torch.equal(padded[2], full[2]) and torch.equal(padded[3], full[3])


def test_extreme_case_is_finite_and_within_the_bar(api, orc):
    """|u|, |l| reach 600 and two cutpoints are 1e-6 apart (cs.extreme_case; the fp64 reference itself is checked against longdouble
    on the CPU in tests/test_onehot_ordinal_cpu.py)"""
    p, num, codes, desc, nl, level_col, y, theta = cs.extreme_case()
    C = cs.EXTREME_CLASSES
    plan = _plan(api, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    H, g, ll, w = _check_pass(plan, num, codes, y, theta, C, X, "extreme")
    assert math.isfinite(float(ll.item())) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(H).all()) and bool(torch.isfinite(w).all())


def test_unordered_cutpoints_and_bad_responses_give_nan(api, orc):
    from dlsa_amd import engine
    n, q, nlevels, C = 3001, 2, (3,), 5
    plan, num, codes, y, theta, X = _pass_inputs(api, orc, n, q, nlevels, C, True)
    dn, dc = dev(num), dev(codes)
    bad = theta.copy()
    bad[[C - 3, C - 2]] = bad[[C - 2, C - 3]]
    assert math.isnan(float(engine.onehot_ordinal_pass(plan, dn, dc, dev(y), dev(bad), C)[2].item()))
    bad = theta.copy()
    bad[1] = bad[0]                                             # equal cutpoints are not strictly increasing either
    assert math.isnan(float(engine.onehot_ordinal_pass(plan, dn, dc, dev(y), dev(bad), C)[2].item()))
    for value in (float("nan"), 7.5):
        yb = y.copy()
        yb[[5, 1700]] = value
        assert math.isnan(float(engine.onehot_ordinal_pass(plan, dn, dc, dev(yb), dev(theta), C)[2].item()))
    assert math.isfinite(float(engine.onehot_ordinal_pass(plan, dn, dc, dev(y), dev(theta), C)[2].item()))


# ---- fit ----------------------------------------------------------------------------------------------------------------
def _check_fit(r, fits, K, what):
    assert r["status"] == [0] * K and r["rc"] == 0, (r["status"], r["rc"])
    for k, (b, H, ll, evals, halvings) in enumerate(fits):
        figs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H),
                rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b), abs(r["loglik"][k] - ll) / abs(ll))
        print("fit", what, "partition", k, "rel err coef %.2e Sig_inv %.2e Sig_invMcoef %.2e loglik %.2e" % figs, "evaluations", r["n_iter"][k],
              "reference", evals)
        assert max(figs) <= TOL_FIT, (k, figs)
        assert r["n_iter"][k] == evals, (k, r["n_iter"][k], evals)
        Sn = r["Sig_inv"][k].cpu().numpy()
        assert np.array_equal(Sn, Sn.T)


@pytest.mark.parametrize("case", cs.FIT_CASES + [cs.MASKED_FIT_CASE], ids=lambda c: "%d-%s-C%d-K%d" % (c[0], "x".join(map(str, c[2])), c[3], c[4]))
def test_fit_matches_reference(api, case):
    from dlsa_amd import engine
    n, q, nlevels, C, K, strided, seed, freq = case
    (p, num, codes, desc, nl, level_col, X, y), fits = cs.fit_reference(case)
    assert cs.lds_route(p, C)[0] == (case != cs.MASKED_FIT_CASE)
    _, first, rows, step = cs.parts(n, K, strided)
    plan = _plan(api, p, desc, nl, level_col)
    r = engine.onehot_ordinal_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step, classes=C)
    _check_fit(r, fits, K, case)


def test_structured_equals_dense_and_strided_equals_contiguous(api, orc):
    case = cs.FIT_CASES[1]                                      # K = 6 strided
    n, q, nlevels, C, K = case[:5]
    (p, num, codes, desc, nl, level_col, X, y), _ = cs.fit_reference(case)
    spec = _spec(api, q, nlevels, desc)
    assert spec.onehot_plan() is not None
    names = api.ordinal_column_names(spec.names, C)
    assert len(names) == C - 1 + p and names[0] == "intercept:1" and names[C - 1] == spec.names[0]
    dn, dc, dy = dev(num), dev(codes), dev(y)
    a = api.fit_ordinal_design(dn, dc, dy, spec, C, partition_num=K)
    d = api.fit_ordinal_design(dn, dc, dy, spec, C, partition_num=K, structured=False)
    assert a.status == [0] * K and d.status == [0] * K and a.names == names and d.names == names
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):
        err = rel(getattr(a, f).cpu().numpy(), getattr(d, f).cpu().numpy())
        print("structured vs dense", f, "%.2e" % err)
        assert err <= TOL_FIT
    print("structured vs dense loglik %.2e" % rel(a.loglik, d.loglik), "evaluations", a.n_iter, d.n_iter)
    assert rel(a.loglik, d.loglik) <= TOL_FIT
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    c = api.fit_ordinal_design(dev(num[perm]), dev(codes[perm]), dev(y[perm]), spec, C, part_offsets=offs)
    assert c.status == [0] * K and c.n_iter == a.n_iter
    for f in ("coef", "Sig_inv", "Sig_invMcoef"):                 # the same rows in the same order: the same bits
        assert torch.equal(getattr(a, f), getattr(c, f)), f
    assert list(a.loglik) == list(c.loglik)


def test_two_classes_equal_the_structured_logistic_fit(api, orc):
    """C = 2 on a plan without a constant column == onehot_irls_fit_ex on the same plan plus one, theta = [-intercept | beta]"""
    from dlsa_amd import engine
    n, q, nlevels, K, C = 20_000, 2, (6, 4), 4, 2
    p, num, codes, desc, nl, level_col, X, y = cs.fit_case(orc.design_matrix, n, q, nlevels, 22, C)
    _, first, rows, step = cs.parts(n, K, True)
    plan = _plan(api, p, desc, nl, level_col)
    a = engine.onehot_ordinal_fit_ex(plan, dev(num), dev(codes), dev(y), first, rows, row_step=step, classes=2)
    # the same columns behind a constant column 0
    kind, src, level, shift, scale = desc
    desc1 = tuple(np.concatenate([[v0], v]).astype(v.dtype) for v0, v in zip((0, 0, 0, 0.0, 1.0), desc))
    plan1 = _plan(api, p + 1, desc1, nl, [c + 1 if c >= 0 else -1 for c in level_col])
    b = engine.onehot_irls_fit_ex(plan1, dev(num), dev(codes), dev(y), first, rows, row_step=step)
    assert a["status"] == [0] * K and b["status"] == [0] * K
    sgn = np.ones(p + 1)
    sgn[0] = -1.0
    for f, flip in (("coef", sgn), ("Sig_inv", sgn[:, None] * sgn[None, :]), ("Sig_invMcoef", sgn)):
        err = rel(a[f].cpu().numpy(), b[f].cpu().numpy() * flip)
        print("two classes vs the structured logistic fit", f, "%.2e" % err)
        assert err <= TOL_FIT


def test_pass_and_fit_are_bit_reproducible(api, orc):
    from dlsa_amd import engine
    case = cs.FIT_CASES[2]
    n, q, nlevels, C, K = case[:5]
    (p, num, codes, desc, nl, level_col, X, y), _ = cs.fit_reference(case)
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc, dy = dev(num), dev(codes), dev(y)
    theta = dev(cs.pass_theta(np.random.default_rng(81), p, C))
    one = engine.onehot_ordinal_pass(plan, dn, dc, dy, theta, C, want_w=True)
    two = engine.onehot_ordinal_pass(plan, dn, dc, dy, theta, C, want_w=True)
    assert all(torch.equal(u, v) for u, v in zip(one, two))
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    a = engine.onehot_ordinal_fit_ex(plan, dn, dc, dy, first, rows, row_step=K, classes=C)
    b = engine.onehot_ordinal_fit_ex(plan, dn, dc, dy, first, rows, row_step=K, classes=C)
    assert a["status"] == [0] * K
    assert torch.equal(a["coef"], b["coef"]) and torch.equal(a["Sig_inv"], b["Sig_inv"]) and torch.equal(a["Sig_invMcoef"], b["Sig_invMcoef"])
    assert a["loglik"] == b["loglik"] and a["n_iter"] == b["n_iter"]


def test_statuses_empty_partition_and_all_levels_kept(api, orc):
    from dlsa_amd import engine
    case = cs.FIT_CASES[0]
    n, q, nlevels, C = case[:4]
    (p, num, codes, desc, nl, level_col, X, y), _ = cs.fit_reference(case)
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc, dy = dev(num), dev(codes), dev(y)
    r = engine.onehot_ordinal_fit_ex(plan, dn, dc, dy, [0, 3000, 3000], [3000, 0, 3000], classes=C)
    assert r["status"] == [0, 4, 0] and r["rc"] == 0 and r["n_iter"][1] == 0 and r["loglik"][1] == 0.0
    assert not r["coef"][1].any() and not r["Sig_inv"][1].any() and not r["Sig_invMcoef"][1].any()
    b, H = orf.fit(X[3000:], y[3000:], C)[:2]
    assert rel(r["coef"][2].cpu().numpy(), b) <= TOL_FIT and rel(r["Sig_inv"][2].cpu().numpy(), H) <= TOL_FIT
    # every level of a factor kept: collinear with the cutpoints -- legal in a pass, NOT_SPD in a fit, as in the dense fit
    rng = np.random.default_rng(5)
    pk, numk, codesk, desck, nlk, lck = cs.design(rng, n, q, nlevels, baseline=False)
    Xk, _ = orc.design_matrix(numk, codesk, *desck)
    plank = _plan(api, pk, desck, nlk, lck)
    theta = cs.pass_theta(rng, pk, C)
    yk = orf.draw(rng, Xk, theta, C)
    _check_pass(plank, numk, codesk, yk, theta, C, Xk, "all levels kept")
    s = engine.onehot_ordinal_fit_ex(plank, dev(numk), dev(codesk), dev(yk), [0], [n], classes=C)
    dense = engine.ordinal_fit_ex(dev(Xk), dev(yk), [0], [n], classes=C)
    print("all levels kept: structured status", s["status"], "dense status", dense["status"])
    assert s["status"] == dense["status"] == [2]                # DLSA_PART_NOT_SPD


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _small(api, orc, C=3, n=1200, seed=61):
    p, num, codes, desc, nl, level_col, X, y = cs.fit_case(orc.design_matrix, n, 2, (4, 3), seed, C)
    return p, num, codes, _plan(api, p, desc, nl, level_col), X, y


def test_a_plan_with_a_constant_column_is_refused(api, orc):
    from dlsa_amd import engine, _lib
    from test_gpu_onehot import _random_design
    rng = np.random.default_rng(3)
    n, C = 500, 3
    p, num, codes, desc, nl, level_col = _random_design(rng, n, 2, (4, 3))            # with its constant column
    plan = _plan(api, p, desc, nl, level_col)
    assert _lib.load().dlsa_onehot_ordinal_workspace_bytes(plan._h, n, C, 1) == 0
    y = dev(rng.integers(0, C, n).astype(np.float64))
    with pytest.raises(_lib.DlsaError) as ex:
        engine.onehot_ordinal_pass(plan, dev(num), dev(codes), y, dev(np.concatenate([[-1.0, 1.0], np.zeros(p)])), C)
    assert ex.value.code == 1 and "onehot_ordinal_pass" in str(ex.value) and "constant column" in str(ex.value)
    with pytest.raises(_lib.DlsaError) as ex:
        engine.onehot_ordinal_fit_ex(plan, dev(num), dev(codes), y, [0], [n], classes=C)
    assert ex.value.code == 1 and "onehot_ordinal_fit" in str(ex.value) and "constant column" in str(ex.value)
    # the frame-level entry refuses the spec before it builds anything
    spec = _spec(api, 2, (4, 3), desc)
    with pytest.raises(ValueError, match="constant column"):
        api.fit_ordinal_design(dev(num), dev(codes), y, spec, C)


@pytest.mark.parametrize("bad", [1.5, -1.0, 3.0, float("nan")])
def test_a_response_that_is_no_class_code_is_refused(api, orc, bad):
    from dlsa_amd import engine, _lib
    C = 3
    p, num, codes, plan, X, y = _small(api, orc, C)
    y[[700, 900]] = bad
    dn, dc = dev(num), dev(codes)
    with pytest.raises(_lib.DlsaError) as ex:
        engine.onehot_ordinal_fit_ex(plan, dn, dc, dev(y), [0, 600], [600, 600], classes=C)
    assert ex.value.code == 1 and "onehot_ordinal_fit: partition 1 has 2 rows whose response is not a class code 0 .. 2" in str(ex.value)
    assert engine.onehot_ordinal_fit_ex(plan, dn, dc, dev(y), [0], [600], classes=C)["status"] == [0]      # the first partition alone fits


def test_a_partition_that_lacks_a_class_is_refused(api, orc):
    from dlsa_amd import engine, _lib
    C = 4
    p, num, codes, plan, X, y = _small(api, orc, C, n=1800, seed=63)
    y[600:1200][y[600:1200] == 2] = 1.0
    with pytest.raises(_lib.DlsaError) as ex:
        engine.onehot_ordinal_fit_ex(plan, dev(num), dev(codes), dev(y), [0, 600, 1200], [600] * 3, classes=C)
    assert ex.value.code == 1 and "partition 1 has no row of class 2" in str(ex.value)


def test_too_many_coefficients_are_refused(api, orc):
    """J + p = 2049: p = 2042 at C = 8"""
    from dlsa_amd import engine, _lib
    rng = np.random.default_rng(64)
    n, q, nlevels, C = 50, 2, (2041,), 8
    p, num, codes, desc, nl, level_col = cs.design(rng, n, q, nlevels)
    assert C - 1 + p == 2049
    plan = _plan(api, p, desc, nl, level_col)
    dn, dc, dy = dev(num), dev(codes), dev(np.zeros(n))
    td = torch.zeros(C - 1 + p, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="exceed the solver's 2048"):
        engine.onehot_ordinal_pass(plan, dn, dc, dy, td, C)
    with pytest.raises(ValueError, match="exceed the solver's 2048"):
        engine.onehot_ordinal_fit_ex(plan, dn, dc, dy, [0], [n], classes=C)
    lib = _lib.load()                                           # the C ABI's own check, below the Python one
    assert lib.dlsa_onehot_ordinal_workspace_bytes(plan._h, n, C, 1) == 0 and lib.dlsa_onehot_ordinal_workspace_bytes(plan._h, n, C - 1, 1) > 0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = lib.dlsa_onehot_ordinal_pass_f64(plan._h, dn.data_ptr(), q, dc.data_ptr(), 1, dy.data_ptr(), td.data_ptr(), C, n, None, 0, td.data_ptr(),
                                          None, None, ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and "exceed the solver's 2048" in _lib.last_error()
    first, rows = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(n)
    rc = lib.dlsa_onehot_ordinal_fit_f64(plan._h, dn.data_ptr(), q, dc.data_ptr(), 1, dy.data_ptr(), first, rows, 1, 1, C, 1e-13, 100,
                                         td.data_ptr(), td.data_ptr(), td.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and "exceed the solver's 2048" in _lib.last_error()


# ---- frame level and end to end ---------------------------------------------------------------------------------------------
def test_ordinal_model_structured_frame_and_eval(api):
    import pandas as pd
    rng = np.random.default_rng(2)
    n, labels = 6000, ["low", "mid", "high"]
    df = pd.DataFrame({"y": "low", "dist": rng.normal(5.0, 2.0, n), "carrier": rng.choice(["AA", "BB", "CC"], n, p=[0.5, 0.3, 0.2]),
                       "region": rng.choice(["n", "s", "e", "w"], n)})
    Xo = np.column_stack([df["dist"], df["carrier"] == "BB", df["carrier"] == "CC", df["region"] == "n", df["region"] == "s",
                          df["region"] == "w"]).astype(float)
    truth = np.array([0.5, 2.0, 0.3, 0.4, -0.2, 0.2, -0.1, 0.3])
    cls = orf.draw(rng, Xo, truth, 3)
    df["y"] = [labels[int(c)] for c in cls]
    dummy_info = {"factor_selected": {"carrier": ["AA", "BB", "CC"], "region": ["e", "n", "s", "w"]},
                  "factor_dropped": {"carrier": [], "region": []},
                  "factor_selected_names": {"carrier": ["carrier_AA", "carrier_BB", "carrier_CC"],
                                            "region": ["region_e", "region_n", "region_s", "region_w"]}}
    baseline = ["carrier_AA", "region_e"]
    names = ["intercept:1", "intercept:2", "dist", "carrier_BB", "carrier_CC", "region_n", "region_s", "region_w"]
    want = ["par_id", "coef", "Sig_invMcoef"] + names
    kw = dict(dummy_info=dummy_info, dummy_factors_baseline=baseline)
    out = api.ordinal_model(df, "y", labels, structured=True, **kw)
    dense = api.ordinal_model(df, "y", labels, structured=False, **kw)
    default = api.ordinal_model(df, "y", labels, **kw)
    assert list(out.columns) == want and list(dense.columns) == want
    assert default.to_numpy().tobytes() == dense.to_numpy().tobytes()      # the default is the dense path
    figs = (rel(out["coef"], dense["coef"]), rel(out[names].to_numpy(), dense[names].to_numpy()), rel(out["Sig_invMcoef"], dense["Sig_invMcoef"]))
    print("ordinal_model structured vs dense: coef %.2e Sig_inv %.2e Sig_invMcoef %.2e" % figs)
    assert max(figs) <= TOL_FIT
    # a missing level: the zero block of J + p names and the reference's warning, from the codes
    sub = df[df["carrier"] != "CC"].reset_index(drop=True)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        zero = api.ordinal_model(sub, "y", labels, structured=True, **kw)
    assert any("missing in this data chunk" in str(w.message) and "Skip modeling" in str(w.message) for w in wlist)
    assert list(zero.columns) == want and zero.shape == (8, 11) and float(np.abs(zero.to_numpy()).max()) == 0.0
    # eval: the log-likelihood of each estimator column, structured against dense and against the reference
    par = pd.DataFrame({"mle": out["coef"].to_numpy(), "away": orf.away_from_optimum(6, 3)})
    ev = api.ordinal_model_eval(df, "y", par, labels, structured=True, **kw)
    evd = api.ordinal_model_eval(df, "y", par, labels, structured=False, **kw)
    ev0 = api.ordinal_model_eval(df, "y", par, labels, **kw)
    assert list(ev.columns) == ["mle", "away"] and ev.shape == (1, 2) and ev0.to_numpy().tobytes() == evd.to_numpy().tobytes()
    print("ordinal_model_eval structured vs dense %.2e" % rel(ev.to_numpy()[0], evd.to_numpy()[0]))
    assert rel(ev.to_numpy()[0], evd.to_numpy()[0]) <= TOL_PASS


def test_end_to_end_dlsa_with_unpenalised_cutpoints(api, orc):
    """fit_ordinal_design -> dlsa_mapred -> dlsa(unpenalized="intercepts") against the same pipeline on the reference's blocks, at the
    bars of the dense family's end-to-end test (1e-10 for the combine, 1e-8 for the path); the cutpoints are never shrunk"""
    case = cs.FIT_CASES[1]
    n, q, nlevels, C, K = case[:5]
    (p, num, codes, desc, nl, level_col, X, y), fits = cs.fit_reference(case)
    spec = _spec(api, q, nlevels, desc)
    mb = api.fit_ordinal_design(dev(num), dev(codes), dev(y), spec, C, partition_num=K)
    names = api.ordinal_column_names(spec.names, C)
    assert mb.status == [0] * K and mb.names == names
    out = api.dlsa_mapred(mb)
    ols, oneshot, S = orc.dlsa_mapred_blocks([f[0] for f in fits], [f[1] @ f[0] for f in fits], [f[1] for f in fits])
    figs = (rel(out["beta_byOLS"].to_numpy(), ols), rel(out["beta_byONESHOT"].to_numpy(), oneshot), rel(out.iloc[:, 2:].to_numpy(), S))
    print("end to end: rel err WLS %.2e one-shot %.2e Sig_inv %.2e" % figs)
    assert max(figs) <= TOL_FIT
    U = api.intercept_columns(names)
    assert U == list(range(C - 1))
    res = api.dlsa(out.iloc[:, 2:], out["beta_byOLS"], n, unpenalized="intercepts")
    r = ur.path(S, ols, U, n, "lar")
    by_aic, by_bic = r["theta"][int(np.argmin(r["AIC"]))], r["theta"][int(np.argmin(r["BIC"]))]
    ea, eb = rel(res["beta_byAIC"].to_numpy(), by_aic), rel(res["beta_byBIC"].to_numpy(), by_bic)
    print("end to end: AIC point %.1e BIC point %.1e" % (ea, eb))
    assert ea <= 1e-8 and eb <= 1e-8
    assert np.all(res["beta_byBIC"].to_numpy()[U] != 0) and np.all(res["beta_byAIC"].to_numpy()[U] != 0)
