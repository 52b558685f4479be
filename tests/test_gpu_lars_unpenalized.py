"""GPU: the LARS path with u >= 2 leading unpenalised coefficients (dlsa_lars_lsa_f64 with `intercept` = u; lsa.lars_path_device
and dlsa() with `unpenalized`) against tests/lars_unpenalized_reference.py -- the oracle's path of the host-reduced problem -- and
against the library's own one-intercept path on the same problem.

Bars: the project's LARS bars (tests/test_gpu_kernels.py): 1e-8 relative l-infinity on beta, beta0, theta, AIC and BIC; 1e-7 on the
correlated designs at rho >= 0.97.  The path certificate (tests/lars_certificate.py, its own TOL / TOL_DERIVED) runs on every case,
on the float64 host reduction.  Every run reads the grid-abort count before and after: a path that came from the single-workgroup
rerun did not test the kernel the case names."""
import ctypes
import functools

import numpy as np
import pytest

import guarded_workspace as gw
import lars_certificate as lc
import lars_problems
import lars_unpenalized_reference as ur
import stream_gate as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("beta", "beta0", "theta", "AIC", "BIC")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


@pytest.fixture(scope="module")
def lsa():
    from dlsa_amd import lsa
    return lsa


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the cached problems are read-only)


def aborts():
    from dlsa_amd import _lib
    return _lib.load().dlsa_lars_grid_barrier_timeout(0.0)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# beyond the reference's problems: (p, rho, seed, u, type) on lars_problems' "corr" design, U drawn with the seed
EXTRA = {
    "m=1,u=2": (3, 0.3, 1, 2, "lar"), "m=2,u=2": (4, 0.3, 2, 2, "lasso"), "m=3,u=2": (5, 0.3, 3, 2, "lasso"),
    "u=32,p=96": (96, 0.5, 4, 32, "lasso"),
    "odd m=55": (60, 0.5, 5, 5, "lasso"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(S, b, n, U, type, reference path, bar)"""
    if name in EXTRA:
        p, rho, seed, u, typ = EXTRA[name]
        S, b, n = lars_problems.problem(("corr", p, rho, seed))
        U = sorted(int(i) for i in np.random.default_rng(seed).choice(p, u, replace=False))
        return S, b, n, U, typ, ur.path(S, b, U, n, typ), 1e-8
    S, b, n, U, typ = ur.problem(name)
    return S, b, n, U, typ, ur.problem_path(name), 1e-7 if name[0] == "corr" and name[2] >= 0.97 else 1e-8


def run(lsa, S, b, n, U, typ, **kw):
    before = aborts()
    r = lsa.lars_path_device(dev(S), dev(b), False, float(n), type=typ, unpenalized=U, **kw)
    out = {k: r[k].cpu().numpy() for k in KEYS}
    assert aborts() == before, "a grid launch aborted: the path came from the single-workgroup rerun"
    return out


def check(name, r, label=""):
    S, b, n, U, typ, ref, bar = case(name)
    assert r["beta"].shape == ref["beta"].shape, (r["beta"].shape, ref["beta"].shape)
    assert r["beta0"].shape == ref["beta0"].shape and r["theta"].shape == ref["theta"].shape
    errs = {k: ur.rel(r[k], ref[k]) for k in KEYS}
    Sig, bR, _, _ = ur.reduce(S, b, U)
    res = lc.certify(Sig, bR, False, n, typ, {k: r[k] for k in ("beta", "AIC", "BIC")})
    print("lars unpenalized %s%s: m %d u %d steps %d  vs reference %s  certificate %.1e"
          % (name, label, len(b) - len(U), len(U), r["beta"].shape[0] - 1, {k: "%.1e" % v for k, v in errs.items()}, max(res.values())))
    assert all(v <= bar for v in errs.values()), (errs, bar)


ALL = list(ur.PROBLEMS) + sorted(EXTRA)


@pytest.mark.parametrize("name", ALL, ids=str)
def test_parity_with_the_reference(lsa, name):
    """the four multinomial shapes, m = 1, 2, 3, u = 32, an odd m, and the three correlated lasso problems with drops: 120 (one
    lars_q workgroup), 257 (lars_q's shared pass), 449 (lars_c at its first width)"""
    S, b, n, U, typ, ref, _ = case(name)
    if name in ur.PROBLEMS and name[0] == "corr":
        assert ref["beta"].shape[0] - 1 > ref["beta"].shape[1]           # the reduced path has drops
    check(name, run(lsa, S, b, n, U, typ))


M257, M120 = ("corr", 264, 0.97, 3), ("corr", 127, 0.98, 12)


@pytest.mark.parametrize("name,opts", [
    (M257, dict(lars_q=0)),                     # lars.hip, the grid kernel
    (M257, dict(lars_q=0, lars_wgs=1)),         # lars.hip, the single workgroup
    (M257, dict(lars_q=2)),                     # lars_c.hip forced narrow
    (M120, dict(lars_q_lds=False)),                 # lars_q.hip with Q and RT in global memory
    (("multinomial", 7, 41), dict(lars_q_lds=False, lars_q_wgs=1)),
], ids=str)
def test_parity_on_every_kernel(lsa, kopt, name, opts):
    S, b, n, U, typ, _, _ = case(name)
    kopt.set(**opts)
    check(name, run(lsa, S, b, n, U, typ), " %s" % opts)


def test_just_past_the_column_split(lsa):
    """m = 2045, u = 2: lars.hip's grid kernel by the dispatch (m, not p = 2047, decides); the certificate only"""
    p = 2047
    S, b, n = lars_problems.problem(("corr", p, 0.5, 7))
    U = [5, 1200]
    r = run(lsa, S, b, n, U, "lar")
    Sig, bR, W, R = ur.reduce(S, b, U)
    res = lc.certify(Sig, bR, False, n, "lar", {k: r[k] for k in ("beta", "AIC", "BIC")})
    beta0 = (bR[None, :] - r["beta"]) @ W.T
    theta = np.zeros((r["beta"].shape[0], p))
    theta[:, R] = r["beta"]
    theta[:, U] = b[U][None, :] + beta0
    e0, et = ur.rel(r["beta0"], beta0), ur.rel(r["theta"], theta)
    print("lars unpenalized m = 2045: steps %d certificate %.1e beta0 %.1e theta %.1e" % (r["beta"].shape[0] - 1, max(res.values()), e0, et))
    assert r["beta"].shape[1] == 2045 and e0 <= lc.TOL_DERIVED and et <= lc.TOL_DERIVED


# ---- new code against old code on the same problem ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [("multinomial", J, pe) for J, pe in ur.MULTINOMIAL_SHAPES] + ["u=32,p=96", "odd m=55", M257], ids=str)
def test_nested_identity_on_the_device(eng, lsa, name):
    """U[1:] eliminated on the host, U[0] by the library's one-intercept path (the scalar Schur complement, as before), against all
    of U eliminated on the device.  Bar 1e-8; 1e-7 on the rho = 0.97 design, whose paths carry that bar everywhere in this project."""
    S, b, n, U, typ, _, bar = case(name)
    p = len(b)
    keep = [U[0]] + ur.rest(p, U)
    order = sorted(keep)
    Sig, bR, _, R = ur.reduce(S, b, U[1:])
    assert R == order
    at = [order.index(j) for j in keep]
    old = eng.lars_path(dev(Sig[np.ix_(at, at)]), dev(bR[at]), True, float(n), type=typ)
    new = run(lsa, S, b, n, U, typ)
    errs = {k: ur.rel(new[k], old[k].cpu().numpy()) for k in ("beta", "AIC", "BIC")}
    errs["beta0"] = ur.rel(new["beta0"][:, 0], old["beta0"].cpu().numpy())
    print("nested identity %s:" % (name,), errs)
    assert all(v <= bar for v in errs.values()), errs


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
def test_one_and_none_are_the_old_paths_to_the_bit(lsa):
    S, b, n, _, typ, _, _ = case(M120)
    Sd, bd = dev(S), dev(b)
    a = lsa.lars_path_device(Sd, bd, True, float(n), type=typ)
    c = lsa.lars_path_device(Sd, bd, False, float(n), type=typ, unpenalized=[0])
    assert all(torch.equal(a[k], c[k]) for k in ("beta", "AIC", "BIC")) and torch.equal(a["beta0"], c["beta0"][:, 0])
    assert torch.equal(c["theta"][:, 1:], c["beta"]) and torch.equal(c["theta"][:, 0], c["beta0"][:, 0] + bd[0])
    a = lsa.lars_path_device(Sd, bd, False, float(n), type=typ)
    c = lsa.lars_path_device(Sd, bd, False, float(n), type=typ, unpenalized=[])
    assert all(torch.equal(a[k], c[k]) for k in ("beta", "AIC", "BIC")) and c["beta0"].shape == (a["beta"].shape[0], 0)
    assert torch.equal(c["theta"], c["beta"])


def test_any_positions_are_the_leading_form_of_the_permuted_problem(eng, lsa):
    S, b, n, _, typ, _, _ = case(("multinomial", 7, 6))
    U = [3, 17]
    perm = U + ur.rest(len(b), U)
    lead = eng.lars_path(dev(S[np.ix_(perm, perm)]), dev(b[perm]), 2, float(n), type=typ)
    r = lsa.lars_path_device(dev(S), dev(b), False, float(n), type=typ, unpenalized=U)
    assert lead["beta0"].shape == (lead["beta"].shape[0], 2)
    assert all(torch.equal(lead[k], r[k]) for k in ("beta", "beta0", "AIC", "BIC"))
    assert torch.equal(r["theta"][:, perm[2:]], r["beta"])


@pytest.mark.parametrize("name", [("multinomial", 7, 6), ("corr", 456, 0.97, 5)], ids=str)
def test_two_runs_give_the_same_bits(lsa, name):
    S, b, n, U, typ, _, _ = case(name)
    a, c = run(lsa, S, b, n, U, typ), run(lsa, S, b, n, U, typ)
    assert all(np.array_equal(a[k], c[k]) for k in KEYS)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.0


def raw_call(eng, S, b, u, n=100.0, typ=0, max_steps=0, short=0):
    """dlsa_lars_lsa_f64 itself on sentinel-filled outputs inside guards: (rc, message, outputs untouched, guards intact)"""
    from dlsa_amd import _lib
    lib = _lib.load()
    p = S.shape[0]
    m = max(1, p - max(0, min(u, p - 1)))
    ms = max_steps if max_steps > 0 else 8 * m
    sizes = {"beta": (ms + 1) * m, "beta0": (ms + 1) * max(1, min(max(u, 0), 32)), "aic": ms + 1, "bic": ms + 1}
    pad = 4096
    bufs = {k: torch.full((pad + v + pad,), SENTINEL, dtype=torch.float64, device="cuda") for k, v in sizes.items()}
    nb = lib.dlsa_lars_workspace_bytes(p)
    ws = torch.full((gw.GUARD_BYTES + nb + gw.GUARD_BYTES,), gw.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    steps = ctypes.c_int(-7)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = lib.dlsa_lars_lsa_f64(P(S), S.stride(0), P(b), p, u, float(n), typ, 2.220446049250313e-16, max_steps,
                               P(bufs["beta"], 8 * pad), P(bufs["beta0"], 8 * pad), P(bufs["aic"], 8 * pad), P(bufs["bic"], 8 * pad),
                               ctypes.byref(steps), P(ws, gw.GUARD_BYTES), nb - short, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    untouched = all(bool((t == SENTINEL).all()) for t in bufs.values())
    pads = all(bool((t[:pad] == SENTINEL).all()) and bool((t[-pad:] == SENTINEL).all()) for t in bufs.values())
    guards = bool((ws[:gw.GUARD_BYTES] == gw.GUARD_BYTE).all()) and bool((ws[gw.GUARD_BYTES + nb:] == gw.GUARD_BYTE).all())
    return rc, _lib.last_error() if rc else "", untouched, pads and guards, steps.value


def _singular_cases():
    rng = np.random.default_rng(11)
    n, p = 400, 20
    X = rng.standard_normal((n, p))
    w = rng.random(n) * 0.25 + 0.01
    b = rng.standard_normal(p)
    dup = X.copy()
    dup[:, 3] = dup[:, 1]                       # a repeated column among the first five
    zero = X.copy()
    zero[:, 2] = 0.0                            # an absent level
    S = X.T @ (w[:, None] * X)
    nan = S.copy()
    nan[1, 3] = nan[3, 1] = np.nan
    return {"repeated column": (dup.T @ (w[:, None] * dup), b, 3), "zero column": (zero.T @ (w[:, None] * zero), b, 2), "NaN": (nan, b, None)}


@pytest.mark.parametrize("what", ["repeated column", "zero column", "NaN"])
def test_a_block_that_is_not_positive_definite_is_refused(eng, what):
    S, b, pivot = _singular_cases()[what]
    before = aborts()
    rc, msg, untouched, intact, _ = raw_call(eng, dev(S), dev(b), 5)
    print(what, rc, msg)
    assert rc == 4 and "not positive definite" in msg and untouched and intact and aborts() == before
    if pivot is not None:
        assert "pivot %d " % pivot in msg
    from dlsa_amd import _lib
    with pytest.raises(_lib.DlsaError) as e:
        eng.lars_path(dev(S), dev(b), 5, 100.0)
    assert e.value.code == 4
    if what == "zero column":                   # the same matrix with the first coefficient alone unpenalised: a path
        ok = raw_call(eng, dev(S), dev(b), 1)
        assert ok[0] == 0 and ok[3] and ok[4] > 0


@pytest.mark.parametrize("u", [20, 33, -1, 21])
def test_counts_out_of_range_are_invalid(eng, u):
    S, b, _ = _singular_cases()["NaN"]
    rc, msg, untouched, intact, _ = raw_call(eng, dev(np.nan_to_num(S)), dev(b), u)
    assert rc == 1 and msg and untouched and intact


# ---- the memory contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [("multinomial", 7, 6), ("corr", 456, 0.97, 5)], ids=str)
def test_exact_guarded_poisoned_workspace(eng, lsa, monkeypatch, name):
    """u = 7 at m = 35 and at m = 449 on exactly dlsa_lars_workspace_bytes(p) bytes between guards, poisoned with 0xFF and with 0x00:
    the bits of the plain run, the guards intact; one byte fewer is refused"""
    S, b, n, U, typ, _, _ = case(name)
    plain = run(lsa, S, b, n, U, typ)
    for fill in (gw.POISON, 0x00):
        with pytest.MonkeyPatch.context() as mp:
            g = gw.guarded(mp, fill)
            r = run(lsa, S, b, n, U, typ)
            g.check()
            assert [c for c, _ in g.queries] == ["lars_path"] and g.queries[0][1] == eng._lib.load().dlsa_lars_workspace_bytes(len(b))
        assert all(np.array_equal(r[k], plain[k]) for k in KEYS), "fill 0x%02X changes the result" % fill
    perm = U + ur.rest(len(b), U)
    rc, msg, untouched, intact, _ = raw_call(eng, dev(S[np.ix_(perm, perm)]), dev(b[perm]), len(U), n=n, short=1)
    assert rc == 3 and untouched and intact, (rc, msg)


# ---- the stream contract ------------------------------------------------------------------------------------------------------------
def test_late_inputs_on_a_side_stream(eng, lsa):
    """u = 7 on a side stream whose inputs arrive behind a gate on that stream, the wrapper's allocations poisoned: the bits of the
    default-stream run (prepare, path and finish kernels, the gather and the scatter all wait for the stream they were given)"""
    S, b, n, U, typ, _, _ = case(("multinomial", 7, 41))
    side = sg.side_stream()
    call = lambda S_, b_: lsa.lars_path_device(S_, b_, False, float(n), type=typ, unpenalized=U)
    ready = dict(S_=dev(S), b_=dev(b))
    ref = call(**ready)
    late = {k: torch.full_like(t, float("nan")) for k, t in ready.items()}
    torch.cuda.synchronize()
    try:
        with pytest.MonkeyPatch.context() as mp, torch.cuda.stream(side):
            mp.setattr(eng, "torch", sg.PoisonTorch())
            done = sg.gate(side, 0.3)
            for k, t in late.items():
                t.copy_(ready[k])
            assert not done.query(), "the gate on the side stream had ended before the call: the inputs were not late"
            out = call(**late)
            side.synchronize()
    finally:
        torch.cuda.synchronize()
    assert all(torch.equal(out[k], ref[k]) for k in KEYS)
    check(("multinomial", 7, 41), {k: out[k].cpu().numpy() for k in KEYS}, " late")


# ---- end to end: rows -> blocks -> combine -> BIC-selected coefficients -------------------------------------------------------------
def _selected(S, ols, n, U):
    r = ur.path(S, ols, U, n, "lar")
    return r["theta"][int(np.argmin(r["AIC"]))], r["theta"][int(np.argmin(r["BIC"]))]


def _end_to_end(api, out, n, J, pe):
    names = list(out.columns[2:])
    U = api.intercept_columns(names)
    assert U == [j * pe for j in range(J)]
    res = api.dlsa(out.iloc[:, 2:], out["beta_byOLS"], n, unpenalized="intercepts")
    assert list(res.columns) == ["beta_byAIC", "beta_byBIC"] and res.shape == (J * pe, 2)
    by_aic, by_bic = _selected(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n, U)
    ea, eb = ur.rel(res["beta_byAIC"].to_numpy(), by_aic), ur.rel(res["beta_byBIC"].to_numpy(), by_bic)
    bic = res["beta_byBIC"].to_numpy()
    pen = np.delete(bic, U)
    print("end to end J = %d pe = %d: AIC point %.1e BIC point %.1e; %d of %d penalised coefficients are zero at the BIC point"
          % (J, pe, ea, eb, int((pen == 0).sum()), pen.size))
    assert ea <= 1e-8 and eb <= 1e-8
    assert np.all(bic[U] != 0) and np.all(res["beta_byAIC"].to_numpy()[U] != 0) and np.any(pen == 0)
    # the same selection through indices and through names
    res2 = api.dlsa(out.iloc[:, 2:], out["beta_byOLS"], n, unpenalized=[names[i] for i in U])
    assert np.array_equal(res2.to_numpy(), res.to_numpy())


@pytest.mark.parametrize("C,p", [(3, 6), (8, 4)])
def test_end_to_end_multinomial_with_intercepts(C, p):
    import dlsa_amd
    import multinomial_reference as mr
    n, K = 24_000, 8
    X, y = mr.data(90, n, p, C, True)
    mb = dlsa_amd.fit_multinomial_partitions(dev(X), dev(y), C, partition_num=K, fit_intercept=True)
    assert mb.status == [0] * K
    _end_to_end(dlsa_amd, dlsa_amd.dlsa_mapred(mb), n, C - 1, p + 1)


def test_end_to_end_structured_multinomial():
    """fit_multinomial_design with the intercept a plan column: its names carry intercept:<j>"""
    import dlsa_amd
    import test_gpu_onehot_multinomial as tom
    from oracle import dlsa_oracle as orc
    n, q, nlevels, K, C = 40_000, 2, (6, 4), 4, 3
    p, num, codes, desc, nl, level_col, X, y = tom._fit_case(orc, n, q, nlevels, 90, C)
    spec = tom._spec(dlsa_amd, q, nlevels, desc)
    mb = dlsa_amd.fit_multinomial_design(dev(num), dev(codes), dev(y), spec, C, partition_num=K)
    assert mb.status == [0] * K and mb.names[0] == "intercept:1" and mb.names[p] == "intercept:2"
    _end_to_end(dlsa_amd, dlsa_amd.dlsa_mapred(mb), n, C - 1, p)
