"""The Newton-step solvers of dlsa_amd/csrc/chol.hip, route by route, against an extended-precision solve.

Inside a fit a wrong solver is invisible: the gradient and Sig_inv come from the data passes, so a step that is somewhat wrong
only costs passes.  Here every route runs alone, through dlsa_newton_solve_probe_f64 (the launch functions the drivers call), on
SPD systems of known condition number, and is held to the textbook n eps bounds of Cholesky / symmetric elimination, with
c = max(p, 8) eps and kappa the matrix's own 2-norm condition number:

    eta = |v - S x|_inf / (|S|_inf |x|_inf + |v|_inf) <= c        forward error |x - x_ref|_inf / |x_ref|_inf <= c kappa
    |Hinv S - I|_max, |Linv L - I|_max, |Hinv - Hinv'|_max / |Hinv|_max <= c kappa        |L L' - S|_max <= c |S|_max

every measure evaluated in numpy.longdouble (tests/solve_reference.py).  The caps are conditions, not measurements:
tests/test_solve_reference_cpu.py shows plain fp64 computations of the same quantities using at most a quarter of them.
The second half is the contract of the three `stats` doubles, which the drivers read as stopping rule and partition status.
Each case prints its figures as fractions of the caps ("frac ...", shown with pytest -s)."""
import numpy as np
import pytest

import solve_reference as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BLOCKED_P = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 113, 257, 500)
SWEEP_P = (1, 2, 3, 55, 56, 57, 63, 64, 65, 100, 111, 112)
KAPPAS = (10.0, 1e6, 1e10)
PAD = 3                       # row pitch lds = p + 3, NaN in the padding
SENTINEL = -7.0625            # what output buffers hold before a call


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dlsa_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared reference cases are read-only)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pitched(S, lds=None):
    """S as a flat buffer with row pitch lds and NaN in the padding"""
    p = S.shape[0]
    buf = np.full((p, lds or p + PAD), np.nan)
    buf[:, :p] = S
    return buf.reshape(-1)


def run(eng, route, S, v, ref=None, v2=None, lds=None):
    """one system through one route: (x, M [p, p], stats) as numpy; S must come back bit-unchanged"""
    p = S.shape[0]
    lds = lds or p + PAD
    host = pitched(S, lds)
    Sd = dev(host)
    x = torch.full((p,), SENTINEL, dtype=torch.float64, device="cuda")
    M = torch.full((p * p,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda")
    eng.newton_solve_probe(route, Sd, dev(v), p, lds, ref=None if ref is None else dev(ref),
                           v2=None if v2 is None else dev(v2), x=x, M=M, stats=st)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Sd.cpu().numpy()), bits(host)), "the solver wrote into S"
    return x.cpu().numpy(), M.cpu().numpy().reshape(p, p), st.cpu().numpy()


def run_route(eng, route, S, v, ref=None):
    """the right-hand side of the reported solve is v on every route (route "reuse" factors with another one first)"""
    if route == "reuse":
        other = np.random.default_rng(5).standard_normal(len(v))
        return run(eng, route, S, other, ref=ref, v2=v)
    return run(eng, route, S, v, ref=ref)


def check_stats(x, stats, ref, info=0.0):
    assert stats[0] == np.max(np.abs(x)), "stats[0] is not max|x| of the returned x"
    assert stats[1] == (0.0 if ref is None else np.max(np.abs(ref))), "stats[1] is not max|ref|"
    assert stats[2] == info, "info %r, expected %r" % (stats[2], info)


def some_ref(p, kappa):
    """every other case passes no ref (stats[1] must then be 0)"""
    return None if (p + int(np.log10(kappa))) % 2 else np.random.default_rng(p).standard_normal(p) * 3.0


def report(route, p, kappa, **fracs):
    print("frac route=%s p=%d kappa=%.0e %s" % (route, p, kappa, " ".join("%s=%.4f" % kv for kv in fracs.items())))


def solve_fractions(c, x):
    p, k = c["S"].shape[0], c["kappa"]
    return sr.backward_error(c["S"], x, c["v"]) / sr.cap(p), sr.forward_error(x, c["x"]) / (sr.cap(p) * k)


# ---- accuracy, route by route ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("p", BLOCKED_P)
def test_factor_route(eng, p, kappa):
    """blocked factor + triangular solves: eta, forward error, L L' = S on the lower triangle, exact zeros above the diagonal;
    the reuse route on the same right-hand side returns the same bits, whichever right-hand side the factor was made with"""
    c = sr.case(p, kappa)
    S, v, ref = c["S"], c["v"], some_ref(p, kappa)
    x, L, st = run(eng, "factor", S, v, ref=ref)
    check_stats(x, st, ref)
    eta, fwd = solve_fractions(c, x)
    fac = sr.factor_residual(L, S) / sr.cap(p)
    assert np.all(np.triu(L, 1) == 0.0)
    x1, L1, st1 = run(eng, "reuse", S, v, ref=ref, v2=v)
    assert np.array_equal(bits(x1), bits(x)) and np.array_equal(bits(L1), bits(L)) and np.array_equal(bits(st1), bits(st))
    x2, L2, st2 = run_route(eng, "reuse", S, v, ref=ref)           # the factor was made for another right-hand side
    assert np.array_equal(bits(x2), bits(x)) and np.array_equal(bits(L2), bits(L))
    check_stats(x2, st2, ref)
    report("factor", p, kappa, eta=eta, forward=fwd, factor=fac)
    assert eta <= 1.0 and fwd <= 1.0 and fac <= 1.0


@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("p", BLOCKED_P)
def test_inverse_route(eng, p, kappa):
    """explicit inverse of the factor + x = Linv' (Linv v): the eta cap of the factor route, forward error, Linv L = I against the
    factor of the factor route, (Linv' Linv) S = I, exact zeros above the diagonal of Linv"""
    c = sr.case(p, kappa)
    S, v, ref, k = c["S"], c["v"], some_ref(p, kappa), c["kappa"]
    x, Linv, st = run(eng, "inverse", S, v, ref=ref)
    check_stats(x, st, ref)
    _, L, _ = run(eng, "factor", S, v)
    assert np.all(np.triu(Linv, 1) == 0.0)
    eta, fwd = solve_fractions(c, x)
    lil = sr.identity_residual(Linv, L) / (sr.cap(p) * k)
    Hinv = np.dot(Linv.T.astype(sr.LD), Linv.astype(sr.LD))
    inv = sr.identity_residual(Hinv, S) / (sr.cap(p) * k)
    report("inverse", p, kappa, eta=eta, forward=fwd, LinvL=lil, inverse=inv)
    assert eta <= 1.0 and fwd <= 1.0 and lil <= 1.0 and inv <= 1.0


@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("p", SWEEP_P)
def test_sweep_route(eng, p, kappa):
    """sweep-operator inverse (p <= 112, the 112 template-unrolled sweeps): eta, forward error, Hinv S = I, symmetry of Hinv"""
    c = sr.case(p, kappa)
    S, v, ref, k = c["S"], c["v"], some_ref(p, kappa), c["kappa"]
    x, Hinv, st = run(eng, "sweep", S, v, ref=ref)
    check_stats(x, st, ref)
    assert np.all(np.isfinite(Hinv))
    eta, fwd = solve_fractions(c, x)
    inv = sr.identity_residual(Hinv, S) / (sr.cap(p) * k)
    sym = sr.asymmetry(Hinv) / (sr.cap(p) * k)
    report("sweep", p, kappa, eta=eta, forward=fwd, inverse=inv, symmetry=sym)
    assert eta <= 1.0 and fwd <= 1.0 and inv <= 1.0 and sym <= 1.0


@pytest.mark.parametrize("kappa", KAPPAS)
def test_inverse_route_at_the_lds_limit(eng, kappa):
    """p = 2036: the largest p whose 4 p + 48 doubles fit inv_apply_kernel's 64 KB of LDS.  eta only (no longdouble factor here)."""
    p = 2036
    S = sr.spd_matrix(p, kappa, p)
    v = np.random.default_rng(p).standard_normal(p)
    for route in ("factor", "inverse"):
        x, _, st = run(eng, route, S, v)
        check_stats(x, st, None)
        eta = sr.backward_error(S, x, v) / sr.cap(p)
        report(route, p, kappa, eta=eta)
        assert eta <= 1.0


def test_inverse_apply_refuses_what_does_not_fit_its_lds(eng):
    """p = 2037 needs 64 KB + 32 B: launch_inv_apply says so itself and launches nothing (x keeps what it held)"""
    from dlsa_amd._lib import DlsaError
    p = 2037
    S = np.eye(p)
    Sd, vd = dev(S.reshape(-1)), dev(np.ones(p))
    x = torch.full((p,), SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(DlsaError, match="inverse apply: p=2037 too large") as e:
        eng.newton_solve_probe("inverse", Sd, vd, p, p, x=x)
    assert e.value.code == 1
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    assert np.all(xh == 1.0)                                 # the factor's own solve of S = I ran; nothing came after it
    xs, _, st = run(eng, "factor", S, np.ones(p))
    assert np.all(xs == 1.0) and st[2] == 0.0
    with pytest.raises(DlsaError, match="spd_inverse_small: p=113"):
        eng.newton_solve_probe("sweep", dev(np.eye(113).reshape(-1)), dev(np.ones(113)), 113, 113)


# ---- the stats contract ----------------------------------------------------------------------------------------------
ROUTES = ("factor", "reuse", "inverse", "sweep")
STATUS_P = {"factor": (33, 65, 113, 257), "reuse": (33, 65, 113), "inverse": (33, 65, 113, 257), "sweep": (33, 57, 64, 112)}
ROUTE_P = [(r, p) for r in ROUTES for p in STATUS_P[r]]


def near_identity(p):
    """SPD with entries O(1) whose elimination stays benign when a failed pivot is replaced by 1, as the kernels do: I + 0.01 G
    (pivots ~ 1, multipliers ~ 0.01), so the arithmetic that continues past the failure is finite and the code under test is the
    only thing that decides stats[2]"""
    G = np.random.default_rng(300 + p).uniform(-1.0, 1.0, (p, p))
    return np.eye(p) + 0.005 * (G + G.T)


@pytest.mark.parametrize("route,p", ROUTE_P)
def test_non_positive_pivot_is_code_1(eng, route, p):
    """a finite matrix made indefinite by lowering ONE diagonal entry: first block, block edge, later block, last (partial) block"""
    v = np.random.default_rng(p).standard_normal(p)
    for k in sorted({0, 31, 32, 33, p - 1} & set(range(p))):
        S = near_identity(p)
        S[k, k] -= 2.0
        x, _, st = run_route(eng, route, S, v)
        assert np.all(np.isfinite(x)), (k, "the continued arithmetic left the finite range")
        assert st[2] == 1.0, (k, st[2])
        assert st[0] == np.max(np.abs(x))


def poisoned(p, what, bad):
    S, v = near_identity(p), np.random.default_rng(p).standard_normal(p)
    j0 = ((p - 1) // 32) * 32                              # first row of the last 32-block
    if what == "diagonal":
        S[min(5, p - 1), min(5, p - 1)] = bad
    elif what == "diagonal of the last block":
        S[p - 1, p - 1] = bad
    elif what == "below the diagonal, first block":
        S[3, 1] = S[1, 3] = bad
    elif what == "below the diagonal, last block":          # (a last block of one row has nothing below its diagonal:
        i, j = p - 1, (j0 if j0 < p - 1 else p - 2)         #  the entry then sits in the panel under the block before)
        S[i, j] = S[j, i] = bad
    elif what == "v":
        v[p // 2] = bad
    elif what == "diagonal, then a non-positive pivot in the same block":
        S[2, 2] = bad
        S[7, 7] -= 2.0
    elif what == "diagonal, then a non-positive pivot in the last block":
        S[j0, j0] = bad
        S[p - 1, p - 1] -= 2.0
    return S, v


POISON = ("diagonal", "diagonal of the last block", "below the diagonal, first block", "below the diagonal, last block", "v",
          "diagonal, then a non-positive pivot in the same block", "diagonal, then a non-positive pivot in the last block")


@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
@pytest.mark.parametrize("route,p", ROUTE_P)
def test_non_finite_input_is_code_2(eng, route, p, bad):
    """NaN / Inf on the diagonal, below it in the first and in the last block, in v alone -- and a NaN diagonal entry FOLLOWED by a
    non-positive pivot in the same 32-block: the worst code wins (chol_diag_kernel used to keep the last one: it went on with
    sq = 1 and finite numbers, met the non-positive pivot and reported 1, "not SPD", where the sweep route and the header say NaN)"""
    for what in POISON:
        if what.endswith("last block") and "then" in what and (p - 1) % 32 == 0:
            continue                                       # a last block of one row holds one pivot
        S, v = poisoned(p, what, bad)
        _, _, st = run_route(eng, route, S, v)
        assert st[2] == 2.0, (what, st[2])


def test_c_entries_map_the_codes_as_the_header_says(eng):
    """dlsa_spd_solve_f64: code 1 -> DLSA_ERR_NOT_SPD (4), code 2 -> DLSA_ERR_NAN (6).  dlsa_wls_solve_f64: code 2 -> DLSA_ERR_NAN;
    a failed pivot is no error there but the way into the lstsq branch (full rank for an indefinite, well-conditioned S)."""
    from dlsa_amd._lib import DlsaError
    p = 65
    v = np.random.default_rng(p).standard_normal(p)
    indef = near_identity(p)
    indef[40, 40] -= 2.0
    with pytest.raises(DlsaError) as e:
        eng.spd_solve(dev(indef), dev(v))
    assert e.value.code == 4
    theta, rank = eng.wls_solve(dev(indef), dev(v))
    assert rank == p and sr.forward_error(theta.cpu().numpy(), np.linalg.solve(indef, v)) < 1e-10
    for what in ("diagonal", "below the diagonal, last block", "v", "diagonal, then a non-positive pivot in the same block"):
        S, vv = poisoned(p, what, float("nan"))
        for solve in (eng.spd_solve, eng.wls_solve):
            with pytest.raises(DlsaError) as e:
                solve(dev(S), dev(vv))
            assert e.value.code == 6, (what, solve.__name__, e.value.code)


# ---- the batched sweep -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (57, 100, 112))
def test_batched_sweep(eng, p):
    """five distinct systems, lda > p, strides beyond the dense ones, stats pitch 3 (as the lock step passes it), two members
    switched off, one indefinite: active members equal the single-system launch in bits (stats included), everything else in
    the output buffers -- inactive members, the gaps between members -- keeps what it held"""
    count, lda = 5, p + PAD
    ss, sv, sm, st_ = p * lda + 7, p + 5, p * p + 11, 3
    active = [1, 0, 1, 1, 0]
    mats = [np.array(sr.spd_matrix(p, kap, 900 + 10 * b + p)) for b, kap in enumerate((10.0, 1e3, 10.0, 1e6, 1e10))]
    mats[2] = near_identity(p)
    mats[2][p // 2, p // 2] -= 2.0                          # the indefinite member, between two sound ones
    rng = np.random.default_rng(p)
    vs, refs = rng.standard_normal((count, p)), rng.standard_normal((count, p))
    Sb, vb, rb = np.full(count * ss, np.nan), np.full(count * sv, np.nan), np.full(count * sv, np.nan)
    for b in range(count):
        Sb[b * ss: b * ss + p * lda] = pitched(mats[b], lda)
        vb[b * sv: b * sv + p], rb[b * sv: b * sv + p] = vs[b], refs[b]
    Sd = dev(Sb)
    x = torch.full((count * sv,), SENTINEL, dtype=torch.float64, device="cuda")
    M = torch.full((count * sm,), SENTINEL, dtype=torch.float64, device="cuda")
    st = torch.full((count * st_,), SENTINEL, dtype=torch.float64, device="cuda")
    eng.newton_solve_probe("sweep_batched", Sd, dev(vb), p, lda, count=count, ref=dev(rb), ss=ss, sv=sv, sm=sm, st=st_,
                           active=torch.tensor(active, dtype=torch.int32, device="cuda"), x=x, M=M, stats=st)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Sd.cpu().numpy()), bits(Sb))
    want_x, want_M, want_st = np.full(count * sv, SENTINEL), np.full(count * sm, SENTINEL), np.full(count * st_, SENTINEL)
    for b in range(count):
        if active[b]:
            xs, Hs, sts = run(eng, "sweep", mats[b], vs[b], ref=refs[b], lds=lda)
            want_x[b * sv: b * sv + p], want_M[b * sm: b * sm + p * p], want_st[b * 3: b * 3 + 3] = xs, Hs.reshape(-1), sts
    got_st = st.cpu().numpy()
    assert np.array_equal(bits(got_st), bits(want_st)), (got_st, want_st)
    assert np.array_equal(bits(x.cpu().numpy()), bits(want_x))
    assert np.array_equal(bits(M.cpu().numpy()), bits(want_M))
    assert [got_st[3 * b + 2] for b in (0, 2, 3)] == [0.0, 1.0, 0.0]
    for b in (0, 3):
        assert got_st[3 * b] == np.max(np.abs(want_x[b * sv: b * sv + p])) and got_st[3 * b + 1] == np.max(np.abs(refs[b]))
        assert sr.backward_error(mats[b], want_x[b * sv: b * sv + p], vs[b]) <= sr.cap(p)
