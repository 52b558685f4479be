"""The spectral route of the WLS combine (dlsa_amd/csrc/eigsolve.hip: parallel two-sided Jacobi, then lstsq's truncated
pseudo-inverse) against an extended-precision eigendecomposition, through dlsa_sym_pinv_probe_f64 -- the solve entry's own call
with the sweep count and the eigenvectors handed out as well.

tests/test_gpu_wls.py compares with fp64 LAPACK at 1e-9 on Gaussian Wishart matrices.  Here the spectra are the ones the
combine of one-hot blocks produces -- repeated eigenvalues, clusters, exact null spaces, indefinite and graded ones -- at the
sizes where the launch geometry changes (p = 1: no rotation; 2: one pair; odd p: the zero-padded index takes part in the
schedule; 8, 33: a (32, 8) block partly full, half = 17 crosses its y extent; 64, 65: half = 32, 33 cross its x extent; 130:
several blocks each way; 257, 500: closed forms only), and every result is held to the p eps class of Jacobi, C = 8 max(p, 8) eps:

    |sorted lambda - sorted lambda_ref| <= C lmax      |S V - V diag(lambda)|_max <= C lmax      |V'V - I|_max <= C
    rank = the reference's      |theta - theta_ref|_inf <= C (lmax / min kept |lambda|) |theta_ref|_inf
    |N' theta|_2 <= C |theta|_2 for the reference's null basis N (the minimum-norm property)      sweeps <= 40

every measure evaluated in numpy.longdouble (tests/pinv_reference.py).  The caps are conditions, not measurements:
tests/test_pinv_reference_cpu.py shows a plain fp64 Jacobi using at most half of each, and every case at least a factor 4 away
from the singular-value cut on both sides, so no rank here depends on rounding.  Each case prints its figures as fractions of
the caps ("frac ...", shown with pytest -s); the module prints the worst per spectrum class and the sweep counts at its end."""
import collections

import numpy as np
import pytest

import pinv_reference as pr
import solve_reference as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAD = 3                       # row pitch lds = p + 3, NaN in the padding
ids = lambda c: "%s-%d" % c if isinstance(c, tuple) else str(c)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dlsa_amd import engine
    return engine


@pytest.fixture(scope="module")
def table():
    """worst fraction of each cap per spectrum class, sweeps per (class, p); printed when the module is done"""
    t = {"worst": collections.defaultdict(dict), "sweeps": collections.defaultdict(dict)}
    yield t
    for kind, w in t["worst"].items():
        print("worst kind=%s %s | sweeps %s" % (kind, " ".join("%s=%.4f" % kv for kv in sorted(w.items())),
                                              " ".join("%d:%d" % kv for kv in sorted(t["sweeps"][kind].items()))))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared reference cases are read-only)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pitched(S, lds):
    """S as a flat buffer with row pitch lds and NaN in the padding"""
    p = S.shape[0]
    buf = np.full((p, lds), np.nan)
    buf[:, :p] = S
    return buf.reshape(-1)


def probe(eng, S, v, rcond=None, lds=None, ldv=None):
    """(theta, rank, eigenvalues, sweeps, V [p, p]) as numpy; S must come back bit-unchanged"""
    p = S.shape[0]
    lds = lds or p
    host = pitched(S, lds)
    Sd = dev(host)
    theta, rank, eig, sweeps, V = eng.sym_pinv_probe(Sd, dev(v), p, lds, rcond=rcond, ldv=ldv)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Sd.cpu().numpy()), bits(host)), "the solver wrote into S"
    Vh = V.cpu().numpy()
    assert np.all(np.isnan(Vh[:, p:])), "the eigenvector copy wrote past its p columns"
    return theta.cpu().numpy(), rank, np.array(eig, dtype=np.float64), sweeps, np.ascontiguousarray(Vh[:, :p])


def same(a, b):
    return a[1] == b[1] and all(np.array_equal(bits(x), bits(y)) for x, y in zip((a[0], a[2]) + tuple(a[4:]), (b[0], b[2]) + tuple(b[4:])))


def wls(eng, S, v):
    theta, rank = eng.wls_solve(dev(S), dev(v))
    return theta.cpu().numpy(), rank


# ---- accuracy, case by case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.CASES, ids=ids)
def test_decomposition_and_solve(eng, table, case):
    c = pr.case(*case)
    kind, p, S, v = c["kind"], c["p"], c["S"], c["v"]
    theta, rank, eig, sweeps, V = probe(eng, S, v)
    assert eig.shape == (p,) and np.all(np.isfinite(eig)) and np.all(np.isfinite(V)) and np.all(np.isfinite(theta))
    f = pr.fractions(c, eig, V, theta)
    print("frac kind=%s p=%d sweeps=%d rank=%d %s" % (kind, p, sweeps, rank, " ".join("%s=%.4f" % kv for kv in f.items())))
    for k, x in f.items():
        table["worst"][kind][k] = max(table["worst"][kind].get(k, 0.0), x)
    table["sweeps"][kind][p] = sweeps
    # the solve entry is the same call: the same bits
    t2, r2, e2 = eng.sym_pinv_solve(dev(S), dev(v))
    assert r2 == rank and np.array_equal(bits(t2.cpu().numpy()), bits(theta)) and np.array_equal(bits(e2), bits(eig))
    assert rank == c["rank"], (rank, c["rank"])
    assert 0 <= sweeps <= 40 and (sweeps > 0 or p == 1)
    worst = max(f, key=f.get)
    assert f[worst] <= 1.0, (worst, f[worst])
    if c["singular"] or c["indefinite"]:
        # a failed or roundoff-sized pivot sends wls_solve down this route with lstsq's rcond: the same theta and rank
        t3, r3 = wls(eng, S, v)
        assert r3 == rank and np.array_equal(bits(t3), bits(theta))


# ---- single-purpose tests --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (4, 33))
def test_explicit_rcond(eng, p):
    """spectrum {1, 1e-3, 1e-6, 1e-9} repeated to fill p: rcond between the groups keeps the prefixes, rcond = 0 keeps every
    non-zero eigenvalue -- and not the exact zero of the padded index at odd p"""
    S, v = pr.rcond_case(p)
    lam, V = pr.eigh_ld(S)
    ranks = []
    for rcond in pr.RCONDS + (0.0,):
        ref = pr.pinv_from_eig(lam, V, v, rcond)
        theta, rank, eig, _, _ = probe(eng, S, v, rcond=rcond)
        ranks.append(rank)
        assert rank == ref["rank"], (rcond, rank, ref["rank"])
        assert eig.shape == (p,) and np.all(eig != 0.0)
        assert pr.theta_error(theta, ref["theta"]) <= pr.C(p) * float(ref["lmax"] / ref["min_kept"]), rcond
    assert ranks == [(p + 3) // 4, (p + 2) // 4 + (p + 3) // 4, p - p // 4, p]


@pytest.mark.parametrize("case", [("clusters", 33), ("trap", 8), ("halfzero", 65), ("toeplitz", 130)], ids=ids)
def test_row_pitch(eng, case):
    """lds = p + 3 with NaN in the padding columns, V at a pitch of its own: bit-equal to the contiguous call, through the probe, the
    solve entry and wls_solve"""
    c = pr.case(*case)
    p, S, v = c["p"], c["S"], c["v"]
    a = probe(eng, S, v)
    b = probe(eng, S, v, lds=p + PAD, ldv=p + 5)
    assert same(a, b) and a[3] == b[3]
    wide = dev(pitched(S, p + PAD)).view(p, p + PAD)
    t2, r2, e2 = eng.sym_pinv_solve(wide[:, :p], dev(v))
    assert r2 == a[1] and np.array_equal(bits(t2.cpu().numpy()), bits(a[0])) and np.array_equal(bits(e2), bits(a[2]))
    t3, r3 = eng.wls_solve(wide[:, :p], dev(v))
    t4, r4 = wls(eng, S, v)
    assert r3 == r4 and np.array_equal(bits(t3.cpu().numpy()), bits(t4))


@pytest.mark.parametrize("p", (8, 33))
def test_only_the_symmetric_part_is_read(eng, p):
    """an integer S plus an integer skew matrix K: (S + K + (S + K)') / 2 = S exactly, so the results are those of S in bits"""
    rng = np.random.default_rng(p)
    G = rng.integers(-9, 10, (p, p)).astype(np.float64)
    S = np.triu(G) + np.triu(G, 1).T
    S[:, p - 1] = S[:, 0]
    S[p - 1, :] = S[0, :]                                         # (two equal columns: singular, and indefinite)
    S[p - 1, p - 1] = S[0, 0]
    K = np.triu(rng.integers(-9, 10, (p, p)).astype(np.float64), 1)
    K = K - K.T
    v = rng.standard_normal(p)
    a, b = probe(eng, S, v), probe(eng, S + K, v)
    assert same(a, b) and a[3] == b[3] and a[1] < p
    ref = pr.pinv_solve(S, v)
    assert ref["margin"] >= 4.0 and a[1] == ref["rank"]
    assert pr.theta_error(a[0], ref["theta"]) <= pr.C(p) * float(ref["lmax"] / ref["min_kept"])


@pytest.mark.parametrize("p", (3, 7, 65))
def test_identity_at_odd_p_never_shows_the_padded_zero(eng, p):
    v = np.random.default_rng(p).standard_normal(p)
    theta, rank, eig, sweeps, V = probe(eng, np.eye(p), v)
    assert rank == p and np.all(eig == 1.0) and np.array_equal(V, np.eye(p)) and np.array_equal(bits(theta), bits(v))
    theta, rank, eig, _, _ = probe(eng, np.eye(p), v, rcond=0.0)
    assert rank == p and np.all(eig == 1.0)


def scaled_runs(eng, S, v, k):
    s = 2.0 ** k
    a, b = probe(eng, S, v), probe(eng, S * s, v * s)
    assert np.all(np.isfinite(S * s)) and np.all((S * s) / s == S) and np.all((v * s) / s == v)      # the scaling is exact
    return a, b, s


@pytest.mark.parametrize("k", (100, -100))
@pytest.mark.parametrize("case", [("clusters", 33), ("plusminus", 8), ("trap", 7), ("graded", 64)], ids=ids)
def test_power_of_two_covariance(eng, case, k):
    """(2^k S, 2^k v): theta in the same bits, the eigenvalues in the same bits after the exact rescale, V and the sweep count
    the same"""
    c = pr.case(*case)
    a, b, s = scaled_runs(eng, c["S"], c["v"], k)
    assert b[1] == a[1] and b[3] == a[3]
    assert np.array_equal(bits(b[0]), bits(a[0])) and np.array_equal(bits(b[2] / s), bits(a[2])) and np.array_equal(bits(b[4]), bits(a[4]))


@pytest.mark.parametrize("k", (600, -600))
@pytest.mark.parametrize("case", [("trap", 7), ("trap_repeated", 33), ("halfzero", 8)], ids=ids)
def test_power_of_two_covariance_beyond_the_range_of_squares(eng, case, k):
    """entries near 1e+-180: their squares leave the fp64 range.  Before the iteration worked on 2^-e S (max|a| in [1, 2)) the sums
    of squares of its stopping rule underflowed to 0 <= 1e-30 * 0 -- "settled" after one sweep, eigenvalues wrong by 1e-6 .. 1e-3
    with DLSA_OK -- or overflowed into DLSA_ERR_NAN.  lstsq is scale-invariant; singular cases, so that wls_solve comes here too"""
    c = pr.case(*case)
    a, b, s = scaled_runs(eng, c["S"], c["v"], k)
    assert b[1] == a[1] == c["rank"] and b[3] == a[3]
    assert np.array_equal(bits(b[0]), bits(a[0])) and np.array_equal(bits(b[2] / s), bits(a[2])) and np.array_equal(bits(b[4]), bits(a[4]))
    f = pr.fractions(c, b[2] / s, b[4], b[0])
    assert max(f.values()) <= 1.0, f
    t3, r3 = wls(eng, c["S"] * s, c["v"] * s)
    assert r3 == c["rank"] and np.array_equal(bits(t3), bits(a[0]))


@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_non_finite_input_is_an_error_not_a_theta(eng, bad):
    from dlsa_amd._lib import DlsaError
    c = pr.case("linear", 33)
    for i, j in ((5, 9), (0, 0), (32, 32), (32, 1)):
        S = np.array(c["S"])
        S[i, j] = bad                                             # ONE entry (its mirror image stays finite)
        with pytest.raises(DlsaError) as e:
            eng.sym_pinv_solve(dev(S), dev(c["v"]))
        assert e.value.code == 6, ((i, j), e.value.code)
    # wls_solve, indefinite: the first pivot fails (code 1) long before the factorisation reaches the far corner
    S = np.array(c["S"])
    S[0, 0] = -1.0
    S[32, 32] = bad
    with pytest.raises(DlsaError) as e:
        eng.wls_solve(dev(S), dev(c["v"]))
    assert e.value.code == 6
    v = np.array(c["v"])
    v[7] = bad
    S[32, 32] = 1.0
    with pytest.raises(DlsaError) as e:                           # indefinite S, the bad entry in v alone
        eng.wls_solve(dev(S), dev(v))
    assert e.value.code == 6


@pytest.mark.parametrize("p", (8, 64))
def test_routes_of_wls_solve(eng, p):
    """condition number 100 times below 1 / (eps p): the Cholesky route, rank p, the longdouble Cholesky solution within c kappa.
    100 times above: the spectral route, the reference's truncated solution and rank.  (In between both answers are defensible.)"""
    S, v = pr.route_case(p, "below")
    theta, rank = wls(eng, S, v)
    kappa = sr.cond2(S)
    assert rank == p and sr.forward_error(theta, sr.solve(S, v)) <= sr.cap(p) * kappa
    assert np.array_equal(bits(theta), bits(eng.spd_solve(dev(S), dev(v)).cpu().numpy()))
    S, v = pr.route_case(p, "above")
    ref = pr.pinv_solve(S, v)
    theta, rank = wls(eng, S, v)
    assert rank == ref["rank"] == p - p // 4
    assert pr.theta_error(theta, ref["theta"]) <= pr.C(p) * float(ref["lmax"] / ref["min_kept"])


def test_mapred_on_blocks_that_sum_to_the_dummy_trap(eng):
    """K = 3 partitions of an intercept + full one-hot design (integer level counts, integer Sig_invMcoef, so the device's sums are
    exact): dlsa_mapred warns rank L < L + 1 and beta_byOLS is the reference's minimum-norm solution"""
    import dlsa_amd
    L, K = 6, 3
    p = L + 1
    counts = np.array([[2, 0, 1, 3, 1, 0], [1, 2, 0, 1, 0, 4], [0, 1, 2, 0, 3, 1]], dtype=np.float64)
    sig = np.stack([pr.dummy_trap(counts[k]) for k in range(K)])
    coef = np.random.default_rng(5).integers(-3, 4, (K, p)).astype(np.float64)
    smc = np.einsum("kij,kj->ki", sig, coef)
    S, v = sig.sum(0), smc.sum(0)
    assert np.array_equal(S, pr.dummy_trap(counts.sum(0)))
    ref = pr.pinv_solve(S, v)
    assert ref["rank"] == L and ref["margin"] >= 4.0
    names = ["x%d" % i for i in range(p)]
    mb = dlsa_amd.MappedBlocks(dev(coef), dev(smc), dev(sig), names)
    with pytest.warns(UserWarning, match="rank %d < %d" % (L, p)):
        out = dlsa_amd.dlsa_mapred(mb)
    assert np.array_equal(out.iloc[:, 2:].to_numpy(), S)
    beta = out["beta_byOLS"].to_numpy()
    assert pr.theta_error(beta, ref["theta"]) <= pr.C(p) * float(ref["lmax"] / ref["min_kept"])
    assert pr.null_component(pr.trap_null(p)[:, None], beta) <= pr.C(p)
