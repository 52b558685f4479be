"""The extended-precision reference of the spectral solve (tests/pinv_reference.py) against numpy.linalg, mpmath and closed
forms, and the two conditions that make the caps of tests/test_gpu_pinv_solve.py honest:

  * every case sits at least FOUR TIMES away from lstsq's singular-value cut on both sides, in the reference's own spectrum, so
    the rank the GPU test asserts is not a matter of rounding;
  * a plain fp64 cyclic Jacobi with the kernel's stopping rule (off-diagonal mass <= 1e-15 of the Frobenius norm), put through
    the same measures, uses at most HALF of every cap C = 8 max(p, 8) eps on every case.  The worst seen: orthogonality 0.43 of
    its cap (dummy trap, p = 130, 15 sweeps), eigenvalues 0.035, residual 0.045, theta 0.21, null component 0.08.  No cap had
    to be raised.

No GPU, no library."""
import numpy as np
import pytest

import pinv_reference as pr
import solve_reference as sr

LD = pr.LD
TIGHT = 2.0 ** -8                 # the longdouble results against the caps (64-bit mantissa: eps_ld = 2^-11 eps)
ids = lambda c: "%s-%d" % c if isinstance(c, tuple) else str(c)


@pytest.mark.parametrize("case", pr.CASES, ids=ids)
def test_reference_agrees_with_numpy_and_is_far_from_the_cut(case):
    c = pr.case(*case)
    S, v, p, lmax = c["S"], c["v"], c["p"], c["lmax"]
    assert np.array_equal(S, S.T)
    # the decomposition (computed or closed form) reproduces the stored matrix far inside any cap
    assert pr.residual(S, c["V"], c["lam"], lmax) <= TIGHT * sr.cap(p)
    assert pr.orthogonality(c["V"]) <= TIGHT * sr.cap(p)
    assert c["margin"] >= 4.0, c["margin"]
    # numpy's fp64 results sit within their own error of it
    assert pr.eigenvalue_error(np.linalg.eigvalsh(S), c["lam"], lmax) <= sr.cap(p)
    assert c["rank"] == np.linalg.matrix_rank(S)
    ref = np.linalg.lstsq(S, v, rcond=None)[0]
    assert pr.theta_error(ref, c["theta"]) <= pr.C(p) * float(lmax / c["min_kept"])
    if c["singular"]:
        assert pr.null_component(c["N"], c["theta"]) <= TIGHT * sr.cap(p)
        assert c["N"].shape == (p, p - c["rank"])


@pytest.mark.parametrize("case", [c for c in pr.CASES if c[1] <= 16], ids=ids)
def test_eigenvalues_against_mpmath_at_40_digits(case):
    import mpmath
    c = pr.case(*case)
    p = c["p"]
    old = mpmath.mp.dps
    mpmath.mp.dps = 40
    try:
        E = mpmath.mp.eigsy(mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in c["S"]]), eigvals_only=True)
        got = sorted(E)
        lmax = max(abs(e) for e in got)
        exact = lambda l: mpmath.mpf(float(l)) + mpmath.mpf(float(l - LD(float(l))))          # a longdouble is two doubles, exactly
        err = max(abs(exact(l) - e) for l, e in zip(np.sort(c["lam"]), got))
        assert err <= mpmath.mpf(2) ** -60 * max(p, 8) * lmax, err
    finally:
        mpmath.mp.dps = old


@pytest.mark.parametrize("p", (1, 2, 3, 7, 8, 33))
def test_closed_forms_against_the_jacobi_reference(p):
    for S, lam, V in (pr.toeplitz(p), pr.identity_plus_ones(p, 2.0, 1.0), pr.identity_plus_ones(p, 0.0, 1.0)):
        got, _ = pr.eigh_ld(S)
        assert pr.eigenvalue_error(got, lam, np.max(np.abs(lam))) <= TIGHT * sr.cap(p)
    k = np.arange(1, p + 1)
    assert np.allclose(np.asarray(pr.toeplitz(p)[1], dtype=float), 2 - 2 * np.cos(k * np.pi / (p + 1)), rtol=0, atol=1e-14)
    lam = np.asarray(pr.identity_plus_ones(p, 2.0, 1.0)[1], dtype=float)
    assert sorted(lam) == sorted([2.0] * (p - 1) + [2.0 + p])


@pytest.mark.parametrize("p", (2, 3, 7, 8, 33, 64, 65, 130))
def test_dummy_trap_has_the_known_null_vector(p):
    c = pr.case("trap", p)
    S = c["S"]
    assert np.all(S == np.round(S)) and S[0, 0] == S[0, 1:].sum() and np.array_equal(np.diag(S)[1:], S[0, 1:])
    z = pr.trap_null(p)
    assert np.all(np.dot(S, np.sign(np.asarray(z, dtype=np.float64))) == 0)      # (1, -1, .., -1): exactly, in integers
    assert c["rank"] == p - 1 and c["N"].shape[1] == 1
    n = c["N"][:, 0]
    assert float(np.max(np.abs(n * np.sign(n[0]) - z))) <= TIGHT * sr.cap(p)
    assert float(np.abs(c["dropped"][0])) <= TIGHT * sr.cap(p) * float(c["lmax"])


@pytest.mark.parametrize("p", [p for p in pr.ALL_P if pr.rep_block(p)])
def test_block_repetition_repeats_the_block_spectrum(p):
    b = pr.rep_block(p)
    c = pr.case("trap_repeated", p)
    lam_b, _ = pr.eigh_ld(pr.dummy_trap(pr.trap_counts(b - 1)))
    assert np.array_equal(c["lam"], np.sort(np.tile(lam_b, p // b)))
    assert c["rank"] == (b - 1) * (p // b)


@pytest.mark.parametrize("p", (4, 33))
def test_rcond_cases_are_far_from_every_cut(p):
    S, v = pr.rcond_case(p)
    lam, V = pr.eigh_ld(S)
    groups = [int(np.sum(np.resize(pr.RCOND_SPECTRUM, p) >= g)) for g in (1.0, 1e-3, 1e-6)]
    for rcond, rank in zip(pr.RCONDS, groups):
        r = pr.pinv_from_eig(lam, V, v, rcond)
        assert r["rank"] == rank and r["margin"] >= 4.0, (rcond, r["rank"], r["margin"])
    r = pr.pinv_from_eig(lam, V, v, 0.0)
    assert r["rank"] == p and r["margin"] == np.inf


@pytest.mark.parametrize("p", (8, 64))
@pytest.mark.parametrize("side", ("below", "above"))
def test_route_cases_are_far_from_the_cut(p, side):
    S, v = pr.route_case(p, side)
    r = pr.pinv_solve(S, v)
    assert r["margin"] >= 4.0, r["margin"]
    if side == "below":
        kappa = float(r["lmax"] / r["min_kept"])
        assert r["rank"] == p and abs(kappa * 100 * pr.EPS * p - 1) < 1e-3
        assert pr.theta_error(r["theta"], sr.solve(S, v)) <= TIGHT * sr.cap(p) * kappa      # the two longdouble solves agree
    else:
        assert r["rank"] == p - p // 4


def test_measures_see_a_structural_error():
    """the null vector tilted towards the top eigenvector by 1e-6, one eigenvalue pair swapped against V, theta with a sliver of
    the null vector: each measure leaves its cap by orders of magnitude"""
    c = pr.case("trap", 33)
    p, lam, V = 33, np.asarray(c["lam"], dtype=np.float64), np.asarray(c["V"], dtype=np.float64)
    th = np.asarray(c["theta"], dtype=np.float64)
    assert max(pr.fractions(c, lam, V, th).values()) <= 1.0
    Vb = V.copy()
    Vb[:, 0] += 1e-6 * V[:, p - 1]
    f = pr.fractions(c, lam, Vb, th)
    assert f["orth"] > 1e3 and f["resid"] > 1e2
    lb = lam.copy()
    lb[[5, 6]] = lb[[6, 5]]
    f = pr.fractions(c, lb, V, th)
    assert f["resid"] > 1e3 and f["eig"] == pr.fractions(c, lam, V, th)["eig"]          # the sorted spectrum alone does not see it
    f = pr.fractions(c, lam, V, th + 1e-9 * np.max(np.abs(th)) * np.asarray(c["N"][:, 0], dtype=np.float64))
    assert f["null"] > 1e3


def fp64_stand_in(c):
    lam, V, sweeps = pr.jacobi_eigh(c["S"], np.float64, 1e-15, max_sweeps=200)
    r = pr.pinv_from_eig(lam, V, c["v"], pr.EPS * c["p"], dtype=np.float64)
    return lam, V, r, sweeps


@pytest.mark.parametrize("case", pr.CASES, ids=ids)
def test_fp64_jacobi_stays_twice_inside_the_caps(case):
    c = pr.case(*case)
    lam, V, r, sweeps = fp64_stand_in(c)
    f = pr.fractions(c, lam, V, r["theta"])
    print("%s p=%d sweeps=%d fractions of the caps: %s" % (c["kind"], c["p"], sweeps, ", ".join("%s %.3g" % kv for kv in f.items())))
    assert r["rank"] == c["rank"]
    worst = max(f, key=f.get)
    assert f[worst] * 2.0 <= 1.0, (worst, f[worst])
