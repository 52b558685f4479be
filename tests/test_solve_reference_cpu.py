"""The extended-precision solver reference (tests/solve_reference.py) against numpy.linalg, and the condition that makes the
caps of tests/test_gpu_newton_solvers.py honest: plain fp64 stand-ins for the routes of chol.hip -- numpy.linalg.solve for the
factor routes, the factor's explicit inverse, a ten-line numpy sweep inverse -- stay at least FOUR TIMES inside every cap on every
(p, kappa) the GPU file uses.  No GPU, no library."""
import numpy as np
import pytest

import solve_reference as sr

BLOCKED_P = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 113, 257, 500)
SWEEP_P = (1, 2, 3, 55, 56, 57, 63, 64, 65, 100, 111, 112)
KAPPAS = (10.0, 1e6, 1e10)
MARGIN = 4.0


def sweep_inverse(S):
    """A -> -A^-1 by the sweep operator on every pivot in turn, in fp64 (the arithmetic of spd_inverse_small_kernel)"""
    A = np.array(S, dtype=np.float64)
    for k in range(A.shape[0]):
        d = A[k, k]
        s = A[:, k].copy()
        s[k] = d - 1.0
        A -= np.outer(s, s) / d
        A[k, k] = -1.0 / d
    return -A


@pytest.mark.parametrize("p", (1, 2, 5, 33, 64, 130))
@pytest.mark.parametrize("kappa", KAPPAS)
def test_reference_agrees_with_numpy_linalg(p, kappa):
    c = sr.case(p, kappa, seed=1)
    S, v, k = c["S"], c["v"], c["kappa"]
    assert abs(k / (kappa if p > 1 else 1.0) - 1) < 1e-4                 # the matrix has the condition number it was built for
    L = sr.cholesky(S)
    assert L.dtype == np.longdouble and np.all(np.triu(L, 1) == 0)
    assert sr.factor_residual(L, S) < 4 * np.finfo(np.longdouble).eps * p
    # numpy's fp64 results sit within their own error of the longdouble ones
    assert sr.forward_error(np.linalg.solve(S, v), c["x"]) <= sr.cap(p) * k
    Hinv = sr.inverse(S, L)
    assert np.max(np.abs(np.linalg.inv(S) - Hinv)) <= sr.cap(p) * k * float(np.max(np.abs(Hinv)))
    assert float(np.max(np.abs(np.linalg.cholesky(S) - L))) <= sr.cap(p) * k
    # and the longdouble results are far more exact than any cap (64-bit mantissa: eps_ld = 2^-11 eps)
    tight = 2.0 ** -8
    assert sr.backward_error(S, c["x"], v) <= tight * sr.cap(p)
    assert sr.identity_residual(Hinv, S) <= tight * sr.cap(p) * k
    assert sr.asymmetry(Hinv) <= sr.cap(p)


def test_measures_see_a_structural_error():
    """one wrong term in a factor, one dropped column of an inverse: every measure leaves its cap by orders of magnitude"""
    c = sr.case(65, 10.0, seed=1)
    S, v, k = c["S"], c["v"], c["kappa"]
    L = np.asarray(sr.cholesky(S), dtype=np.float64)
    Lb = L.copy()
    Lb[64, 63] = 0.0                                                     # the panel's last column against the 1-row block
    xb = np.asarray(sr.backward(Lb, sr.forward(Lb, v)), dtype=np.float64)
    assert sr.backward_error(S, xb, v) > 1e3 * sr.cap(65)
    assert sr.forward_error(xb, c["x"]) > 1e3 * sr.cap(65) * k
    assert sr.factor_residual(Lb, S) > 1e3 * sr.cap(65)
    H = np.asarray(sr.inverse(S), dtype=np.float64)
    H[:, 64] = 0.0
    assert sr.identity_residual(H, S) > 0.5 and sr.asymmetry(H) > 1e3 * sr.cap(65) * k


def test_indefinite_matrix_is_refused():
    S = np.array(sr.case(5, 10.0, seed=1)["S"])
    S[3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        sr.cholesky(S)


@pytest.mark.parametrize("p", sorted(set(BLOCKED_P) | set(SWEEP_P)))
@pytest.mark.parametrize("kappa", KAPPAS)
def test_fp64_stand_ins_stay_four_times_inside_the_caps(p, kappa):
    c = sr.case(p, kappa)
    S, v, k, x = c["S"], c["v"], c["kappa"], c["x"]
    cp = sr.cap(p)
    got = {}
    if p in BLOCKED_P:
        xs = np.linalg.solve(S, v)
        L = np.linalg.cholesky(S)
        Linv = np.linalg.solve(L, np.eye(p))
        xe = Linv.T @ (Linv @ v)
        got.update({"solve eta": sr.backward_error(S, xs, v) / cp, "solve forward": sr.forward_error(xs, x) / (cp * k),
                    "factor": sr.factor_residual(L, S) / cp, "Linv L": sr.identity_residual(Linv, L) / (cp * k),
                    "inverse eta": sr.backward_error(S, xe, v) / cp, "inverse forward": sr.forward_error(xe, x) / (cp * k),
                    "Linv'Linv S": sr.identity_residual(np.dot(Linv.T.astype(sr.LD), Linv.astype(sr.LD)), S) / (cp * k)})
    if p in SWEEP_P:
        H = sweep_inverse(S)
        xw = H @ v
        got.update({"sweep eta": sr.backward_error(S, xw, v) / cp, "sweep forward": sr.forward_error(xw, x) / (cp * k),
                    "sweep Hinv S": sr.identity_residual(H, S) / (cp * k), "sweep symmetry": sr.asymmetry(H) / (cp * k)})
    print("p=%d kappa=%.0e fractions of the caps: %s" % (p, kappa, ", ".join("%s %.3g" % kv for kv in got.items())))
    worst = max(got, key=got.get)
    assert got[worst] * MARGIN <= 1.0, (worst, got[worst])


def test_eta_alone_at_the_lds_limit_of_the_inverse_apply():
    """p = 2036 (the GPU file checks eta only there: the longdouble factor is too slow)"""
    p = 2036
    S = sr.spd_matrix(p, 1e6, p)
    v = np.random.default_rng(p).standard_normal(p)
    L = np.linalg.cholesky(S)
    Linv = np.linalg.solve(L, np.eye(p))
    assert sr.backward_error(S, Linv.T @ (Linv @ v), v) * MARGIN <= sr.cap(p)
