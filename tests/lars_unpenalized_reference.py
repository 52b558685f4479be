"""Reference for the LARS path with several unpenalised coefficients (a helper, not a conftest; numpy only).

The oracle (oracle/dlsa_oracle.py: lars_lsa) knows the reference's ONE unpenalised coefficient at position 0.  For a set U of them
the problem is reduced on the host by the block Schur complement -- with R the remaining indices in their original order,

    A11 = S[U, U]   A12 = S[U, R]   A22 = S[R, R]        Sigma = A22 - A12' A11^-1 A12        W = A11^-1 A12

-- and the oracle runs on (Sigma, b[R]) without an intercept: for |U| = 1 this is exactly what its intercept branch does
(lsa.py:98-104).  beta0_k = W (b[R] - beta_k) (lsa.py:203-205 for |U| = 1: b[U] is not included) and theta_k is the whole coefficient
vector in the caller's order, theta_k[U] = b[U] + beta0_k, theta_k[R] = beta_k.

reduce() works in float64 or in numpy.longdouble (numpy.linalg has no longdouble: the u x u solve is a Gauss-Jordan elimination
with partial pivoting written here, u <= 32); the path itself is the oracle's, float64.  The problems of the tests are here too, so
that the CPU and the GPU file run the same ones and the oracle runs are shared (functools.lru_cache; the results are read-only)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lars_problems  # noqa: E402
from oracle import dlsa_oracle as orc  # noqa: E402


def rest(p, U):
    chosen = set(int(i) for i in U)
    return [j for j in range(p) if j not in chosen]


def _solve(A, B):
    """A^-1 B in the dtype of A (Gauss-Jordan, partial pivoting)"""
    A, B = A.copy(), B.copy()
    u = A.shape[0]
    for k in range(u):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            B[[k, piv]] = B[[piv, k]]
        d = A[k, k]
        A[k] = A[k] / d
        B[k] = B[k] / d
        for r in range(u):
            if r != k:
                f = A[r, k]
                A[r] = A[r] - f * A[k]
                B[r] = B[r] - f * B[k]
    return B


def reduce(S, b, U, dtype=np.float64):
    """(Sigma [m, m], b[R] [m], W [u, m], R) of the problem (S, b) with the coefficients U unpenalised, computed in `dtype` and
    returned in it; Sigma is symmetrised ((X + X') / 2: the two halves differ by rounding)."""
    S = np.asarray(S, dtype=dtype)
    b = np.asarray(b, dtype=dtype).ravel()
    U = [int(i) for i in U]
    R = rest(S.shape[0], U)
    if not U:
        return S.copy(), b.copy(), np.zeros((0, len(R)), dtype=dtype), R
    A11, A12, A22 = S[np.ix_(U, U)], S[np.ix_(U, R)], S[np.ix_(R, R)]
    W = _solve(A11, A12)
    Sig = A22 - A12.T @ W
    return (Sig + Sig.T) / 2, b[R], W, R


def path(S, b, U, n, type="lar", dtype=np.float64, max_steps=None):
    """{'beta' [K+1, m], 'beta0' [K+1, u], 'theta' [K+1, p], 'AIC', 'BIC', 'R'}: the oracle's path of the reduced problem"""
    Sig, bR, W, R = reduce(S, b, U, dtype)
    r = orc.lars_lsa(np.asarray(Sig, dtype=np.float64), np.asarray(bR, dtype=np.float64), False, n, type=type, max_steps=max_steps)
    beta = np.asarray(r["beta"], dtype=np.float64)
    beta0 = np.asarray((bR[None, :] - beta.astype(dtype)) @ W.T, dtype=np.float64)
    theta = np.zeros((beta.shape[0], len(R) + len(U)))
    theta[:, R] = beta
    if len(U):
        theta[:, [int(i) for i in U]] = np.asarray(b, dtype=np.float64).ravel()[[int(i) for i in U]][None, :] + beta0
    return {"beta": beta, "beta0": beta0, "theta": theta, "AIC": np.asarray(r["AIC"], float).ravel(), "BIC": np.asarray(r["BIC"], float).ravel(), "R": R}


def rel(a, b):
    """relative l-infinity distance of a from b"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return float("inf")
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b)))) if a.size else 0.0


# ---- the problems ---------------------------------------------------------------------------------------------------------------
def multinomial_information(J, pe, seed=0):
    """(S, b, n, U): the information matrix of a softmax fit with J = C - 1 non-reference classes on n rows [1 | x], class-major
    (block (j, k) = X' diag(pi_j (delta_jk - pi_k)) X), an estimate b near the coefficients that drew pi, and U = the class
    intercepts j pe."""
    rng = np.random.default_rng(1000 * J + pe + seed)
    n = 40 * J * pe
    X = np.column_stack([np.ones(n), rng.random((n, pe - 1)) - 0.5])
    B = np.zeros((pe, J))
    B[0] = 0.3 * rng.standard_normal(J)
    B[1:1 + max(1, (pe - 1) * 2 // 5)] = rng.choice([-1.0, 1.0], size=(max(1, (pe - 1) * 2 // 5), J))
    eta = np.column_stack([np.zeros(n), X @ B])
    pr = np.exp(eta - eta.max(1, keepdims=True))
    pr = (pr / pr.sum(1, keepdims=True))[:, 1:]
    S = np.zeros((J * pe, J * pe))
    for j in range(J):
        for k in range(J):
            w = pr[:, j] * ((1.0 if j == k else 0.0) - pr[:, k])
            S[j * pe:(j + 1) * pe, k * pe:(k + 1) * pe] = X.T @ (w[:, None] * X)
    S = (S + S.T) / 2
    b = B.T.ravel() + 0.05 * rng.standard_normal(J * pe)
    return S, b, n, [j * pe for j in range(J)]


MULTINOMIAL_SHAPES = ((2, 6), (7, 6), (2, 41), (7, 41))
# lars_problems "corr" problems whose REDUCED lasso paths have drops (more steps than variables): (p, rho, seed) -> m = p - 7
CORR_CASES = ((127, 0.98, 12), (264, 0.97, 3), (456, 0.97, 5))


def corr_problem(p, rho, seed):
    S, b, n = lars_problems.problem(("corr", p, rho, seed))
    U = sorted(int(i) for i in np.random.default_rng(seed).choice(p, 7, replace=False))
    return S, b, n, U


@functools.lru_cache(maxsize=None)
def problem(name):
    """name: ("multinomial", J, pe) or ("corr", p, rho, seed) -> (S, b, n, U, type), read-only arrays"""
    if name[0] == "multinomial":
        S, b, n, U = multinomial_information(name[1], name[2])
        typ = "lar"
    else:
        S, b, n, U = corr_problem(*name[1:])
        typ = "lasso"
    S.setflags(write=False)
    b.setflags(write=False)
    return S, b, n, U, typ


@functools.lru_cache(maxsize=None)
def problem_path(name, dtype_name="float64"):
    S, b, n, U, typ = problem(name)
    r = path(S, b, U, n, typ, dtype={"float64": np.float64, "longdouble": np.longdouble}[dtype_name])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


PROBLEMS = tuple(("multinomial", J, pe) for J, pe in MULTINOMIAL_SHAPES) + tuple(("corr",) + c for c in CORR_CASES)
