"""Extended-precision reference for the Newton-step solvers (dlsa_amd/csrc/chol.hip): SPD test matrices of known condition
number, a Cholesky solve and inverse written out in numpy.longdouble (no LAPACK), and the error measures the solver tests
assert on, all evaluated in longdouble.  Plain CPU code: nothing here touches the GPU or the library."""
import functools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def spd_matrix(p, kappa, seed):
    """S = Q diag(lambda) Q' with lambda = logspace(0, -log10 kappa, p) and Q the orthogonal factor of a seeded Gaussian
    matrix, symmetrised: an fp64 SPD matrix whose entries are O(1) and whose 2-norm condition number is kappa (1 at p = 1)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    lam = np.logspace(0.0, -np.log10(kappa), p)
    S = (Q * lam) @ Q.T
    return (S + S.T) / 2


def cond2(S):
    """the matrix's own 2-norm condition number (symmetric eigenvalues of the fp64 matrix as it is stored)"""
    ev = np.abs(np.linalg.eigvalsh(np.asarray(S, dtype=np.float64)))
    return float(ev.max() / ev.min())


def cap(p):
    """c = max(p, 8) eps: the n eps class constant of the caps (p eps; 8 eps where p eps would be below the handful of
    roundings that a solve of any size makes)"""
    return max(p, 8) * EPS


def cholesky(S):
    """lower Cholesky factor of S in longdouble, column by column (raises on a non-positive pivot)"""
    A = np.array(S, dtype=LD)
    p = A.shape[0]
    L = np.zeros((p, p), dtype=LD)
    for j in range(p):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < p:
            L[j + 1:, j] = (A[j + 1:, j] - np.dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


def forward(L, B):
    """solve L Y = B (L lower triangular; B a vector or a matrix of columns)"""
    Y = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        Y[i] = (Y[i] - np.dot(L[i, :i], Y[:i])) / L[i, i]
    return Y


def backward(L, B):
    """solve L' X = B"""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - np.dot(L[i + 1:, i], X[i + 1:])) / L[i, i]
    return X


def solve(S, v, L=None):
    """x = S^-1 v by the longdouble factor"""
    L = cholesky(S) if L is None else L
    return backward(L, forward(L, v))


def inverse(S, L=None):
    """S^-1 = Linv' Linv with Linv = L^-1 by forward substitution on the identity"""
    L = cholesky(S) if L is None else L
    Linv = forward(L, np.eye(L.shape[0], dtype=LD))
    return np.dot(Linv.T, Linv)


@functools.lru_cache(maxsize=None)
def case(p, kappa, seed=0):
    """One shared, read-only test system per (p, kappa): S, v ~ N(0, 1), the matrix's condition number and the longdouble
    solution.  Computed once, used by every test that asks for it."""
    S = spd_matrix(p, kappa, 1000 * seed + p)
    v = np.random.default_rng(77 + 1000 * seed + p).standard_normal(p)
    x = solve(S, v)
    S.setflags(write=False)
    v.setflags(write=False)
    x.setflags(write=False)
    return {"S": S, "v": v, "kappa": cond2(S), "x": x}


# ---- the error measures (every product and norm in longdouble) --------------------------------------------------------
def backward_error(S, x_hat, v):
    """normwise backward error  eta = |v - S x|_inf / (|S|_inf |x|_inf + |v|_inf)"""
    S, x_hat, v = np.asarray(S, dtype=LD), np.asarray(x_hat, dtype=LD), np.asarray(v, dtype=LD)
    r = v - np.dot(S, x_hat)
    return float(np.max(np.abs(r)) / (np.max(np.sum(np.abs(S), axis=1)) * np.max(np.abs(x_hat)) + np.max(np.abs(v))))


def forward_error(x_hat, x_ref):
    """|x - x_ref|_inf / |x_ref|_inf"""
    x_hat, x_ref = np.asarray(x_hat, dtype=LD), np.asarray(x_ref, dtype=LD)
    return float(np.max(np.abs(x_hat - x_ref)) / np.max(np.abs(x_ref)))


def identity_residual(A, B):
    """|A B - I|_max  (A = Hinv, B = S;  A = Linv, B = L)"""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    return float(np.max(np.abs(np.dot(A, B) - np.eye(A.shape[0], dtype=LD))))


def factor_residual(L_hat, S):
    """|L L' - S|_max over the lower triangle, relative to |S|_max"""
    L_hat, S = np.asarray(L_hat, dtype=LD), np.asarray(S, dtype=LD)
    return float(np.max(np.abs(np.tril(np.dot(L_hat, L_hat.T) - S))) / np.max(np.abs(S)))


def asymmetry(H):
    """|H - H'|_max / |H|_max"""
    H = np.asarray(H, dtype=np.float64)
    return float(np.max(np.abs(H - H.T)) / np.max(np.abs(H)))
