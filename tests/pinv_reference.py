"""Extended-precision reference for the spectral route of the WLS combine (dlsa_amd/csrc/eigsolve.hip): a cyclic Jacobi
eigendecomposition written out in numpy.longdouble (no LAPACK), lstsq's truncated pseudo-inverse built from it, symmetric test
matrices -- prescribed spectra and closed forms whose every entry is exact in fp64 -- and the error measures the tests assert
on, all evaluated in longdouble.  Plain CPU code: nothing here touches the GPU or the library."""
import functools

import numpy as np

from solve_reference import EPS, LD, cap

PI = LD(4) * np.arctan(LD(1))
FACTOR = 8.0                                    # the caps are C = FACTOR * cap(p) (see test_pinv_reference_cpu.py)


def C(p):
    return FACTOR * cap(p)


# ---- the eigendecomposition -------------------------------------------------------------------------------------------
def jacobi_eigh(S, dtype=LD, tol=1e-18, max_sweeps=60):
    """Sequential cyclic-by-rows Jacobi on the symmetric matrix S in `dtype`, until the off-diagonal Frobenius norm is at most
    tol |S|_F.  Returns (lam ascending, V with the eigenvectors as columns, sweeps)."""
    A = np.array(S, dtype=dtype)
    A = (A + A.T) / 2
    p = A.shape[0]
    Vt = np.eye(p, dtype=dtype)                                        # rows are the eigenvectors (row updates are contiguous)
    fro = np.sqrt(np.sum(A * A))
    skip = tol * fro / (2 * max(p, 1))                                 # (threshold Jacobi) p^2 such entries are half the target
    sweeps = 0
    R = np.zeros((2, 2), dtype=dtype)
    while sweeps < max_sweeps:
        off = np.sqrt(2 * np.sum(np.tril(A, -1) ** 2))
        if off <= tol * fro:
            break
        sweeps += 1
        for i in range(p - 1):
            for j in (i + 1 + np.nonzero(np.abs(A[i, i + 1:]) > skip)[0]):
                aij = A[i, j]
                if not abs(aij) > skip:                                # (rotations of this row may have cleared it meanwhile)
                    continue
                aii, ajj = A[i, i], A[j, j]
                tau = (ajj - aii) / (2 * aij)
                t = (1 if tau >= 0 else -1) / (abs(tau) + np.sqrt(1 + tau * tau))
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                R[0, 0], R[0, 1], R[1, 0], R[1, 1] = c, -s, s, c       # rows i, j <- c r_i - s r_j, s r_i + c r_j
                ij = [i, j]
                new = np.dot(R, A[ij])
                new[0, i], new[1, j] = aii - t * aij, ajj + t * aij
                new[0, j] = new[1, i] = 0
                A[ij] = new
                A[:, ij] = new.T
                Vt[ij] = np.dot(R, Vt[ij])
    else:
        raise np.linalg.LinAlgError("no convergence in %d sweeps" % max_sweeps)
    lam = np.diag(A).copy()
    order = np.argsort(lam, kind="stable")
    return lam[order], np.ascontiguousarray(Vt[order].T), sweeps


def eigh_ld(S):
    """(lam ascending, V) of the fp64 matrix as it is stored, in longdouble"""
    lam, V, _ = jacobi_eigh(S, LD, 1e-18)
    return lam, V


def pinv_from_eig(lam, V, v, rcond, dtype=LD):
    """lstsq's answer from an eigendecomposition: cut = rcond max|lambda|, theta = sum over |lambda_i| > cut of v_i (v_i'v) / lambda_i.
    margin: the smallest ratio, in either direction, of any |lambda| to the cut (inf for an exact zero)."""
    lam, V, v = np.asarray(lam, dtype=dtype), np.asarray(V, dtype=dtype), np.asarray(v, dtype=dtype)
    mag = np.abs(lam)
    lmax = mag.max()
    cut = dtype(rcond) * lmax
    keep = mag > cut
    theta = np.dot(V[:, keep], np.dot(V[:, keep].T, v) / lam[keep]) if keep.any() else np.zeros(len(v), dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(keep, mag / cut, cut / mag)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)                   # 0 against a cut of 0: an exact zero is dropped at any rcond
    return {"theta": theta, "rank": int(keep.sum()), "kept": lam[keep], "dropped": lam[~keep], "margin": float(ratio.min()),
            "lmax": lmax, "min_kept": mag[keep].min() if keep.any() else lmax, "N": V[:, ~keep], "cut": cut}


def pinv_solve(S, v, rcond=None):
    """the reference solve of (S, v): eigh_ld, then the cut.  rcond=None is lstsq's eps p."""
    p = np.shape(S)[0]
    lam, V = eigh_ld(S)
    return pinv_from_eig(lam, V, v, EPS * p if rcond is None else rcond)


# ---- matrices ---------------------------------------------------------------------------------------------------------
def prescribed(lam, seed):
    """Q diag(lam) Q' with Q the orthogonal factor of a seeded Gaussian matrix: the product in longdouble, rounded once to fp64,
    symmetrised.  Its eigenvalues are NEAR lam; the truth is eigh_ld of what is returned."""
    lam = np.asarray(lam, dtype=LD)
    p = len(lam)
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((p, p)))
    Q = Q.astype(LD)
    S = np.dot(Q * lam, Q.T).astype(np.float64)
    return (S + S.T) / 2


SPECTRA = {
    "linear": lambda p: np.linspace(1.0, 2.0, p),
    "clusters": lambda p: np.where(np.arange(p) < p // 2, 1.0, 2.0),
    "plusminus": lambda p: np.where(np.arange(p) % 2 == 0, 1.0, -1.0),
    "graded": lambda p: np.logspace(0.0, -12.0, p),
    "halfzero": lambda p: np.concatenate([np.linspace(1.0, 2.0, (p + 1) // 2), np.zeros(p // 2)]),
}


def toeplitz(p):
    """tridiagonal 2, -1: lambda_k = 2 - 2 cos(k pi / (p + 1)) = 4 sin^2(k pi / (2 (p + 1))), v_jk = sqrt(2 / (p + 1)) sin(j k pi / (p + 1))"""
    S = 2.0 * np.eye(p) - np.eye(p, k=1) - np.eye(p, k=-1)
    k = np.arange(1, p + 1, dtype=LD)
    lam = 4 * np.sin(k * PI / (2 * (p + 1))) ** 2
    V = np.sqrt(LD(2) / (p + 1)) * np.sin(np.outer(k, k) * PI / (p + 1))
    return S, lam, V


def identity_plus_ones(p, c, d):
    """c I + d 11': eigenvalue c on the p - 1 Helmert contrasts (1, .., 1, -k, 0, ..) / sqrt(k (k + 1)), c + p d on 1 / sqrt(p)"""
    S = c * np.eye(p) + d * np.ones((p, p))
    V = np.zeros((p, p), dtype=LD)
    for k in range(1, p):
        V[:k, k - 1] = 1
        V[k, k - 1] = -k
        V[:, k - 1] /= np.sqrt(LD(k) * (k + 1))
    V[:, p - 1] = 1 / np.sqrt(LD(p))
    lam = np.full(p, c, dtype=LD)
    lam[p - 1] = c + LD(p) * d
    return S, lam, V


def diagonal(p, seed):
    """the integers -2 .. p - 3 in a seeded order on the diagonal: unsorted, indefinite, and singular from p = 3"""
    d = np.random.default_rng(seed).permutation(np.arange(p) - 2).astype(np.float64)
    return np.diag(d), d.astype(LD), np.eye(p, dtype=LD)


def trap_counts(L):
    return np.array([1 + (5 * l + 2) % 7 for l in range(L)], dtype=np.float64)


def dummy_trap(counts):
    """X'X of an intercept beside the FULL one-hot set of a factor with the given level counts: [[N, n'], [n, diag(n)]], rank L of
    L + 1, null vector (1, -1, .., -1) / sqrt(L + 1)"""
    n = np.asarray(counts, dtype=np.float64)
    L = len(n)
    S = np.zeros((L + 1, L + 1))
    S[0, 0] = n.sum()
    S[0, 1:] = S[1:, 0] = n
    S[1:, 1:] = np.diag(n)
    return S


def trap_null(p):
    z = -np.ones(p, dtype=LD)
    z[0] = 1
    return z / np.sqrt(LD(p))


def block_repeat(B, reps):
    """diag(B, .., B): every eigenvalue of B `reps`-fold, eigenvectors those of B in each block (eigh_ld of the ONE block)"""
    b = B.shape[0]
    S = np.kron(np.eye(reps), B)
    lam_b, V_b = eigh_ld(B)
    return S, np.tile(lam_b, reps), np.kron(np.eye(reps, dtype=LD), V_b)


def hadamard(p, c, d):
    """c I + d W with W = diag(H_n / sqrt(n)) over the blocks n = 256, 64, 16, 4, 1 that fill p greedily, H_n the Sylvester
    Hadamard matrix: sqrt(n) is a power of two, so every entry is exact, the blocks are DENSE, and W W = I: the eigenvalues are
    c + d and c - d, each about p / 2 fold.  W_n is the k-fold Kronecker power of H_2 / sqrt(2), whose eigenvectors are the
    rotation by pi / 8; so are those of W_n, Kronecker powers of it."""
    u = np.array([[np.cos(PI / 8), -np.sin(PI / 8)], [np.sin(PI / 8), np.cos(PI / 8)]], dtype=LD)
    S, V, lam, at = np.zeros((p, p)), np.zeros((p, p), dtype=LD), np.zeros(p, dtype=LD), 0
    while at < p:
        n = max(b for b in (256, 64, 16, 4, 1) if b <= p - at)
        H, U, w = np.ones((1, 1)), np.ones((1, 1), dtype=LD), np.ones(1, dtype=LD)
        for _ in range(int(np.log2(n))):
            H, U, w = np.kron(H, np.array([[1.0, 1.0], [1.0, -1.0]])), np.kron(U, u), np.kron(w, np.array([1, -1], dtype=LD))
        sl = slice(at, at + n)
        S[sl, sl], V[sl, sl], lam[sl] = c * np.eye(n) + d * H / np.sqrt(n), U, c + d * w
        at += n
    return S, lam, V


def rep_block(p):
    """the block size the repetition uses at p (at least two blocks), or None"""
    for b in (5, 4, 3):
        if p % b == 0 and p // b >= 2:
            return b
    return None


# ---- the cases --------------------------------------------------------------------------------------------------------
PRESCRIBED_P = (2, 3, 7, 8, 33, 64, 65, 130)
ALL_P = (1, 2, 3, 7, 8, 33, 64, 65, 130, 257, 500)
CLOSED = ("toeplitz", "identity_plus_ones", "ones", "identity", "diagonal", "trap", "trap_repeated", "hadamard_clusters",
          "hadamard_projector")


def fits(kind, p):
    if kind in SPECTRA:
        return p in PRESCRIBED_P
    if kind == "trap":
        return 2 <= p <= 130                        # the one block is decomposed by eigh_ld
    if kind == "trap_repeated":
        return rep_block(p) is not None
    if kind == "hadamard_clusters":                 # dense two-cluster spectra {1, 2} and {0, 1} beyond the sizes eigh_ld reaches
        return p in (257, 500)
    if kind == "hadamard_projector":
        return p == 500
    return True


CASES = [(kind, p) for kind in tuple(SPECTRA) + CLOSED for p in ALL_P if fits(kind, p)]
SEED = {kind: 100 + i for i, kind in enumerate(tuple(SPECTRA) + CLOSED)}


@functools.lru_cache(maxsize=None)
def case(kind, p):
    """One shared, read-only test system per (kind, p): S, v ~ N(0, 1), the longdouble eigendecomposition (lam ascending, V) and
    the reference solve at lstsq's rcond = eps p.  Computed once, used by every test that asks for it."""
    seed = 1000 * SEED[kind] + p
    if kind in SPECTRA:
        S = prescribed(SPECTRA[kind](p), seed)
        lam, V = eigh_ld(S)
    else:
        if kind == "toeplitz":
            S, lam, V = toeplitz(p)
        elif kind == "identity_plus_ones":
            S, lam, V = identity_plus_ones(p, 2.0, 1.0)
        elif kind == "ones":
            S, lam, V = identity_plus_ones(p, 0.0, 1.0)
        elif kind == "identity":
            S, lam, V = np.eye(p), np.ones(p, dtype=LD), np.eye(p, dtype=LD)
        elif kind == "diagonal":
            S, lam, V = diagonal(p, seed)
        elif kind == "hadamard_clusters":
            S, lam, V = hadamard(p, 1.5, 0.5)
        elif kind == "hadamard_projector":
            S, lam, V = hadamard(p, 0.5, 0.5)
        elif kind == "trap":
            S = dummy_trap(trap_counts(p - 1))
            lam, V = eigh_ld(S)
        else:
            b = rep_block(p)
            S, lam, V = block_repeat(dummy_trap(trap_counts(b - 1)), p // b)
        order = np.argsort(lam, kind="stable")
        lam, V = lam[order], np.ascontiguousarray(V[:, order])
    v = np.random.default_rng(77 + seed).standard_normal(p)
    out = {"kind": kind, "p": p, "S": S, "v": v, "lam": lam, "V": V}
    out.update(pinv_from_eig(lam, V, v, EPS * p))
    out["singular"] = out["rank"] < p
    out["indefinite"] = bool(lam.min() < 0)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


RCOND_SPECTRUM = (1.0, 1e-3, 1e-6, 1e-9)
RCONDS = (3e-2, 3e-5, 3e-8)                     # cuts between the four groups, a factor 30 from either neighbour


@functools.lru_cache(maxsize=None)
def rcond_case(p):
    """the four-group spectrum, repeated to fill p, for the explicit-rcond test"""
    S = prescribed(np.resize(RCOND_SPECTRUM, p), 9000 + p)
    v = np.random.default_rng(9077 + p).standard_normal(p)
    S.setflags(write=False)
    v.setflags(write=False)
    return S, v


@functools.lru_cache(maxsize=None)
def route_case(p, side):
    """the two routes of wls_solve: three quarters of the spectrum in logspace(0, -6), the last quarter at a floor 100 times
    above lstsq's cut eps p ("below": condition number 1 / (100 eps p), every eigenvalue kept) or 100 times under it ("above":
    what is stored there is rounding noise of the entries, all of it dropped)"""
    floor = EPS * p * (100.0 if side == "below" else 0.01)
    S = prescribed(np.concatenate([np.logspace(0.0, -6.0, p - p // 4), np.full(p // 4, floor)]), 9500 + p)
    v = np.random.default_rng(9577 + p).standard_normal(p)
    S.setflags(write=False)
    v.setflags(write=False)
    return S, v


# ---- the error measures (every product and norm in longdouble) --------------------------------------------------------
def eigenvalue_error(lam_hat, lam, lmax):
    """max |sorted computed - sorted true| / max|lambda|"""
    return float(np.max(np.abs(np.sort(np.asarray(lam_hat, dtype=LD)) - np.sort(np.asarray(lam, dtype=LD)))) / lmax)


def residual(S, V_hat, lam_hat, lmax):
    """|S V - V diag(lam)|_max / max|lambda|"""
    S, V_hat, lam_hat = np.asarray(S, dtype=LD), np.asarray(V_hat, dtype=LD), np.asarray(lam_hat, dtype=LD)
    return float(np.max(np.abs(np.dot(S, V_hat) - V_hat * lam_hat)) / lmax)


def orthogonality(V_hat):
    """|V'V - I|_max"""
    V_hat = np.asarray(V_hat, dtype=LD)
    return float(np.max(np.abs(np.dot(V_hat.T, V_hat) - np.eye(V_hat.shape[1], dtype=LD))))


def theta_error(theta_hat, theta):
    """|theta - theta_ref|_inf / |theta_ref|_inf"""
    theta_hat, theta = np.asarray(theta_hat, dtype=LD), np.asarray(theta, dtype=LD)
    return float(np.max(np.abs(theta_hat - theta)) / np.max(np.abs(theta)))


def null_component(N, theta_hat):
    """|N' theta|_2 / |theta|_2 for an orthonormal basis N of the dropped space (0 for the minimum-norm solution)"""
    N, theta_hat = np.asarray(N, dtype=LD), np.asarray(theta_hat, dtype=LD)
    nt = np.sqrt(np.sum(theta_hat ** 2))
    return float(np.sqrt(np.sum(np.dot(N.T, theta_hat) ** 2)) / nt) if nt > 0 and N.shape[1] else 0.0


def fractions(c, lam_hat, V_hat, theta_hat):
    """every measure of one computed decomposition and solve of case c, as a fraction of its cap"""
    p = c["p"]
    cp = C(p)
    lmax = c["lmax"]
    out = {"eig": eigenvalue_error(lam_hat, c["lam"], lmax) / cp,
           "resid": residual(c["S"], V_hat, lam_hat, lmax) / cp,
           "orth": orthogonality(V_hat) / cp,
           "theta": theta_error(theta_hat, c["theta"]) / (cp * float(lmax / c["min_kept"]))}
    if c["singular"]:
        out["null"] = null_component(c["N"], theta_hat) / cp
    return out
