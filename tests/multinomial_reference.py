"""numpy reference of the multinomial logistic (softmax) map step: C classes coded 0 .. C - 1, class 0 the reference (eta_0 = 0),
J = C - 1, the parameter class-major theta = [beta_1 | ... | beta_J] with pe = p + intercept entries each (intercept first).  With
D = [1 | X] or X:
    eta_j = D beta_j,  p_j = e^eta_j / sum_k e^eta_k,  loglik = sum_i log p_{y_i},
    g_j = D'(1[y = j] - p_j),  H_jk = D' diag(p_j (delta_jk - p_k)) D.
The softmax of a row: M = max(0, eta_1 .. eta_J), e_k = exp(eta_k - M), T = the sum of the e_k without the first that attains M
(which is exactly 1), p_k = e_k / (1 + T), the row's term eta_y - M - log1p(T).  Every function takes a `dtype`: np.float64, or
np.longdouble for the run the fp64 one is checked against."""
import numpy as np


def design(X, intercept, dtype=np.float64):
    X = np.asarray(X, dtype=dtype)
    return np.concatenate([np.ones((X.shape[0], 1), dtype=dtype), X], 1) if intercept else X


def terms(X, y, theta, C, intercept=False, dtype=np.float64, h_cols=None):
    """(loglik, g [J pe], H [J pe, J pe], P [J, n]) at theta.  h_cols: only the first h_cols columns of every block column of H are
    formed, H is [J pe, J h_cols] (a wide H in longdouble takes long)."""
    D = design(X, intercept, dtype)
    n, pe = D.shape
    J = C - 1
    B = np.asarray(theta, dtype=dtype).reshape(J, pe)
    yi = np.asarray(y).astype(np.int64)
    full = np.concatenate([np.zeros((n, 1), dtype=dtype), D @ B.T], 1)
    M = full.max(1)
    e = np.exp(full - M[:, None])
    rest = e.copy()
    rest[np.arange(n), full.argmax(1)] = 0          # (argmax: the first index that attains the maximum)
    T = rest.sum(1)
    P = e / (1 + T)[:, None]
    ll = (full[np.arange(n), yi] - M - np.log1p(T)).sum()
    R = -P[:, 1:]
    R[np.arange(n)[yi > 0], yi[yi > 0] - 1] += 1
    g = (D.T @ R).T.reshape(-1)
    hc = pe if h_cols is None else h_cols
    H = np.zeros((J * pe, J * hc), dtype=dtype)
    for j in range(J):
        for k in range(j, J):
            w = P[:, j + 1] * ((1 if j == k else 0) - P[:, k + 1])
            blk = (D * w[:, None]).T @ D[:, :hc]
            if hc == pe:
                blk = (blk + blk.T) / 2             # (a BLAS product is symmetric up to rounding only)
            H[j * pe:(j + 1) * pe, k * hc:(k + 1) * hc] = blk
            H[k * pe:(k + 1) * pe, j * hc:(j + 1) * hc] = blk
    return ll, g, H, P[:, 1:].T.copy()


def start(y, p, C, intercept=False, dtype=np.float64):
    """theta = 0, class j's intercept at log(n_j / n_0): the exact MLE of the intercept-only model"""
    pe = p + (1 if intercept else 0)
    theta = np.zeros((C - 1, pe), dtype=dtype)
    if intercept:
        cnt = np.bincount(np.asarray(y).astype(np.int64), minlength=C).astype(dtype)
        theta[:, 0] = np.log(cnt[1:] / cnt[0])
    return theta.reshape(-1)


def _solve(H, g, dtype):
    """H^-1 g; LAPACK has no longdouble, so the wide type takes the fp64 solve with one refinement of the residual in `dtype`"""
    if dtype is np.float64:
        return np.linalg.solve(H, g)
    H64 = H.astype(np.float64)
    step = np.linalg.solve(H64, g.astype(np.float64)).astype(dtype)
    return step + np.linalg.solve(H64, (g - H @ step).astype(np.float64)).astype(dtype)


def fit(X, y, C, intercept=False, tol=1e-13, max_iter=100, dtype=np.float64):
    """The engine's safeguarded Newton loop, evaluation by evaluation: start(), an evaluated point whose likelihood is worse than
    the last accepted one's (by more than 1e-12 of it) or not finite is replaced by the midpoint towards the last accepted point (at
    most 30 times in a row), the fit stops when the next step |delta|_inf <= tol max(1, |theta|_inf).  Returns (coef, Sig_inv = H at
    coef, loglik at coef, the evaluations up to the last accepted one)."""
    X = np.asarray(X)
    theta = start(y, X.shape[1], C, intercept, dtype)
    prev, ll_prev, halvings, n_iter = None, None, 0, 0
    for it in range(max_iter + 1):
        ll, g, H, _ = terms(X, y, theta, C, intercept, dtype)
        worse = (not np.isfinite(ll)) or (ll_prev is not None and ll < ll_prev - 1e-12 * abs(ll_prev))
        if ll_prev is not None and worse and halvings < 30:
            halvings += 1
            theta = prev + (theta - prev) / 2
            continue
        halvings, n_iter = 0, it + 1
        delta = _solve(H, g, dtype)
        if np.max(np.abs(delta)) <= tol * max(1.0, np.max(np.abs(theta))):
            break
        prev, ll_prev, theta = theta, ll, theta + delta
    return theta, H, ll, n_iter


def block(X, y, C, intercept=False):
    """The DLSA block of one partition: (coef, Sig_inv, Sig_invMcoef)."""
    b, S = fit(X, y, C, intercept)[:2]
    return b, S, S @ b


def logistic_fit(X, y, intercept=False, tol=1e-13, max_iter=100):
    """A plain logistic Newton fit (y in {0, 1}) written without the softmax: what C = 2 must equal.  Returns (coef, H, loglik)."""
    D = design(X, intercept)
    y = np.asarray(y, dtype=np.float64)
    beta = np.zeros(D.shape[1])
    if intercept:
        beta[0] = np.log(y.sum() / (len(y) - y.sum()))
    for _ in range(max_iter + 1):
        eta = D @ beta
        mu = 1.0 / (1.0 + np.exp(-eta))
        ll = (y * eta - np.logaddexp(0.0, eta)).sum()
        g = D.T @ (y - mu)
        H = (D * (mu * (1.0 - mu))[:, None]).T @ D
        delta = np.linalg.solve(H, g)
        if np.max(np.abs(delta)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
        beta = beta + delta
    return beta, H, ll


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------
def true_theta(p, C, intercept):
    """class j = 1 .. C - 1: +-1 / max(1, sqrt(p / 10)) on the first max(1, int(0.4 p)) columns, the sign alternating with the class
    and growing a little with it so that no two classes share a coefficient vector; intercepts +-0.2"""
    pe = p + (1 if intercept else 0)
    B = np.zeros((C - 1, pe))
    k = max(1, int(0.4 * p))
    for j in range(1, C):
        sign = 1.0 if j % 2 else -1.0
        B[j - 1, pe - p:pe - p + k] = sign * (1.0 + 0.1 * j) / max(1.0, np.sqrt(p / 10))
        if intercept:
            B[j - 1, 0] = 0.2 * sign
    return B.reshape(-1)


def draw(rng, X, theta, C, intercept):
    """class codes drawn from the softmax at theta"""
    P = terms(X, np.zeros(len(X)), theta, C, intercept)[3]
    cdf = np.cumsum(np.concatenate([1.0 - P.sum(0, keepdims=True), P], 0), 0).T
    return np.minimum((rng.random(len(X))[:, None] > cdf).sum(1), C - 1).astype(np.float64)


def data(seed, n, p, C, intercept):
    """X ~ U(-0.5, 0.5), y drawn at true_theta; the first C rows carry the classes 0 .. C - 1, so none is absent (n >= C)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    y = draw(rng, X, true_theta(p, C, intercept), C, intercept)
    m = min(n, C)
    y[:m] = np.arange(m)
    return X, y


def away_from_optimum(m):
    return np.linspace(-0.8, 0.6, m) / max(1.0, np.sqrt(m / 10))


ETA_SPAN_CLASSES = 4


def eta_span_case():
    """n = 2000, p = 3, C = 4, intercept: the coefficients 300, -300 and 150 on a column from -1 to 1, so the eta of a row span up to
    600 across the classes and every class dominates somewhere.  Returns (X, y, theta)."""
    n, p, C = 2000, 3, ETA_SPAN_CLASSES
    X, y = data(20, n, p, C, True)
    X[:, 0] = np.linspace(-1.0, 1.0, n)
    theta = np.array([[-0.4, 300.0, 0.3, -0.2], [0.2, -300.0, -0.1, 0.4], [0.1, 150.0, 0.2, 0.1]]).reshape(-1)
    return X, y, theta


# (n, p, C, intercept) of the fits the GPU file checks against fit()
FIT_SHAPES = [(600, 7, 3, 1), (600, 7, 3, 0), (2000, 20, 5, 1), (1500, 50, 3, 1), (3000, 100, 3, 1), (400, 3, 8, 1)]

CALIBRATION_K, CALIBRATION_ROWS, CALIBRATION_CLASSES, CALIBRATION_SEED = 24, 1500, 3, 2026
CALIBRATION_TRUTH = np.array([0.3, 1.0, -1.0, 0.5, 0.0, -0.2, -0.8, 0.6, 0.0, 0.7])      # [beta_1 | beta_2], intercept first, p = 4


def calibration_case(seed=CALIBRATION_SEED):
    """CALIBRATION_K strided partitions (row i belongs to partition i % K) of CALIBRATION_ROWS rows, 4 features + intercept, 3 classes
    drawn at CALIBRATION_TRUTH: the block has dimension 10"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (CALIBRATION_K * CALIBRATION_ROWS, 4))
    return X, draw(rng, X, CALIBRATION_TRUTH, CALIBRATION_CLASSES, True)


def calibration_q(coef, Sig_inv):
    """sum_k (theta_k - theta*)' Sig_inv_k (theta_k - theta*): chi-square on K * 10 degrees of freedom when Sig_inv is the information"""
    d = np.asarray(coef) - CALIBRATION_TRUTH
    return float(np.einsum("ki,kij,kj->", d, np.asarray(Sig_inv), d))
