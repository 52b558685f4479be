"""numpy reference of the ordinal (proportional-odds, cumulative logit) map step: C ordered classes coded 0 .. C - 1, J = C - 1,
    logit P(y <= j) = alpha_{j+1} - x'beta,  j = 0 .. J - 1,      theta = [alpha_1 .. alpha_J | beta_1 .. beta_p].
For a row of class c with eta = x'beta, u = alpha_{c+1} - eta, l = alpha_c - eta and F the logistic cdf:
    A = F(u), Abar = F(-u), B = F(l), Bbar = F(-l)    (top class: A = 1, Abar = 0; class 0: B = 0, Bbar = 1)
    E_c = -expm1(-(alpha_{c+1} - alpha_c)) for an interior class, 1 for the two end classes
    log P(y = c) = log A + log Bbar + log E,  dl/deta = B - Abar (= A + B - 1),  w = A Abar + B Bbar
    s_u = Abar / (Bbar E),  s_l = B / (A E),  q = s_u s_l
    g_beta = X'(B - Abar),  g_alpha_j = sum_{y = j-1} s_u - sum_{y = j} s_l
    N_bb = X' diag(w) X,  N_{alpha_j beta} = X'v_j,  v_j = -(1[y = j-1] A Abar + 1[y = j] B Bbar)
    N_{alpha_j alpha_j} = sum_{y = j-1} (A Abar + q) + sum_{y = j} (B Bbar + q),  N_{alpha_j alpha_j+1} = -sum_{y = j} q.
F(t), F(-t) and log F(t) come from e^{-|t|}.  Cutpoints that are not strictly increasing give loglik = NaN.  Every function takes a
`dtype`: np.float64, or np.longdouble for the run the fp64 one is checked against.

Recorded on the CPU (test_ordinal_cpu.py asserts them):
    terms() against central differences of itself in longdouble (h = 1e-6): score 3.4e-12, information 6.7e-12;
    fp64 against longdouble, relative l-inf of (loglik, g, H, w): <= 1.8e-15 at away_from_optimum, (1.9e-16, 3.4e-16, 3.3e-16,
    8.7e-15) in the extreme case (asserted at 1e-13);
    the fits of FIT_SHAPES: every class present (smallest class count 38), 5 - 6 evaluations, condition number <= 8.5e1;
    the calibration case's Q of this reference alone: CALIBRATION_Q_REFERENCE (within 2 standard deviations of 168)."""
import numpy as np


def _logistic(t):
    """(F(t), F(-t), log F(t)) from e^{-|t|}"""
    e = np.exp(-np.abs(t))
    big = 1 / (1 + e)
    small = e * big
    pos = t >= 0
    return np.where(pos, big, small), np.where(pos, small, big), np.where(pos, 0, t) - np.log1p(e)


def terms(X, y, theta, C, dtype=np.float64):
    """(loglik, g [d], H [d, d], w [n]) at theta = [alpha | beta], d = C - 1 + p"""
    X = np.asarray(X, dtype=dtype)
    n, p = X.shape
    J = C - 1
    theta = np.asarray(theta, dtype=dtype)
    al, beta = theta[:J], theta[J:]
    yi = np.asarray(y).astype(np.int64)
    eta = X @ beta
    one, zero = dtype(1), dtype(0)
    top, bot = yi == J, yi == 0
    E = np.ones(C, dtype=dtype)
    with np.errstate(all="ignore"):
        E[1:J] = -np.expm1(-(al[1:] - al[:-1]))
        A, Ab, lA = _logistic(al[np.minimum(yi, J - 1)] - eta)
        Bb, B, lBb = _logistic(eta - al[np.maximum(yi - 1, 0)])
        A, Ab, lA = np.where(top, one, A), np.where(top, zero, Ab), np.where(top, zero, lA)
        B, Bb, lBb = np.where(bot, zero, B), np.where(bot, one, Bb), np.where(bot, zero, lBb)
        Ey = E[yi]
        ll = (lA + lBb + np.log(Ey)).sum()
        if not np.all(al[1:] > al[:-1]):
            ll = dtype(np.nan)
        aa, bb = A * Ab, B * Bb
        su, sl = Ab / (Bb * Ey), B / (A * Ey)
        q = su * sl
    w = aa + bb
    d = J + p
    g = np.zeros(d, dtype=dtype)
    H = np.zeros((d, d), dtype=dtype)
    g[J:] = X.T @ (B - Ab)
    Hbb = (X * w[:, None]).T @ X
    H[J:, J:] = (Hbb + Hbb.T) / 2                # (a BLAS product is symmetric up to rounding only)
    for j in range(J):
        up, lo = yi == j, yi == j + 1
        g[j] = su[up].sum() - sl[lo].sum()
        v = -(np.where(up, aa, zero) + np.where(lo, bb, zero))
        H[j, J:] = H[J:, j] = X.T @ v
        H[j, j] = (aa + q)[up].sum() + (bb + q)[lo].sum()
        if j + 1 < J:
            H[j, j + 1] = H[j + 1, j] = -q[lo].sum()
    return ll, g, H, w


def start(y, p, C, dtype=np.float64):
    """beta = 0, alpha_j = the logit of the cumulative class share: the exact MLE of the null model"""
    cnt = np.bincount(np.asarray(y).astype(np.int64), minlength=C).astype(dtype)
    cum = np.cumsum(cnt)[:C - 1]
    return np.concatenate([np.log(cum / (cnt.sum() - cum)), np.zeros(p, dtype=dtype)])


def _solve(H, g, dtype):
    """H^-1 g; LAPACK has no longdouble, so the wide type takes the fp64 solve with one refinement of the residual in `dtype`"""
    if dtype is np.float64:
        return np.linalg.solve(H, g)
    H64 = H.astype(np.float64)
    step = np.linalg.solve(H64, g.astype(np.float64)).astype(dtype)
    return step + np.linalg.solve(H64, (g - H @ step).astype(np.float64)).astype(dtype)


def fit(X, y, C, tol=1e-13, max_iter=100, dtype=np.float64):
    """The engine's safeguarded Newton loop, evaluation by evaluation: start(), an evaluated point whose likelihood is worse than
    the last accepted one's (by more than 1e-12 of it) or not finite (crossed cutpoints) is replaced by the midpoint towards the last
    accepted point (at most 30 times in a row), the fit stops when the next step |delta|_inf <= tol max(1, |theta|_inf).  Returns
    (coef, Sig_inv = H at coef, loglik at coef, the evaluations up to the last accepted one)."""
    X = np.asarray(X)
    theta = start(y, X.shape[1], C, dtype)
    prev, ll_prev, halvings, n_iter = None, None, 0, 0
    for it in range(max_iter + 1):
        ll, g, H, _ = terms(X, y, theta, C, dtype)
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


def block(X, y, C):
    """The DLSA block of one partition: (coef, Sig_inv, Sig_invMcoef)."""
    b, S = fit(X, y, C)[:2]
    return b, S, S @ b


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------
def true_theta(p, C):
    """cutpoints at the logits of j / C (equal class shares at eta = 0), beta = 1 / max(1, sqrt(p / 10)) with alternating sign on the
    first max(1, int(0.4 p)) columns"""
    share = np.arange(1, C) / C
    beta = np.zeros(p)
    k = max(1, int(0.4 * p))
    beta[:k] = np.where(np.arange(k) % 2 == 0, 1.0, -1.0) / max(1.0, np.sqrt(p / 10))
    return np.concatenate([np.log(share / (1 - share)), beta])


def draw(rng, X, theta, C):
    """class codes drawn from the model at theta: the number of cutpoints whose cumulative probability a uniform draw exceeds"""
    J = C - 1
    cdf = 1.0 / (1.0 + np.exp(-(theta[None, :J] - (X @ theta[J:])[:, None])))
    return (rng.random(len(X))[:, None] > cdf).sum(1).astype(np.float64)


def data(seed, n, p, C):
    """X ~ U(-0.5, 0.5), y drawn at true_theta; the first C rows carry the classes 0 .. C - 1, so none is absent (n >= C)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    y = draw(rng, X, true_theta(p, C), C)
    m = min(n, C)
    y[:m] = np.arange(m)
    return X, y


def away_from_optimum(p, C):
    """strictly increasing cutpoints from -1 to 1.3, beta from -0.8 to 0.6 scaled like true_theta"""
    return np.concatenate([np.linspace(-1.0, 1.3, C - 1), np.linspace(-0.8, 0.6, p) / max(1.0, np.sqrt(p / 10))])


def unordered(p, C):
    """away_from_optimum with the last two cutpoints exchanged (C >= 3)"""
    theta = away_from_optimum(p, C)
    theta[[C - 3, C - 2]] = theta[[C - 2, C - 3]]
    return theta


EXTREME_CLASSES = 5


def extreme_case():
    """n = 2000, p = 3, C = 5: the coefficient 400 on a column from -1 to 1 and the cutpoints -200, -50, -50 + 1e-6, 150, so |u| and
    |l| reach 600 and the cutpoints of class 2 are 1e-6 apart.  Nine rows in ten carry the class that is the likely one at their eta
    (0, 1, 3 and 4 each over a stretch of the column; class 2, with P <= 2.5e-7 everywhere, can be that nowhere), every tenth row
    carries the class (i / 10) % 5 wherever it lies: that puts every class, class 2 included, at both ends of the column.  Returns
    (X, y, theta)."""
    n, p, C = 2000, 3, EXTREME_CLASSES
    X, _ = data(20, n, p, C)
    X[:, 0] = np.linspace(-1.0, 1.0, n)
    theta = np.array([-200.0, -50.0, -50.0 + 1e-6, 150.0, 400.0, 0.3, -0.2])
    eta = X @ theta[4:]
    y = (eta[:, None] > theta[None, :4]).sum(1).astype(np.float64)
    y[::10] = (np.arange(0, n, 10) // 10) % C
    return X, y, theta


# (n, p, C) of the passes and of the fits the GPU file checks against terms() and fit()
PASS_SHAPES = [(6001, 5, 3), (6001, 5, 8), (4001, 1, 2), (4001, 2, 4), (5003, 127, 3), (5003, 128, 3), (5003, 129, 3), (4001, 130, 8),
               (3001, 257, 5), (2001, 600, 3)]
FIT_SHAPES = [(600, 7, 3), (2000, 20, 5), (400, 3, 8), (3000, 100, 3), (1500, 50, 4), (300, 5, 2), (4001, 130, 8)]

CALIBRATION_K, CALIBRATION_ROWS, CALIBRATION_CLASSES, CALIBRATION_SEED = 24, 1500, 4, 2026
CALIBRATION_TRUTH = np.array([-1.0, 0.2, 1.1, 1.0, -1.0, 0.5, 0.0])      # [alpha_1 .. alpha_3 | beta], p = 4: d = 7
CALIBRATION_DF = CALIBRATION_K * 7                                         # 168
CALIBRATION_Q_REFERENCE = 169.59    # this reference's own Q at CALIBRATION_SEED: 0.09 standard deviations (sqrt(336) = 18.33) from 168


def calibration_case(seed=CALIBRATION_SEED):
    """CALIBRATION_K strided partitions (row i belongs to partition i % K) of CALIBRATION_ROWS rows, 4 features, 4 classes drawn at
    CALIBRATION_TRUTH: the block has dimension 7"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (CALIBRATION_K * CALIBRATION_ROWS, 4))
    return X, draw(rng, X, CALIBRATION_TRUTH, CALIBRATION_CLASSES)


def calibration_q(coef, Sig_inv):
    """sum_k (theta_k - theta*)' Sig_inv_k (theta_k - theta*): chi-square on K * 7 degrees of freedom when Sig_inv is the information"""
    d = np.asarray(coef) - CALIBRATION_TRUTH
    return float(np.einsum("ki,kij,kj->", d, np.asarray(Sig_inv), d))
