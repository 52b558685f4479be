"""numpy reference of the Tweedie (compound Poisson-Gamma) map step (log link, variance power 1 < xi < 2, optional offset, optional
intercept as column 0 of the design): the quasi-log-likelihood at a dispersion, score, observed information, the Pearson and
deviance sums, and the per-partition Newton fit with the block it returns.  With a = mu^(1 - xi) = exp((1 - xi) eta), b = mu^(2 - xi)
= exp((2 - xi) eta) and nu = 1 / dispersion:
    loglik = nu sum (y a / (1 - xi) - b / (2 - xi)),  g = nu D'(y a - b),  H = nu D' diag((xi - 1) y a + (2 - xi) b) D,
    P = sum (y - mu)^2 mu^-xi,  Dev = 2 sum (y^(2 - xi) / ((1 - xi)(2 - xi)) - y a / (1 - xi) + b / (2 - xi)) with y^(2 - xi) = 0 at y = 0,
    estimated dispersion = P / (n - pe).
loglik is the part of the log density that depends on beta; the series factor of the density is left out.  Every function takes a
`dtype`: np.float64, or np.longdouble for the run the fp64 one is checked against."""
import numpy as np


def design(X, intercept, dtype=np.float64):
    X = np.asarray(X, dtype=dtype)
    return np.concatenate([np.ones((X.shape[0], 1), dtype=dtype), X], 1) if intercept else X


def _eta(X, beta, offset, intercept, dtype):
    eta = design(X, intercept, dtype) @ np.asarray(beta, dtype=dtype)
    return eta if offset is None else eta + np.asarray(offset, dtype=dtype)


def terms(X, y, beta, power, offset=None, intercept=False, dispersion=1.0, dtype=np.float64, h_cols=None):
    """(loglik, g, H, w, P, Dev) at beta, the power and the given dispersion, with D = [1 | X] or X; w is the weight per row at unit
    dispersion.  Scalars are returned in `dtype`.  h_cols: only the first h_cols columns of H (a wide H in longdouble takes long)."""
    D = design(X, intercept, dtype)
    y = np.asarray(y, dtype=dtype)
    eta = _eta(X, beta, offset, intercept, dtype)
    c1, c2 = dtype(1) - dtype(power), dtype(2) - dtype(power)
    nu = dtype(1) / dtype(dispersion)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):      # (a step that overflows mu is rejected by fit's halving)
        a, b = np.exp(c1 * eta), np.exp(c2 * eta)
        ya = y * a
        w = -c1 * ya + c2 * b
        ll = nu * (ya / c1 - b / c2).sum()
        g = nu * (D.T @ (ya - b))
        H = nu * ((D * w[:, None]).T @ D[:, :h_cols])
        d = y - np.exp(eta)
        P = (d * d * np.exp(-dtype(power) * eta)).sum()
        pos = y > 0
        yp = np.zeros_like(y)
        yp[pos] = np.exp(c2 * np.log(y[pos]))
        dev = 2 * (yp / (c1 * c2) - ya / c1 + b / c2).sum()
    return ll, g, H, w, P, dev


def start(X, y, power, offset=None, intercept=False, dtype=np.float64):
    """beta = 0, the intercept at log(sum y e^((1 - xi) o) / sum e^((2 - xi) o)): the exact MLE of the intercept-only model"""
    y = np.asarray(y, dtype=dtype)
    beta = np.zeros(np.asarray(X).shape[1] + (1 if intercept else 0), dtype=dtype)
    if intercept:
        o = np.zeros(len(y), dtype=dtype) if offset is None else np.asarray(offset, dtype=dtype)
        c1, c2 = dtype(1) - dtype(power), dtype(2) - dtype(power)
        beta[0] = np.log((y * np.exp(c1 * o)).sum() / np.exp(c2 * o).sum())
    return beta


def _solve(H, g, dtype):
    """H^-1 g; LAPACK has no longdouble, so the wide type takes the fp64 solve with one refinement of the residual in `dtype`
    (Newton corrects what is left: the iterate converges in the type the terms are evaluated in)"""
    if dtype is np.float64:
        return np.linalg.solve(H, g)
    H64 = H.astype(np.float64)
    step = np.linalg.solve(H64, g.astype(np.float64)).astype(dtype)
    return step + np.linalg.solve(H64, (g - H @ step).astype(np.float64)).astype(dtype)


def fit(X, y, power, offset=None, intercept=False, dispersion=None, tol=1e-14, max_iter=100, dtype=np.float64):
    """Newton from start() with step halving, at unit dispersion (beta does not depend on it); then the dispersion (the given one,
    or Pearson's P / (n - pe)) scales the information.  Returns (coef, Sig_inv = H / dispersion at coef, loglik at (coef, that
    dispersion), the dispersion, P, Dev)."""
    def ev(b, phi=1.0):
        return terms(X, y, b, power, offset, intercept, phi, dtype)
    beta = start(X, y, power, offset, intercept, dtype)
    ll, g, H = ev(beta)[:3]
    for _ in range(max_iter):
        step = _solve(H, g, dtype)
        t = dtype(1)
        for _ in range(30):
            ll_new, g_new, H_new = ev(beta + t * step)[:3]
            if np.isfinite(ll_new) and ll_new >= ll - 1e-12 * abs(ll):
                break
            t = t / 2
        beta = beta + t * step
        ll, g, H = ll_new, g_new, H_new
        if np.max(np.abs(t * step)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
    _, _, H, _, P, dev = ev(beta)
    phi = P / (len(y) - len(beta)) if dispersion is None else dtype(dispersion)
    return beta, H / phi, ev(beta, phi)[0], phi, P, dev


def block(X, y, power, offset=None, intercept=False, dispersion=None):
    """The DLSA block of one partition: (coef, Sig_inv, Sig_invMcoef)."""
    b, S = fit(X, y, power, offset, intercept, dispersion)[:2]
    return b, S, S @ b


def draw(rng, mu, power, dispersion):
    """compound Poisson-Gamma draws with mean mu and variance dispersion * mu^power: N ~ Poisson(mu^(2 - xi) / (phi (2 - xi))), y the
    sum of N Gamma(shape (2 - xi) / (xi - 1), scale phi (xi - 1) mu^(xi - 1)) draws, 0 at N = 0"""
    N = rng.poisson(mu ** (2.0 - power) / (dispersion * (2.0 - power)))
    y = rng.gamma(np.maximum(N, 1) * ((2.0 - power) / (power - 1.0)), dispersion * (power - 1.0) * mu ** (power - 1.0))
    return np.where(N > 0, y, 0.0)


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------
DATA_DISPERSION = {1.1: 0.8, 1.2: 2.0, 1.5: 0.8, 1.8: 0.5, 1.9: 0.8}      # of the draws: about 40 % zeros at 1.2, 5 % at 1.5, none at 1.8


def data(seed, n, p, intercept, offset, power=1.5, b0=0.3):
    """X ~ U(-0.5, 0.5), beta* as test_gpu_poisson._data, y compound Poisson-Gamma draws around mu at DATA_DISPERSION[power],
    offsets log U(0.5, 2).  At power >= 1.5 zeros are rare, so row 0 is made one: every case has a row with y = 0."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.where(np.arange(p) < max(1, int(0.4 * p)), 0.5, 0.0) / max(1.0, np.sqrt(p / 10))
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    eta = X @ beta + (b0 if intercept else 0.0) + (0.0 if o is None else o)
    y = draw(rng, np.exp(eta), power, DATA_DISPERSION[power])
    if power >= 1.5:
        y[0] = 0.0
    return X, y, o


def away_from_optimum(pe):
    return np.linspace(-0.8, 0.6, pe) / max(1.0, np.sqrt(pe / 10))


def eta_span_case(power):
    """n = 2000, p = 3, intercept and offset, beta_1 = 300 on a column from -1 to 1: eta spans 600"""
    n, p = 2000, 3
    X, y, o = data(20, n, p, True, True, power)
    X[:, 0] = np.linspace(-1.0, 1.0, n)
    return X, y, o, np.array([-0.4, 300.0, 0.3, -0.2])


CALIBRATION = [(1.8, 0.3), (1.2, 2.0)]                 # (power, dispersion) of test_block_is_calibrated
CALIBRATION_TRUTH = np.array([0.3, 0.5, -0.5, 0.25, 0.0, -0.25])


def calibration_case(power, dispersion, K=40, m=1500, seed=2026):
    """K partitions of m rows, 5 features + intercept, offsets log U(0.5, 2), draws at (power, dispersion) around CALIBRATION_TRUTH"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (K * m, 5))
    o = np.log(rng.uniform(0.5, 2.0, K * m))
    y = draw(rng, np.exp(CALIBRATION_TRUTH[0] + X @ CALIBRATION_TRUTH[1:] + o), power, dispersion)
    return X, y, o


def calibration_q(coef, Sig_inv):
    """sum_k (b_k - b*)' Sig_inv_k (b_k - b*): chi-square on K * 6 degrees of freedom when Sig_inv carries the right scale"""
    d = np.asarray(coef) - CALIBRATION_TRUTH
    return float(np.einsum("ki,kij,kj->", d, np.asarray(Sig_inv), d))
