"""numpy reference of the Poisson regression map step (log link, optional offset, optional intercept as column 0 of the
design): log-likelihood, score, Fisher information and the per-partition Newton fit with the block it returns."""
import math

import numpy as np


def design(X, intercept):
    X = np.asarray(X, dtype=np.float64)
    return np.concatenate([np.ones((X.shape[0], 1)), X], 1) if intercept else X


def lgamma_const(y):
    return float(sum(math.lgamma(v + 1.0) for v in np.asarray(y, dtype=np.float64)))


def terms(X, y, beta, offset=None, intercept=False):
    """(loglik = sum y eta - mu - lgamma(y + 1), g = D'(y - mu), H = D' diag(mu) D, mu) with D = [1 | X] or X."""
    D = design(X, intercept)
    eta = D @ beta + (0.0 if offset is None else offset)
    with np.errstate(over="ignore", invalid="ignore"):         # (a step that overflows mu is rejected by fit's halving)
        mu = np.exp(eta)
        ll = float(y @ eta - mu.sum()) - lgamma_const(y)
        g = D.T @ (y - mu)
        H = (D * mu[:, None]).T @ D
    return ll, g, H, mu


def fit(X, y, offset=None, intercept=False, tol=1e-14, max_iter=100):
    """Newton from beta = 0 (the intercept at log(sum y / sum e^o)) with step halving; returns (coef, H at coef, loglik)."""
    D = design(X, intercept)
    beta = np.zeros(D.shape[1])
    o = np.zeros(len(y)) if offset is None else offset
    if intercept:
        beta[0] = np.log(y.sum() / np.exp(o).sum())
    ll, g, H, _ = terms(X, y, beta, offset, intercept)
    for _ in range(max_iter):
        step = np.linalg.solve(H, g)
        t = 1.0
        for _ in range(30):
            ll_new, g_new, H_new, _ = terms(X, y, beta + t * step, offset, intercept)
            if np.isfinite(ll_new) and ll_new >= ll - 1e-12 * abs(ll):
                break
            t *= 0.5
        beta = beta + t * step
        ll, g, H = ll_new, g_new, H_new
        if np.max(np.abs(t * step)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
    return beta, H, ll


def block(X, y, offset=None, intercept=False):
    """The DLSA block of one partition: (coef, Sig_inv, Sig_invMcoef)."""
    b, H, _ = fit(X, y, offset, intercept)
    return b, H, H @ b
