"""numpy reference of the Gamma regression map step (log link, optional offset, optional intercept as column 0 of the design):
the full log-likelihood at a dispersion, score, observed information, the Pearson and deviance sums, and the per-partition Newton
fit with the block it returns.  With r = y / mu and nu = 1 / dispersion:
    loglik = nu sum(-r - eta) + n (nu log nu - lgamma nu) + (nu - 1) sum log y,  g = nu D'(r - 1),  H = nu D' diag(r) D,
    P = sum (r - 1)^2,  Dev = 2 sum (r - 1 - log r),  estimated dispersion = P / (n - pe)."""
import math

import numpy as np


def design(X, intercept):
    X = np.asarray(X, dtype=np.float64)
    return np.concatenate([np.ones((X.shape[0], 1)), X], 1) if intercept else X


def ll_const(y, dispersion):
    """the beta-free part of the log-likelihood: n (nu log nu - lgamma nu) + (nu - 1) sum log y"""
    nu = 1.0 / dispersion
    return len(y) * (nu * math.log(nu) - math.lgamma(nu)) + (nu - 1.0) * float(np.log(y).sum())


def terms(X, y, beta, offset=None, intercept=False, dispersion=1.0):
    """(loglik, g, H, r, P, Dev) at beta and the given dispersion, with D = [1 | X] or X."""
    D = design(X, intercept)
    eta = D @ beta + (0.0 if offset is None else offset)
    nu = 1.0 / dispersion
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):      # (a step that underflows mu is rejected by fit's halving)
        r = y / np.exp(eta)
        ll = nu * float(-(r + eta).sum()) + ll_const(y, dispersion)
        g = nu * (D.T @ (r - 1.0))
        H = nu * ((D * r[:, None]).T @ D)
        P = float(((r - 1.0) ** 2).sum())
        dev = 2.0 * float((r - 1.0 - np.log(r)).sum())
    return ll, g, H, r, P, dev


def start(X, y, offset=None, intercept=False):
    """beta = 0, the intercept at log(mean(y e^-o)): the exact MLE of the intercept-only model"""
    beta = np.zeros(np.asarray(X).shape[1] + (1 if intercept else 0))
    if intercept:
        beta[0] = np.log(np.mean(y * np.exp(-(0.0 if offset is None else offset))))
    return beta


def fit(X, y, offset=None, intercept=False, dispersion=None, tol=1e-14, max_iter=100):
    """Newton from start() with step halving, at unit dispersion (beta does not depend on it); then the dispersion (the given one,
    or Pearson's P / (n - pe)) scales the information.  Returns (coef, Sig_inv = H / dispersion at coef, loglik at (coef, that
    dispersion), the dispersion, P, Dev)."""
    beta = start(X, y, offset, intercept)
    ll, g, H = terms(X, y, beta, offset, intercept)[:3]
    for _ in range(max_iter):
        step = np.linalg.solve(H, g)
        t = 1.0
        for _ in range(30):
            ll_new, g_new, H_new = terms(X, y, beta + t * step, offset, intercept)[:3]
            if np.isfinite(ll_new) and ll_new >= ll - 1e-12 * abs(ll):
                break
            t *= 0.5
        beta = beta + t * step
        ll, g, H = ll_new, g_new, H_new
        if np.max(np.abs(t * step)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
    _, _, H, _, P, dev = terms(X, y, beta, offset, intercept)
    phi = P / (len(y) - len(beta)) if dispersion is None else float(dispersion)
    return beta, H / phi, terms(X, y, beta, offset, intercept, phi)[0], phi, P, dev


def block(X, y, offset=None, intercept=False, dispersion=None):
    """The DLSA block of one partition: (coef, Sig_inv, Sig_invMcoef)."""
    b, S = fit(X, y, offset, intercept, dispersion)[:2]
    return b, S, S @ b
