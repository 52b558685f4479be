"""numpy / scipy reference of the negative-binomial (NB2) regression map step (log link, optional offset, optional intercept as
column 0 of the design, Var y = mu + alpha mu^2, theta = 1 / alpha): log-likelihood, score, Fisher information and the dispersion
terms at a fixed (beta, alpha); the alternating per-partition fit; a second, independent route to the same MLE (a root of the
profile score with beta refitted at every theta); and the block a partition returns."""
import numpy as np
from scipy import optimize, special

import poisson_reference as pr

design = pr.design


def data(seed, n, p, intercept, offset, alpha, b0=0.3, scale=1.0):
    """The rows of the Poisson tests (uniform features, 0.5 on the first 40 % of the coefficients, scaled down with the width) with
    gamma-mixed counts: y ~ Poisson(mu G), G ~ Gamma(1 / alpha, alpha), i.e. y ~ NB2(mu, alpha).  Returns (X, y, offset or None)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.where(np.arange(p) < max(1, int(0.4 * p)), 0.5, 0.0) * scale / max(1.0, np.sqrt(p / 10))
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    eta = X @ beta + (b0 if intercept else 0.0) + (0.0 if o is None else o)
    y = rng.poisson(np.exp(eta) * rng.gamma(1.0 / alpha, alpha, n)).astype(np.float64)
    return X, y, o


def theta_terms(y, mu, alpha):
    """(s = d loglik / d theta, i = -d2 loglik / d theta2, pearson) of the rows (y, mu): the textbook forms."""
    th = 1.0 / alpha
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = float(np.sum(special.digamma(y + th) - special.digamma(th) + np.log(th) + 1.0 - np.log(th + mu) - (y + th) / (mu + th)))
        i = float(np.sum(-special.polygamma(1, y + th) + special.polygamma(1, th) - 1.0 / th + 2.0 / (mu + th)
                         - (y + th) / (mu + th) ** 2))
        pearson = float(np.sum((y - mu) ** 2 / (mu + alpha * mu * mu)))
    return s, i, pearson


def loglik(y, eta, mu, alpha):
    """the textbook NB2 log-likelihood of the rows"""
    th = 1.0 / alpha
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return float(np.sum(special.gammaln(y + th) - special.gammaln(th) - special.gammaln(y + 1.0) + th * np.log(th)
                            + y * eta - (th + y) * np.log(th + mu)))


def terms(X, y, beta, alpha, offset=None, intercept=False):
    """(loglik, g = D'[(y - mu) / (1 + alpha mu)], H = D' diag(mu / (1 + alpha mu)) D, mu, s, i, pearson) with D = [1 | X] or X."""
    D = design(X, intercept)
    y = np.asarray(y, dtype=np.float64)
    eta = D @ beta + (0.0 if offset is None else offset)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):     # (a step that overflows mu is rejected by the halving)
        mu = np.exp(eta)
        ll = loglik(y, eta, mu, alpha)
        q = 1.0 / (1.0 + alpha * mu)
        g = D.T @ ((y - mu) * q)
        H = (D * (mu * q)[:, None]).T @ D
    return (ll, g, H, mu) + theta_terms(y, mu, alpha)


def fit_beta(X, y, beta, alpha, offset=None, intercept=False, tol=1e-14, max_iter=200):
    """Fisher scoring on beta at a fixed alpha from `beta`, with step halving; returns (beta, number of steps taken)."""
    beta = np.array(beta, dtype=np.float64)
    ll, g, H = terms(X, y, beta, alpha, offset, intercept)[:3]
    steps = 0
    for _ in range(max_iter):
        step = np.linalg.solve(H, g)
        if np.max(np.abs(step)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
        t = 1.0
        for _ in range(30):
            ll_new, g_new, H_new = terms(X, y, beta + t * step, alpha, offset, intercept)[:3]
            if np.isfinite(ll_new) and ll_new >= ll - 1e-12 * abs(ll):
                break
            t *= 0.5
        beta = beta + t * step
        ll, g, H = ll_new, g_new, H_new
        steps += 1
    return beta, steps


def solve_theta(y, mu, alpha, tol=1e-12):
    """Newton on log theta for the rows (y, mu): step s / (i theta), clamped to [-1, 1]; returns alpha (unchanged where the first
    step is already within tol)."""
    prev = np.inf
    for _ in range(60):
        s, i, _ = theta_terms(y, mu, alpha)
        step = s * alpha / i if i > 0 else np.sign(s)
        step = float(np.clip(step, -1.0, 1.0))
        if abs(step) <= tol or (abs(step) <= 1e-8 and abs(step) >= 0.5 * prev):
            break
        prev = abs(step)
        alpha = alpha * np.exp(-step)
    return alpha


def fit(X, y, offset=None, intercept=False, alpha=None, tol=1e-14, max_iter=200):
    """The alternating fit: Poisson start; alpha given: Fisher scoring on beta at that alpha; sum (y - mu)^2 - y <= 0 at the Poisson
    MLE: the MLE is alpha = 0 and the Poisson fit is the answer; otherwise, from the moment start, theta is solved for the current mu
    before every step of beta, until beta's step vanishes and theta stays.  Returns (coef, H at (coef, alpha), loglik, alpha,
    alpha_info = i theta^2, pearson)."""
    y = np.asarray(y, dtype=np.float64)
    b, Hp, llp = pr.fit(X, y, offset, intercept)
    mu = pr.terms(X, y, b, offset, intercept)[3]
    if alpha is not None:
        a = float(alpha)
        b, _ = fit_beta(X, y, b, a, offset, intercept, tol)
    else:
        if np.sum((y - mu) ** 2 - y) <= 0.0:
            return b, Hp, llp, 0.0, 0.0, float(np.sum((y - mu) ** 2 / mu))
        a = solve_theta(y, mu, max(float(np.sum((y - mu) ** 2 - mu) / np.sum(mu * mu)), 1e-3))
        D = design(X, intercept)
        o = 0.0 if offset is None else offset
        _, g, H, mu = terms(X, y, b, a, offset, intercept)[:4]
        for _ in range(max_iter):
            step = np.linalg.solve(H, g)
            a_new = solve_theta(y, mu, a)
            if np.max(np.abs(step)) <= tol * max(1.0, np.max(np.abs(b))) and a_new == a:
                break
            a = a_new
            ll = loglik(y, D @ b + o, mu, a)
            t = 1.0
            for _ in range(30):
                ll_new, g_new, H_new, mu_new = terms(X, y, b + t * step, a, offset, intercept)[:4]
                if np.isfinite(ll_new) and ll_new >= ll - 1e-12 * abs(ll):
                    break
                t *= 0.5
            b = b + t * step
            g, H, mu = g_new, H_new, mu_new
    ll, _, H, _, _, i, pearson = terms(X, y, b, a, offset, intercept)
    return b, H, ll, a, i / (a * a), pearson


def fit_profile(X, y, offset=None, intercept=False, tol=1e-14):
    """The same MLE by another route: brentq on the profile score in log theta, beta refitted to convergence at every theta
    (from the Poisson fit each time, so no state is carried from one theta to the next).  Needs an overdispersed sample."""
    y = np.asarray(y, dtype=np.float64)
    b0 = pr.fit(X, y, offset, intercept)[0]
    mu = pr.terms(X, y, b0, offset, intercept)[3]
    a0 = max(float(np.sum((y - mu) ** 2 - mu) / np.sum(mu * mu)), 1e-3)

    def score(t):
        a = float(np.exp(-t))
        b, _ = fit_beta(X, y, b0, a, offset, intercept, tol)
        return terms(X, y, b, a, offset, intercept)[4] * np.exp(t)

    lo = hi = -np.log(a0)
    while score(lo) < 0.0:
        lo -= 1.0
    while score(hi) > 0.0:
        hi += 1.0
    t = optimize.brentq(score, lo, hi, xtol=1e-15, rtol=8.9e-16, maxiter=200)
    a = float(np.exp(-t))
    b, _ = fit_beta(X, y, b0, a, offset, intercept, tol)
    ll, _, H, _, _, i, pearson = terms(X, y, b, a, offset, intercept)
    return b, H, ll, a, i / (a * a), pearson


def block(X, y, offset=None, intercept=False, alpha=None):
    """The DLSA block of one partition: (coef, Sig_inv, Sig_invMcoef)."""
    b, H = fit(X, y, offset, intercept, alpha)[:2]
    return b, H, H @ b
