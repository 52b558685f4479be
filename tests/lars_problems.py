"""Seeded LSA problems for the wide LARS tests (numpy only, so that an oracle run can be regenerated in a worker process from its
spec instead of shipping a 30 MB Sigma): problem(spec) -> (Sigma, b, n) and oracle_path(spec) -> the oracle's path as numpy.

spec = (kind, p, rho, seed):
  corr      tests/test_gpu_kernels.py's _correlated_lsa_problem: a three-factor design, correlation rho between columns
  zerocol   a few all-zero columns (an absent dummy level)
  ties      Sigma = 3 I (one off-diagonal pair) and |b| in groups of four: exactly tied |Cvec|, several variables enter in one step
  tinyb     30% of b scaled by 1e-12
  pairs     a few column pairs at correlation 0.99995 (a small but honest pivot)
  rankdef   n = p / 2 rows: a rank-deficient Sigma.  Only the path before the active set reaches the rank is well defined: beyond
            it the next pivot r_pp^2 is rounding noise above eps, and the reference itself (the oracle included) runs off to
            |beta| ~ 1e20 .. inf, differently in every implementation -- so these are run with max_steps = n / 2
"""
import numpy as np


def problem(spec):
    kind, p, rho, seed = spec
    rng = np.random.default_rng(seed)
    if kind == "corr":
        n = 6 * p
        L = rng.standard_normal((3, p))
        X = np.sqrt(1 - rho) * rng.standard_normal((n, p)) + np.sqrt(rho) * (rng.standard_normal((n, 3)) @ L)
        S = X.T @ ((rng.random(n) * 0.25)[:, None] * X)
        return S, rng.standard_normal(p), n
    if kind == "ties":
        S = np.eye(p) * 3.0
        S[0, 1] = S[1, 0] = 0.5
        b = np.sign(rng.standard_normal(p)) * np.repeat(rng.random(p // 4 + 1) + 0.5, 4)[:p]
        return S, b, 4 * p
    n = p // 2 if kind == "rankdef" else 4 * p
    X = rng.standard_normal((n, p))
    if kind == "zerocol":
        X[:, rng.choice(p, 3, replace=False)] = 0.0
    if kind == "pairs":
        for _ in range(4):
            a, c = rng.choice(p, 2, replace=False)
            X[:, c] = X[:, a] + 1e-2 * rng.standard_normal(n)
    S = X.T @ ((rng.random(n) * 0.25 + 0.01)[:, None] * X)
    b = rng.standard_normal(p)
    if kind == "tinyb":
        b[rng.random(p) < 0.3] *= 1e-12
    return S, b, n


def oracle_path(job):
    """(spec, intercept, type, max_steps) -> the oracle's {'beta', 'beta0', 'AIC', 'BIC'} (runs in a worker process)"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import dlsa_oracle as orc
    spec, intercept, typ, max_steps = job
    S, b, n = problem(spec)
    return orc.lars_lsa(S, b, intercept, n, type=typ, max_steps=max_steps)
