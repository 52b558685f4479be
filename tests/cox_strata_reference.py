"""numpy reference of the stratified Cox partial likelihood: one common beta, one baseline hazard per stratum, so the log
partial likelihood, the score and the observed information are the sums over the strata of the unstratified quantities on
each stratum's rows.  `stratified` applies any form of tests/cox_reference.py or tests/cox_efron_reference.py stratum by
stratum; `fit` is Newton on that sum.  `clogit_pairs` is the closed form of conditional logistic regression on 1:1 matched
pairs, an oracle that shares no code with the Cox references."""
import numpy as np

from cox_efron_reference import efron_cumsum


def stratified(form, X, time, event, strata, beta):
    X = np.asarray(X, dtype=np.float64)
    p = X.shape[1]
    ll, U, H = 0.0, np.zeros(p), np.zeros((p, p))
    for s in np.unique(strata):
        m = strata == s
        if not np.any(event[m] != 0):           # a stratum without events contributes nothing
            continue
        l, u, h = form(X[m], time[m], event[m], beta)
        ll += l
        U += u
        H += h
    return ll, U, H


def fit(X, time, event, strata, tol=1e-14, max_iter=100, form=efron_cumsum):
    p = X.shape[1]
    beta = np.zeros(p)
    for _ in range(max_iter):
        ll, U, H = stratified(form, X, time, event, strata, beta)
        step = np.linalg.solve(H, U)
        beta = beta + step
        if np.max(np.abs(step)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
    ll, U, H = stratified(form, X, time, event, strata, beta)
    return beta, H, ll


def pair_deltas(X, event, strata):
    """x_case - x_control of every stratum, which must hold exactly one event row and one other row"""
    o = np.lexsort((-(event != 0).astype(np.int64), strata))       # by stratum, the case first
    assert len(o) % 2 == 0 and np.all(strata[o[0::2]] == strata[o[1::2]])
    assert np.all(event[o[0::2]] != 0) and np.all(event[o[1::2]] == 0)
    assert len(np.unique(strata)) == len(o) // 2
    return np.asarray(X, dtype=np.float64)[o[0::2]] - np.asarray(X, dtype=np.float64)[o[1::2]]


def clogit_pairs(X, event, strata, beta):
    """1:1 matched pairs, Delta = x_case - x_control, sigma = 1 / (1 + exp(-Delta beta)):
    loglik = -sum log(1 + exp(-Delta beta)), U = sum (1 - sigma) Delta, H = sum sigma (1 - sigma) Delta Delta'"""
    D = pair_deltas(X, event, strata)
    z = D @ beta
    ll = -float(np.sum(np.logaddexp(0.0, -z)))
    sig = 1.0 / (1.0 + np.exp(-z))
    U = (1.0 - sig) @ D
    H = (D * (sig * (1.0 - sig))[:, None]).T @ D
    return ll, U, H


def clogit_pairs_fit(X, event, strata, tol=1e-14, max_iter=100):
    p = X.shape[1]
    beta = np.zeros(p)
    for _ in range(max_iter):
        ll, U, H = clogit_pairs(X, event, strata, beta)
        step = np.linalg.solve(H, U)
        beta = beta + step
        if np.max(np.abs(step)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
    ll, U, H = clogit_pairs(X, event, strata, beta)
    return beta, H, ll
