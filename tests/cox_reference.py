"""numpy reference of the Cox partial likelihood with Breslow ties (log partial likelihood, score, observed information)
and its Newton fit.  Two forms: `breslow_loop` walks the distinct event times and their risk sets directly (small sizes),
`breslow_cumsum` is the vectorised cumulative-sum form (large sizes)."""
import numpy as np


def breslow_loop(X, time, event, beta):
    X = np.asarray(X, dtype=np.float64)
    eta = X @ beta
    ll, U, H = 0.0, np.zeros(X.shape[1]), np.zeros((X.shape[1], X.shape[1]))
    for t in np.unique(time[event != 0]):
        ev = (time == t) & (event != 0)
        d = float(ev.sum())
        risk = time >= t
        e = np.exp(eta[risk] - eta[risk].max())
        S0 = e.sum()
        S1 = e @ X[risk]
        S2 = (X[risk] * e[:, None]).T @ X[risk]
        a = S1 / S0
        ll += eta[ev].sum() - d * (eta[risk].max() + np.log(S0))
        U += X[ev].sum(0) - d * a
        H += d * (S2 / S0 - np.outer(a, a))
    return ll, U, H


def breslow_cumsum(X, time, event, beta):
    """Rows sorted by descending time; the risk-set sums are prefix sums taken at the end of every tie group, the
    information is X'diag(w)X - A'diag(d)A with w_j = exp(eta_j) * (cumulative hazard at t_j)."""
    X = np.asarray(X, dtype=np.float64)
    o = np.argsort(-time, kind="stable")
    Xs, ts, es = X[o], time[o], (event[o] != 0).astype(np.float64)
    eta = Xs @ beta
    m = eta.max()
    e = np.exp(eta - m)
    n = len(ts)
    end = np.ones(n, dtype=bool)
    end[:-1] = ts[1:] != ts[:-1]
    ends = np.nonzero(end)[0]
    S0 = np.cumsum(e)[ends]
    S1 = np.cumsum(e[:, None] * Xs, axis=0)[ends]
    ev_cum = np.concatenate([[0.0], np.cumsum(es)])
    starts = np.concatenate([[0], ends[:-1] + 1])
    d = ev_cum[ends + 1] - ev_cum[starts]
    A = S1 / S0[:, None]
    ll = float(es @ eta - d @ (m + np.log(S0)))
    U = es @ Xs - d @ A
    hz = d / S0                                   # exp(-m) scaled hazard increments
    c = np.cumsum(hz[::-1])[::-1]                 # suffix over groups
    gid = np.cumsum(np.concatenate([[0], end[:-1].astype(int)]))
    w = e * c[gid]
    H = (Xs * w[:, None]).T @ Xs - (A * d[:, None]).T @ A
    return ll, U, H


def fit(X, time, event, tol=1e-14, max_iter=100, form=breslow_cumsum):
    p = X.shape[1]
    beta = np.zeros(p)
    for _ in range(max_iter):
        ll, U, H = form(X, time, event, beta)
        step = np.linalg.solve(H, U)
        beta = beta + step
        if np.max(np.abs(step)) <= tol * max(1.0, np.max(np.abs(beta))):
            break
    ll, U, H = form(X, time, event, beta)
    return beta, H, ll
