"""numpy reference of the Cox partial likelihood with Efron's approximation for tied event times (log partial likelihood,
score, observed information) and its Newton fit.  Two forms: `efron_loop` is the direct definition (walks the distinct
event times, one max per risk set, loops over l = 0 .. d - 1 and takes S2 - f_l T2 per term; small sizes, the form to
trust), `efron_cumsum` is the vectorised form with per-row weights and at most two rank-one rows per tie group (large sizes).

Group i with d events, risk-set sums S0, S1, S2 and the same sums T0, T1, T2 over the group's event rows only:
    f_l = l / d, phi_l = S0 - f_l T0,
    loglik += sum_events eta - sum_l log phi_l
    U      += sum_events x - sum_l (S1 - f_l T1) / phi_l
    H      += sum_l (S2 - f_l T2) / phi_l - z_l z_l',  z_l = (S1 - f_l T1) / phi_l"""
import numpy as np


def efron_loop(X, time, event, beta):
    X = np.asarray(X, dtype=np.float64)
    p = X.shape[1]
    eta = X @ beta
    ll, U, H = 0.0, np.zeros(p), np.zeros((p, p))
    for t in np.unique(time[event != 0]):
        ev = (time == t) & (event != 0)
        d = int(ev.sum())
        risk = time >= t
        m = eta[risk].max()
        e = np.exp(eta[risk] - m)
        Xr = X[risk]
        S0, S1, S2 = e.sum(), e @ Xr, (Xr * e[:, None]).T @ Xr
        ee = np.exp(eta[ev] - m)
        Xe = X[ev]
        T0, T1, T2 = ee.sum(), ee @ Xe, (Xe * ee[:, None]).T @ Xe
        ll += eta[ev].sum() - d * m
        U += Xe.sum(0)
        for l in range(d):
            f = l / d
            phi = S0 - f * T0
            z = (S1 - f * T1) / phi
            ll -= np.log(phi)
            U -= z
            H += (S2 - f * T2) / phi - np.outer(z, z)
    return ll, U, H


def efron_cumsum(X, time, event, beta, return_rows=False):
    """Rows sorted by descending time; T by per-group sums, S at the end of every tie group by prefix sums of those;
    H = X'diag(w)X - sum_i [S1 T1] K_i [S1 T1]' with w_j = exp(eta_j)(c_j - delta_j h2_g(j)), c the suffix sum of h1 over
    the groups, K_i = [[k0, -k1], [-k1, k2]], k_m = sum_l f_l^m / phi_l^2, taken through its 2 x 2 Cholesky factor as the
    rows L11 S1 + L21 T1 and L22 T1.  return_rows: also the number of such rows (groups with events + groups with d >= 2)."""
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
    starts = np.concatenate([[0], ends[:-1] + 1])
    S0 = np.cumsum(np.add.reduceat(e, starts))
    S1 = np.cumsum(np.add.reduceat(e[:, None] * Xs, starts, axis=0), axis=0)
    d = np.rint(np.add.reduceat(es, starts)).astype(np.int64)
    T0 = np.add.reduceat(e * es, starts)
    T1 = np.add.reduceat((e * es)[:, None] * Xs, starts, axis=0)
    G = len(ends)
    # the (group, l) pairs, flattened
    gi = np.repeat(np.arange(G), d)
    li = np.arange(d.sum()) - np.repeat(np.cumsum(d) - d, d)
    f = li / d[gi]
    phi = S0[gi] - f * T0[gi]

    def per_group(v):
        return np.bincount(gi, weights=v, minlength=G)

    h1, h2 = per_group(1.0 / phi), per_group(f / phi)
    slog = per_group(np.log(phi))
    k0, k1, k2 = per_group(1.0 / phi ** 2), per_group(f / phi ** 2), per_group(f * f / phi ** 2)
    ll = float(es @ eta - d @ np.full(G, m) - slog.sum())
    U = es @ Xs - h1 @ S1 + h2 @ T1
    c = np.cumsum(h1[::-1])[::-1]
    gid = np.cumsum(np.concatenate([[0], end[:-1].astype(int)]))
    w = e * (c[gid] - es * h2[gid])
    has = d > 0
    L11 = np.sqrt(np.where(has, k0, 1.0))
    L21 = -k1 / L11
    L22 = np.sqrt(np.maximum(k2 - L21 ** 2, 0.0))
    R1 = (L11[:, None] * S1 + L21[:, None] * T1)[has]
    R2 = (L22[:, None] * T1)[d > 1]
    H = (Xs * w[:, None]).T @ Xs - R1.T @ R1 - R2.T @ R2
    if return_rows:
        return ll, U, H, int(has.sum() + (d > 1).sum())
    return ll, U, H


def fit(X, time, event, tol=1e-14, max_iter=100, form=efron_cumsum):
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
