"""What the CPU and the GPU tests of the structured one-hot ordinal map step (csrc/onehot_ordinal.hip) share, importable without a
GPU: the designs (test_gpu_onehot._random_design without a constant column, with Zipf or uniform level frequencies), the pass and
fit cases, the structured extreme case, the reference fit with its halvings counted, and a Python statement of the LDS route rule.
The reference is tests/ordinal_reference.py on the dense matrix oracle.dlsa_oracle.design_matrix builds."""
import functools

import numpy as np

import ordinal_reference as orf
from test_gpu_onehot import _random_design
from test_gpu_onehot_poisson import SHAPES

TOL_PASS = 1e-12
TOL_FIT = 1e-10
CLASSES = (2, 3, 5, 8)
LDS_BUDGET = 32 * 1024


def lds_route(p, C):
    """(borders in the pass?, histogram copies with H, histogram copies without H) -- the rule of csrc/onehot_ordinal.hip
    (oh_ord_border, oh_ord_rep): the borders are taken in the pass where (p + J + C p) doubles fit 32 KiB; the copies are the
    largest of 8, 4, 2, 1 that keeps (p + J + copies * cells) doubles within 32 KiB, cells = C p with the borders and p without."""
    J = C - 1
    border = (p + J + C * p) * 8 <= LDS_BUDGET

    def rep(cells):
        r = 8
        while r > 1 and (p + J + r * cells) * 8 > LDS_BUDGET:
            r //= 2
        return r
    return border, rep(C * p if border else p), rep(p)


def shape_p(q, nlevels, baseline):
    """columns of a design without a constant column: q numerics + the levels (less one per factor when baselines are dropped)"""
    return q + sum(nlevels) - (len(nlevels) if baseline else 0)


# (n, q, nlevels, C, baseline dropped?) with J + p <= 2048
PASS_CASES = [(n, q, nl, C, b) for (n, q, nl) in SHAPES for C in CLASSES for b in (True, False) if C - 1 + shape_p(q, nl, b) <= 2048]


def design(rng, n, q, nlevels, baseline=True, freq=None):
    """_random_design without a constant column; freq: None (its uniform draw), "zipf" (1 / rank) or "uniform" (redrawn)"""
    p, num, codes, desc, nl, level_col = _random_design(rng, n, q, nlevels, intercept=False, baseline=baseline)
    if freq is not None:
        for t, L in enumerate(nlevels):
            w = 1.0 / np.arange(1, L + 1) if freq == "zipf" else np.ones(L)
            codes[:, t] = rng.choice(L, n, p=w / w.sum())
    return p, num, codes, desc, nl, level_col


def cutpoints(C):
    share = np.arange(1, C) / C
    return np.log(share / (1 - share))


def pass_theta(rng, p, C):
    """strictly increasing cutpoints around the equal-share ones, beta ~ 0.4 N(0, 1): away from any optimum"""
    return np.concatenate([cutpoints(C) + np.linspace(-0.2, 0.3, C - 1), rng.normal(size=p) * 0.4])


def fit_case(design_matrix, n, q, nlevels, seed, C, freq="zipf", baseline=True):
    """rows drawn from the model at beta ~ 0.3 N(0, 1) and the equal-share cutpoints; design_matrix = oracle.dlsa_oracle.design_matrix"""
    rng = np.random.default_rng(seed)
    p, num, codes, desc, nl, level_col = design(rng, n, q, nlevels, baseline, freq)
    X, _ = design_matrix(num, codes, *desc)
    theta = np.concatenate([cutpoints(C), rng.normal(size=p) * 0.3])
    y = orf.draw(rng, X, theta, C)
    return p, num, codes, desc, nl, level_col, X, y


def parts(n, K, strided):
    """(the partitions' row slices, part_first, part_rows, row_step)"""
    if strided:
        return [slice(k, n, K) for k in range(K)], list(range(K)), [len(range(k, n, K)) for k in range(K)], K
    sl = [slice(k * n // K, (k + 1) * n // K) for k in range(K)]
    return sl, [s.start for s in sl], [s.stop - s.start for s in sl], 1


# (n, q, nlevels, C, K, strided, seed, freq): the four in-pass fits and the one on the masked border route (p = 500 at C = 8)
FIT_CASES = [(6000, 2, (5, 4), 3, 2, True, 1, "zipf"), (24000, 2, (40, 5), 4, 6, True, 24002, "zipf"),
             (12000, 3, (7, 4, 12), 8, 3, False, 41, "zipf"), (40000, 3, (110, 110, 20, 6), 3, 4, False, 40008, "zipf")]
MASKED_FIT_CASE = (20000, 1, (500,), 8, 1, False, 7, "uniform")


def fit_counted(X, y, C, tol=1e-13, max_iter=100):
    """orf.fit's loop with the halvings counted: (coef, H at coef, loglik, evaluations, halvings)"""
    theta = orf.start(y, X.shape[1], C)
    prev, ll_prev, halvings, total, n_iter = None, None, 0, 0, 0
    for it in range(max_iter + 1):
        ll, g, H, _ = orf.terms(X, y, theta, C)
        worse = (not np.isfinite(ll)) or (ll_prev is not None and ll < ll_prev - 1e-12 * abs(ll_prev))
        if ll_prev is not None and worse and halvings < 30:
            halvings += 1
            total += 1
            theta = prev + (theta - prev) / 2
            continue
        halvings, n_iter = 0, it + 1
        delta = np.linalg.solve(H, g)
        if np.max(np.abs(delta)) <= tol * max(1.0, np.max(np.abs(theta))):
            break
        prev, ll_prev, theta = theta, ll, theta + delta
    return theta, H, ll, n_iter, total


@functools.lru_cache(maxsize=None)
def fit_reference(case):
    """the case's rows and, per partition, fit_counted on the dense matrix: computed once, shared by the tests, never changed"""
    from oracle import dlsa_oracle
    n, q, nlevels, C, K, strided, seed, freq = case
    data = fit_case(dlsa_oracle.design_matrix, n, q, nlevels, seed, C, freq)
    X, y = data[6], data[7]
    sl = parts(n, K, strided)[0]
    return data, [fit_counted(X[s], y[s], C) for s in sl]


EXTREME_CLASSES = 5


def extreme_case():
    """n = 2000, C = 5: one numeric running -1 .. 1 (shift 0, scale 1) with the coefficient 400, one 3-level factor with its
    baseline dropped (coefficients 0.3, -0.2), the cutpoints -200, -50, -50 + 1e-6, 150; responses as orf.extreme_case (the likely
    class of the row, every tenth row the class (i / 10) % 5).  Returns (p, num, codes, desc, nl, level_col, y, theta)."""
    n, C = 2000, EXTREME_CLASSES
    rng = np.random.default_rng(20)
    arr = lambda v, t: np.asarray(v, dtype=t)
    desc = (arr([1, 2, 2], np.int32), arr([0, 0, 0], np.int32), arr([0, 1, 2], np.int32), arr([0.0] * 3, np.float64), arr([1.0] * 3, np.float64))
    nl, level_col, p = [3], [-1, 1, 2], 3
    num = np.linspace(-1.0, 1.0, n)[:, None].copy()
    codes = rng.integers(0, 3, (n, 1)).astype(np.int32)
    theta = np.array([-200.0, -50.0, -50.0 + 1e-6, 150.0, 400.0, 0.3, -0.2])
    eta = 400.0 * num[:, 0] + np.where(codes[:, 0] == 1, 0.3, 0.0) + np.where(codes[:, 0] == 2, -0.2, 0.0)
    y = (eta[:, None] > theta[None, :4]).sum(1).astype(np.float64)
    y[::10] = (np.arange(0, n, 10) // 10) % C
    return p, num, codes, desc, nl, level_col, y, theta
