"""The tied inputs of the Efron tests, shared by the CPU checks of the reference (tests/test_cox_efron_cpu.py) and the GPU tests
(tests/test_gpu_cox_efron.py), so that the condition "Efron and Breslow differ on these inputs" is checked on the very
arrays the kernels are run on.  The generator is that of tests/test_gpu_cox.py."""
import numpy as np

PASS_P = [1, 5, 50, 100, 130, 500]
PASS_N = [1, 7, 300, 5000]
EDGE_CASES = ["all_tied", "no_censoring", "single_event", "pairs", "eta_range"]


def data(seed, n, p, ties=None, censor=0.3, scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p)) * scale
    beta = np.where(np.arange(p) < max(1, int(0.4 * p)), 1.0, 0.0)
    t = rng.exponential(1.0, n) / np.exp(X @ beta / max(1.0, scale))
    if ties:
        # the quantile levels by hand (np.quantile takes a minute for 90 000 of them)
        s, pos = np.sort(t), np.linspace(0, 1, ties + 1)[1:] * (n - 1)
        lo = np.floor(pos).astype(np.int64)
        q = s[lo] + (s[np.minimum(lo + 1, n - 1)] - s[lo]) * (pos - lo)
        t = q[np.minimum(np.searchsorted(q, t), ties - 1)]
    ev = (rng.random(n) >= censor).astype(np.float64)
    return X, t, ev


def pass_case(p, n):
    """20 quantile levels (at n = 300 groups of ~15 rows cross the 64-row segments); 7 rows cannot tie on 20 levels, so they
    get 2 levels and no censoring; a single row has nothing to tie with."""
    X, t, ev = data(110 + p + n, n, p, ties=20 if n > 20 else 2, censor=0.3 if n > 20 else 0.0)
    ev[0] = 1.0
    return X, t, ev, np.linspace(-0.5, 0.5, p)


def edge_case(case):
    n, p = 2000, 6
    X, t, ev = data(130, n, p)
    beta = np.linspace(-0.5, 0.5, p)
    if case == "all_tied":                 # one group over all 32 segments, d ~ 1400
        t[:] = 1.0
    elif case == "no_censoring":
        X, t, ev = data(130, n, p, ties=7, censor=0.0)
    elif case == "single_event":
        ev[:] = 0.0
        ev[n // 2] = 1.0
    elif case == "pairs":                  # every time shared by exactly two rows
        t = np.repeat(np.sort(t[: n // 2]), 2)[np.random.default_rng(132).permutation(n)]
    elif case == "eta_range":
        # eta spans more than 700 (exp overflows): a binary column with coefficient 800, as in tests/test_gpu_cox.py
        X, t, ev = data(130, n, p, ties=20)
        X[:, 0] = (np.random.default_rng(131).random(n) < 0.3).astype(np.float64)
        beta[0] = 800.0
        assert np.ptp(X @ beta) > 700
    else:
        raise KeyError(case)
    return X, t, ev, beta
