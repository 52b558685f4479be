"""The inputs of the strata tests, shared by the CPU checks (tests/test_cox_strata_cpu.py) and the GPU tests
(tests/test_gpu_cox_strata.py), so that the condition "stratified and unstratified differ on these inputs" is checked on the
very arrays the kernels are run on.  Built on the generator of the Efron tests (tests/cox_efron_cases.py)."""
import numpy as np

import cox_efron_cases as ec

PASS_P = [1, 5, 50, 130, 520]          # one lane pair; odd p (scalar loads); two column chunks; five (one row per step)
PASS_N = [7, 300, 5000]
LAYOUTS = ["random7", "blocks64", "mixed", "pairs"]
EDGE_CASES = ["empty_strata", "all_tied", "boundary_ties", "eta_range", "single_row"]

# uneven shares; a negative code, a large one, and codes whose order is not that of their first appearance
CODES7 = np.array([-3, 0, 5, 17, 1000, 2_000_000_000, 42], dtype=np.int64)
SHARE7 = np.array([0.30, 0.05, 0.20, 0.02, 0.25, 0.10, 0.08])


def sort_order(t, strata, offs=None):
    """the permutation the kernels read: every partition's rows grouped by stratum (ascending code), descending time inside"""
    offs = [0, len(t)] if offs is None else offs
    parts = []
    for k in range(len(offs) - 1):
        sl = slice(offs[k], offs[k + 1])
        o = np.argsort(-t[sl], kind="stable")
        if strata is not None:
            o = o[np.argsort(strata[sl][o], kind="stable")]
        parts.append(offs[k] + o)
    return np.concatenate(parts).astype(np.int64)


def layout(name, n, seed):
    rng = np.random.default_rng(seed)
    if name == "random7":
        return CODES7[rng.choice(7, size=n, p=SHARE7)]
    if name == "blocks64":             # sorted by code, every stratum fills 64 positions: every boundary is a segment boundary
        return (np.arange(n) // 64)[rng.permutation(n)].astype(np.int64)
    if name == "pairs":                # (an odd n leaves a stratum of one row)
        return (np.arange(n) // 2)[rng.permutation(n)].astype(np.int64)
    if name == "mixed":                # one row; three of two rows; one of 220 rows (more than three segments); the rest random
        sizes = [1, 2, 2, 2] + ([220] if n >= 300 else [])
        codes = np.concatenate([np.full(sz, 10 + i) for i, sz in enumerate(sizes)])[:n]
        rest = n - len(codes)
        codes = np.concatenate([codes, 100 + rng.integers(0, 3, rest)])
        return codes[rng.permutation(n)].astype(np.int64)
    raise KeyError(name)


def pass_case(p, n, name):
    """the tied rows of the Efron pass test (20 time levels, so that equal times meet across stratum boundaries) and a layout"""
    X, t, ev, beta = ec.pass_case(p, n)
    return X, t, ev, beta, layout(name, n, 300 + p + n)


def edge_case(case):
    n, p = 2000, 6
    X, t, ev = ec.data(330, n, p, ties=20)
    beta = np.linspace(-0.5, 0.5, p)
    rng = np.random.default_rng(331)
    strata = rng.integers(0, 5, n)
    if case == "empty_strata":         # no event in the first, a middle and the last stratum of the order
        ev[(strata == 0) | (strata == 2) | (strata == 4)] = 0.0
    elif case == "all_tied":           # every stratum one tie group (d in the hundreds over several segments, boundaries inside segments)
        t = 1.0 + strata.astype(np.float64)
    elif case == "boundary_ties":      # two levels per stratum; the lower one of stratum s is the upper one of stratum s + 1
        t = 10.0 - strata + rng.integers(0, 2, n)
        ev[:] = 1.0
        ev[rng.random(n) < 0.2] = 0.0
    elif case == "eta_range":
        X, t, ev, beta = ec.edge_case("eta_range")
        strata = rng.integers(0, 5, len(t))
    elif case == "single_row":
        X, t, ev, strata = X[:1], t[:1], np.ones(1), strata[:1]
    else:
        raise KeyError(case)
    return X, t, ev, beta, strata.astype(np.int64)


def long_case():
    """n = 300 000: segments of 76 positions (no multiple of 64), 1000 random strata"""
    n, p = 300_000, 3
    X, t, ev = ec.data(340, n, p, ties=2000)
    strata = np.random.default_rng(341).integers(0, 1000, n)
    return X, t, ev, np.array([0.4, -0.3, 0.2]), strata


def pairs_case(sets=2000, p=4):
    """1:1 matched pairs: the case has the event; in half of the pairs the control leaves later, in the others at the same time"""
    rng = np.random.default_rng(350)
    n = 2 * sets
    X = rng.uniform(-1.0, 1.0, (n, p))
    strata = np.repeat(np.arange(sets), 2)
    ev = np.tile([1.0, 0.0], sets)
    t = np.tile([1.0, 2.0], sets)
    t[1::4] = 1.0
    # the case of a pair is the likelier one under beta* = (1, -1, 0.5, 0): swap the rows of a pair accordingly
    D = X[0::2] - X[1::2]
    bstar = np.array([1.0, -1.0, 0.5, 0.0])[:p]
    swap = rng.random(sets) > 1.0 / (1.0 + np.exp(-D @ bstar))
    idx = np.arange(n).reshape(sets, 2)
    idx[swap] = idx[swap][:, ::-1]
    X = X[idx.ravel()]
    perm = rng.permutation(n)
    return X[perm], t[perm], ev[perm], np.linspace(-0.3, 0.3, p), strata[perm]


def fit_case(p, n=20_000, S=5):
    """50 tie levels, 5 strata whose time scale depends on the stratum (so that pooling the strata is another model)"""
    X, t, ev = ec.data(360 + p, n, p, ties=50)
    strata = np.random.default_rng(361 + p).integers(0, S, n)
    return X, t * 4.0 ** strata, ev, strata
