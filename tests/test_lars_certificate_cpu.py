"""CPU: the oracle-free LARS / lasso path certificate (tests/lars_certificate.py) accepts the reference's paths -- the F3 / F3i
goldens and seeded problems with correlation, ties, zero columns and tiny coefficients -- and rejects small mutations of a valid
path at the tolerance the GPU tests use."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from golden_inputs import lars_case
import lars_certificate as lc
from oracle import dlsa_oracle as orc


def _problem(p, rho, seed, kind="plain"):
    rng = np.random.default_rng(seed)
    n = 6 * p + 4
    L = rng.standard_normal((3, p))
    X = np.sqrt(1 - rho) * rng.standard_normal((n, p)) + np.sqrt(rho) * (rng.standard_normal((n, 3)) @ L)
    if kind == "zerocol":                                  # an absent dummy level
        X[:, rng.integers(0, p, 2)] = 0.0
    S = X.T @ ((rng.random(n) * 0.25 + 0.01)[:, None] * X)
    b = rng.standard_normal(p)
    if kind == "ties":                                     # groups of exactly tied |Cvec|: several variables enter in one step
        S = np.eye(p) * 3.0
        S[0, 1] = S[1, 0] = 0.5
        b = np.sign(rng.standard_normal(p)) * np.repeat(rng.random(p // 4 + 1) + 0.5, 4)[:p]
    if kind == "tinyb":
        b[rng.random(p) < 0.3] *= 1e-12
    return S, b, n


# ~30 problems: p 2..300, rho 0 / 0.5 / 0.9 / 0.98, lar and lasso, with and without the intercept, ties, zero columns, tiny b
_KINDS = ["plain"] * 4 + ["ties", "zerocol", "tinyb"]
CASES = []
for _i in range(30):
    _r = np.random.default_rng(700 + _i)
    _kind = _KINDS[_i % len(_KINDS)]
    _p = int(_r.choice([_r.integers(2, 12), _r.integers(12, 80), _r.integers(80, 301)]))
    if _kind != "plain":
        _p = max(_p, 8)
    _icpt = bool(_i % 3 == 1) and _kind != "ties"
    CASES.append((_p, float([0.0, 0.5, 0.9, 0.98][_i % 4]), 7100 + _i, _kind, _icpt, "lasso" if _i % 2 else "lar"))


@pytest.mark.parametrize("name", sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "F3*_lars_*.npz"))))
def test_certificate_accepts_the_golden_paths(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    typ = "lasso" if name.endswith("lasso") else "lar"
    icpt = name.startswith("F3i")
    S, b, n = lars_case(z)
    if "beta" in z.files:                  # the reference's recorded path itself
        r = {"beta": z["beta"], "beta0": z["beta0"], "AIC": z["AIC"], "BIC": z["BIC"]}
    else:                                  # p = 250: only every 10th row is stored; certify the oracle's path
        r = orc.lars_lsa(S, b, icpt, n, type=typ)
    res = lc.certify(S, b, icpt, n, typ, r)
    assert max(res.values()) < 1e-13, res


@pytest.mark.parametrize("p,rho,seed,kind,icpt,typ", CASES)
def test_certificate_accepts_oracle_paths(p, rho, seed, kind, icpt, typ):
    S, b, n = _problem(p, rho, seed, kind)
    r = orc.lars_lsa(S, b, icpt, n, type=typ)
    res = lc.certify(S, b, icpt, n, typ, r)
    assert max(res.values()) < 1e-13, res


def _valid(typ="lasso", icpt=True, p=60, rho=0.9, seed=3):
    S, b, n = _problem(p, rho, seed)
    r = orc.lars_lsa(S, b, icpt, n, type=typ)
    lc.certify(S, b, icpt, n, typ, r)
    return S, b, n, r


def _rejected(S, b, icpt, n, typ, r, cond):
    with pytest.raises(lc.CertificateError) as e:
        lc.certify(S, b, icpt, n, typ, r)
    assert any(c in str(e.value) for c in cond), str(e.value)
    return str(e.value)


def _copy(r):
    return {k: np.array(v, dtype=np.float64) for k, v in r.items()}


def _big_step(r):
    """the step with the largest change of the path (where a relative error of 1e-6 is largest in absolute terms)"""
    return int(np.argmax(np.abs(np.diff(r["beta"], axis=0)).sum(axis=1))) + 1


@pytest.mark.parametrize("typ,icpt", [("lar", False), ("lasso", True)])
def test_certificate_rejects_a_nudged_coefficient(typ, icpt):
    S, b, n, r = _valid(typ, icpt)
    q = _copy(r)
    k = _big_step(r)
    j = int(np.argmax(np.abs(q["beta"][k])))
    q["beta"][k, j] *= 1 + 1e-6
    msg = _rejected(S, b, icpt, n, typ, q, ("equicorrelation", "breakpoint", "step_support", "derived"))
    assert "step %d" % k in msg or "derived" in msg


@pytest.mark.parametrize("scale", [1 + 1e-6, 1 - 1e-6])
@pytest.mark.parametrize("typ", ["lar", "lasso"])
def test_certificate_rejects_a_scaled_step_length(typ, scale):
    S, b, n, r = _valid(typ, False)
    q = _copy(r)
    k = _big_step(r)
    q["beta"][k] = q["beta"][k - 1] + scale * (q["beta"][k] - q["beta"][k - 1])
    _rejected(S, b, False, n, typ, q, ("equicorrelation", "breakpoint", "step_support"))


@pytest.mark.parametrize("typ", ["lar", "lasso"])
def test_certificate_rejects_merged_breakpoints(typ):
    S, b, n, r = _valid(typ, True)
    q = _copy(r)
    k = _big_step(r)
    q = {key: np.delete(v, k, axis=0) for key, v in q.items()}
    _rejected(S, b, True, n, typ, q, ("step_support",))


def test_certificate_rejects_swapped_entry_order():
    S, b, n, r = _valid("lar", False)
    beta = r["beta"]
    first = [int(np.flatnonzero(beta[:, j])[0]) for j in range(beta.shape[1])]
    order = np.argsort(first)
    a, c = int(order[3]), int(order[4])                  # the fourth and fifth variables to enter
    q = _copy(r)
    absb = np.abs(b)
    for k in range(first[a], first[c]):                   # points where a is active and c is not: c takes a's place
        q["beta"][k, c] = beta[k, a] / absb[a] * absb[c]
        q["beta"][k, a] = 0.0
    _rejected(S, b, False, n, "lar", q, ("equicorrelation", "step_support", "breakpoint"))


def test_certificate_rejects_a_flipped_lasso_sign():
    S, b, n, r = _valid("lasso", False)
    q = _copy(r)
    k = _big_step(r)
    j = int(np.argmax(np.abs(q["beta"][k])))
    q["beta"][k, j] = -q["beta"][k, j]
    _rejected(S, b, False, n, "lasso", q, ("lasso_sign", "equicorrelation"))
    # the same path read as a lar path is valid: only the lasso forbids a coefficient whose sign disagrees with its correlation
    rl = orc.lars_lsa(S, b, False, n, type="lar")
    flips = [(k, j) for k in range(rl["beta"].shape[0]) for j in np.flatnonzero(rl["beta"][k])
             if np.sign(rl["beta"][k, j]) != np.sign(rl["beta"][k - 1, j]) and rl["beta"][k - 1, j] != 0]
    assert flips                                          # (this lar path has coefficients that cross zero)
    _rejected(S, b, False, n, "lasso", rl, ("lasso_sign",))


def test_certificate_rejects_a_truncated_path():
    S, b, n, r = _valid("lasso", True)
    q = {k: v[:-3] for k, v in _copy(r).items()}
    _rejected(S, b, True, n, "lasso", q, ("final_point",))
    # a path cut by max_steps is complete as far as it goes
    K = q["beta"].shape[0] - 1
    lc.certify(S, b, True, n, "lasso", q, max_steps=K)


@pytest.mark.parametrize("key", ["beta0", "AIC", "BIC"])
def test_certificate_rejects_derived_outputs_off_by_1e9(key):
    S, b, n, r = _valid("lasso", True)
    q = _copy(r)
    i = int(np.argmax(np.abs(q[key])))
    q[key][i] *= 1 + 1e-9
    _rejected(S, b, True, n, "lasso", q, ("derived",))


def test_certificate_rejects_a_wrong_dof():
    S, b, n, r = _valid("lar", False)
    q = _copy(r)
    q["AIC"][5] += 2.0
    _rejected(S, b, False, n, "lar", q, ("derived",))
