"""CPU: the negative-binomial reference (tests/negbin_reference.py) checked against itself -- analytic terms against numeric
derivatives, the alpha -> 0 limit against mpmath, two independent routes to one MLE, the alpha = 0 branch against the Poisson
reference -- and the parts of the feature that need no GPU: the C ABI declarations, the package exports, simulate_negbin."""
import os
import re

import numpy as np
import pytest

import negbin_reference as nr
import poisson_reference as pr
from conftest import ROOT


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _small(intercept=True, offset=True, alpha=0.7, n=60, p=3, seed=3):
    X, y, o = nr.data(seed, n, p, intercept, offset, alpha)
    beta = np.linspace(-0.4, 0.5, p + intercept)
    return X, y, o, beta


@pytest.mark.parametrize("intercept,offset", [(False, False), (True, True)])
def test_score_and_information_against_central_differences(intercept, offset):
    alpha = 0.7
    X, y, o, beta = _small(intercept, offset, alpha)
    ll, g, H, mu, _, _, _ = nr.terms(X, y, beta, alpha, o, intercept)
    # g against central differences of loglik: truncation h^2 |l'''| / 6 ~ 1e-10 |g|, rounding eps |l| / h ~ 1e-16 * 1e2 / 1e-5 = 1e-9
    h = 1e-5
    gn = np.array([(nr.terms(X, y, beta + h * e, alpha, o, intercept)[0] - nr.terms(X, y, beta - h * e, alpha, o, intercept)[0]) / (2 * h)
                   for e in np.eye(len(beta))])
    assert rel(gn, g) <= 1e-7, rel(gn, g)
    # H is the EXPECTED information.  loglik is linear in y but for beta-free terms, so the expectation of the Hessian is the Hessian with y
    # frozen at mu(beta): central differences of the (just checked) score with y := mu.  Truncation h^2 ~ 1e-10, rounding 1e-16 / 1e-5.
    Hn = np.array([(nr.terms(X, mu, beta + h * e, alpha, o, intercept)[1] - nr.terms(X, mu, beta - h * e, alpha, o, intercept)[1]) / (2 * h)
                   for e in np.eye(len(beta))])
    assert rel(-Hn, H) <= 1e-8, rel(-Hn, H)
    assert np.all(np.linalg.eigvalsh(H) > 0)


def test_theta_score_and_information_against_differences():
    alpha = 0.7
    X, y, o, beta = _small(alpha=alpha)
    th = 1.0 / alpha
    _, _, _, _, s, i, _ = nr.terms(X, y, beta, alpha, o, True)
    h = 1e-5 * th
    f = lambda t: nr.terms(X, y, beta, 1.0 / t, o, True)
    assert abs((f(th + h)[0] - f(th - h)[0]) / (2 * h) - s) <= 1e-7 * max(1.0, abs(s))
    assert abs(-(f(th + h)[4] - f(th - h)[4]) / (2 * h) - i) <= 1e-7 * max(1.0, abs(i))


def test_alpha_derivative_at_zero_is_half_the_dispersion_sum():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    X, y, o, _ = _small(alpha=0.7, n=40)
    b = pr.fit(X, y, o, True)[0]                       # the Poisson MLE
    mu = pr.terms(X, y, b, o, True)[3]

    def loglik(alpha):                                 # the textbook NB2 log-likelihood in 50 digits
        th = 1 / mp.mpf(alpha)
        return sum(mp.loggamma(yi + th) - mp.loggamma(th) - mp.loggamma(yi + 1) + th * mp.log(th) + yi * mp.log(mi)
                   - (th + yi) * mp.log(th + mi) for yi, mi in zip(map(mp.mpf, y), map(mp.mpf, mu)))
    pois = sum(yi * mp.log(mi) - mi - mp.loggamma(yi + 1) for yi, mi in zip(map(mp.mpf, y), map(mp.mpf, mu)))
    want = 0.5 * float(np.sum((y - mu) ** 2 - y))
    a = mp.mpf("1e-9")
    got = float((loglik(a) - pois) / a)                # one-sided: the next term is O(alpha sum mu^3) ~ 1e-9 * 1e3
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    # and the reference's own terms() approach the Poisson ones
    llp = pr.terms(X, y, b, o, True)[0]
    assert abs(nr.terms(X, y, b, 1e-7, o, True)[0] - llp) <= 1e-5 * abs(llp)


GRID = [(p, a) for p in (1, 7, 50, 100, 130) for a in (0.2, 1.0)]


@pytest.mark.parametrize("p,alpha", GRID)
def test_two_routes_reach_one_mle(p, alpha):
    """the alternating fit against the root of the profile score, on the GPU fit test's grid (one partition of it)"""
    n = max(3000, 20 * p)
    X, y, o = nr.data(40 + p, n, p, True, True, alpha)
    b1, H1, ll1, a1, i1, p1 = nr.fit(X, y, o, True)
    b2, H2, ll2, a2, i2, p2 = nr.fit_profile(X, y, o, True)
    assert a1 > 0 and a2 > 0
    assert rel(b1, b2) <= 1e-10 and rel(H1, H2) <= 1e-10, (rel(b1, b2), rel(H1, H2))
    assert abs(a1 - a2) <= 1e-9 * a2, abs(a1 - a2) / a2
    assert abs(ll1 - ll2) <= 1e-10 * abs(ll2)
    # stationarity of the result
    _, g, H, _, s, i, _ = nr.terms(X, y, b1, a1, o, True)
    assert np.max(np.abs(np.linalg.solve(H, g))) <= 1e-10 * max(1.0, np.max(np.abs(b1)))
    assert abs(s * a1 / i) <= 1e-9


def test_underdispersed_sample_is_the_poisson_block():
    rng = np.random.default_rng(8)
    n, p = 4000, 5
    X = rng.uniform(-0.5, 0.5, (n, p))
    mu = np.exp(0.2 + X @ np.array([0.5, 0.5, 0.0, 0.0, 0.0]))
    y = rng.binomial(4, mu / 4).astype(np.float64)     # the Poisson mean with the variance mu (1 - mu / 4)
    b, H, ll, a, info, pearson = nr.fit(X, y, None, True)
    assert a == 0.0 and info == 0.0 and pearson < n
    bp, Hp, llp = pr.fit(X, y, None, True)
    assert np.array_equal(b, bp) and np.array_equal(H, Hp) and ll == llp
    blk, pblk = nr.block(X, y, None, True), pr.block(X, y, None, True)
    assert all(np.array_equal(u, v) for u, v in zip(blk, pblk))


def test_fixed_alpha_fit_is_stationary_in_beta():
    X, y, o = nr.data(5, 3000, 6, True, True, 0.5)
    b, H, ll, a, info, pearson = nr.fit(X, y, o, True, alpha=0.3)
    assert a == 0.3
    _, g, H2, _, _, _, _ = nr.terms(X, y, b, 0.3, o, True)
    assert np.max(np.abs(np.linalg.solve(H2, g))) <= 1e-10 and np.array_equal(H, H2)


# ---- the parts of the feature that need no GPU ---------------------------------------------------------------------------
def test_negbin_entries_are_declared_and_bound():
    from dlsa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dlsa_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("dlsa_negbin_workspace_bytes", "dlsa_negbin_pass_f64", "dlsa_negbin_fit_f64"):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name + " is not declared in include/dlsa_hip.h"
        assert name in _lib.SIGNATURES, name + " is not in _lib.SIGNATURES"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert len(_lib.SIGNATURES["dlsa_negbin_pass_f64"][1]) == 19 and len(_lib.SIGNATURES["dlsa_negbin_fit_f64"][1]) == 25


def test_negbin_entries_validate_arguments_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    lib = _lib.load()
    assert lib.dlsa_negbin_workspace_bytes(1000, 0, 0, 1) == 0 and lib.dlsa_negbin_workspace_bytes(1000, 5, 1, 0) == 0
    assert lib.dlsa_negbin_workspace_bytes(1000, 5, 1, 3) >= lib.dlsa_poisson_workspace_bytes(1000, 5, 1, 3)
    rc = lib.dlsa_negbin_pass_f64(None, 4, None, None, None, 0.5, 10, 4, 0, None, 4, None, None, None, None, None, None, 0, None)
    assert rc == 1 and "null" in _lib.last_error()


# (max_rows, p) -> dlsa_negbin_workspace_bytes for (intercept, row_step) = (0, 1), (0, 25), (1, 1), (1, 25): the values of the library
# before the pass scratch went through count_pass.h's one take list
WORKSPACE_BYTES = {
    (0, 1): (4670976, 4671488, 4670976, 4671488),
    (0, 100): (5541120, 5541632, 5542656, 5543168),
    (0, 130): (11102720, 11103232, 11104768, 11105280),
    (0, 600): (62886912, 62887424, 62896640, 62897152),
    (0, 1025): (151528960, 151529472, 151545344, 151545856),
    (1, 1): (4670976, 4671488, 4670976, 4671488),
    (1, 100): (5541120, 5541632, 5542656, 5543168),
    (1, 130): (11102720, 11103232, 11104768, 11105280),
    (1, 600): (62886912, 62887424, 62896640, 62897152),
    (1, 1025): (151528960, 151529472, 151545344, 151545856),
    (3001, 1): (4980736, 5028864, 4980736, 5028864),
    (3001, 100): (6637312, 6685440, 6638848, 6686976),
    (3001, 130): (13509632, 13557760, 13511680, 13559808),
    (3001, 600): (89148928, 89197056, 89158656, 89206784),
    (3001, 1025): (227336192, 227384320, 227352576, 227400704),
    (10 ** 6, 1): (37185536, 61038080, 37185536, 61038080),
    (10 ** 6, 100): (87601152, 111453696, 87602688, 111455232),
    (10 ** 6, 130): (175737856, 199590400, 175739904, 199592448),
    (10 ** 6, 600): (183744000, 207596544, 183753728, 207606272),
    (10 ** 6, 1025): (319047680, 342900224, 319064064, 342916608),
}


def test_workspace_bytes_are_pinned():
    """the layout takes the pass's six scratch arrays through the helper it shares with poisson.hip: sizes, order and alignment are
    those of the list it replaced"""
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    lib = _lib.load()
    assert len(WORKSPACE_BYTES) == 4 * 5
    for (n, p), want in WORKSPACE_BYTES.items():
        got = tuple(lib.dlsa_negbin_workspace_bytes(n, p, icpt, step) for icpt in (0, 1) for step in (1, 25))
        assert got == want, (n, p, got, want)


def test_package_exports_the_negbin_interface():
    import inspect
    import dlsa_amd
    for name in ("fit_negbin_partitions", "negbin_model", "negbin_model_eval", "simulate_negbin", "combine_dispersion"):
        assert callable(getattr(dlsa_amd, name)), name
    assert "extra" in inspect.signature(dlsa_amd.MappedBlocks.__init__).parameters
    assert "alpha" in inspect.signature(dlsa_amd.fit_negbin_partitions).parameters


def test_combine_dispersion_is_the_information_weighted_log_mean():
    import torch
    import dlsa_amd
    z = torch.zeros
    mb = dlsa_amd.MappedBlocks(z(4, 2), z(4, 2), z(4, 2, 2), ["a", "b"], status=[0, 0, 2, 0],
                               extra={"alpha": [0.5, 2.0, 9.0, 0.0], "alpha_info": [300.0, 100.0, 50.0, 0.0], "pearson": [1.0] * 4})
    assert abs(dlsa_amd.combine_dispersion(mb) - np.exp((300 * np.log(0.5) + 100 * np.log(2.0)) / 400)) <= 1e-15
    assert dlsa_amd.MappedBlocks(z(1, 2), z(1, 2), z(1, 2, 2), ["a", "b"]).extra == {}
    none = dlsa_amd.MappedBlocks(z(1, 2), z(1, 2), z(1, 2, 2), ["a", "b"], extra={"alpha": [0.0], "alpha_info": [0.0], "pearson": [1.0]})
    assert dlsa_amd.combine_dispersion(none) == 0.0


def test_simulate_negbin_on_the_host(monkeypatch):
    """simulate_negbin draws on the host; its rows come from engine.synth (the GPU's seeded generator), replaced here by the oracle's
    restatement of the same generator."""
    import torch
    import dlsa_amd
    from dlsa_amd import models
    from oracle import dlsa_oracle as orc

    def synth(seed, row0, n, p, labels=True, **kw):
        return torch.from_numpy(orc.synth_features(seed, row0, n, p)), None
    monkeypatch.setattr(models.engine, "synth", synth)
    n, p, alpha = 40_000, 6, 0.5
    a = dlsa_amd.simulate_negbin(n, p, 4, alpha, seed=9, exposure=True)
    b = dlsa_amd.simulate_poisson(n, p, 4, seed=9, exposure=True)
    assert list(a.columns) == list(b.columns) == ["partition_id", "y", "exposure"] + ["x%d" % i for i in range(p)]
    assert a.drop(columns=["y"]).equals(b.drop(columns=["y"]))
    beta = np.where(np.arange(p) < int(0.4 * p), 0.5, 0.0)
    mu = a["exposure"].to_numpy() * np.exp(a.iloc[:, 3:].to_numpy() @ beta)
    y = a["y"].to_numpy()
    assert np.all(y >= 0) and np.all(y == np.floor(y))
    # Pearson dispersion at the true mu: E (y - mu)^2 / mu = 1 + alpha mu.  Its standard error at n = 4e4 is ~ sqrt(var / n) with the
    # NB2 fourth moment: a few per cent of the value at most, so 5 % holds with a wide margin
    disp = float(np.mean((y - mu) ** 2 / mu))
    assert abs(disp - (1 + alpha * mu.mean())) <= 0.05 * (1 + alpha * mu.mean()), (disp, 1 + alpha * mu.mean())
    with pytest.raises(ValueError):
        dlsa_amd.simulate_negbin(10, 2, 1, 0.0)
