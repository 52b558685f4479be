"""GPU: the row terms of the probit and cloglog passes (csrc/binary_terms.h through count_pass_kernel) held to ulps over the WHOLE
range of eta, against mpmath values on designs whose eta is known exactly (tests/binary_reference.py -- reference, grids, designs
and the derivation of every bound; tests/test_binary_reference_cpu.py shows that the bounds can be met and that they reject the
textbook forms).

Per link and regime grid: w_out per row, and g, diag H and loglik as sums, at p = 3 (one column chunk, scalar loads), p = 4
(vector loads) and p = 130 (two chunks); without and with the implicit intercept (the reference takes eta := fl(b0 + x)) and with
per-row offsets whose sum with x is the grid point again.  n = 2 G rows: every grid point meets both responses."""
import math

import numpy as np
import pytest

import binary_reference as br

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORST = {}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_pass(eng, d):
    X = torch.zeros((d.n, d.p), dtype=torch.float64, device="cuda")
    X[torch.arange(d.n, device="cuda"), dev(d.col)] = dev(d.x)
    fn = eng.probit_pass if d.link == "probit" else eng.cloglog_pass
    H, g, ll, w = fn(X, dev(d.y), dev(d.beta_full()), offset=dev(d.offset()), fit_intercept=d.b0 is not None, want_H=True, want_w=True)
    return H.cpu().numpy(), g.cpu().numpy(), ll.cpu().numpy(), w.cpu().numpy()


def variants(name):
    """(b0, offset): plain; the implicit intercept at the regime's centre; offsets; the intercept's kernel path (BORDER) with offsets"""
    return ((None, False), (br.regime_centre(name), False), (None, True), (0.0, True))


CASES = [(link, name) for link in br.LINKS for name in br.REGIMES[link] + ("full",)]


@pytest.mark.parametrize("p", [3, 4, 130])
@pytest.mark.parametrize("link,name", CASES)
def test_pass_terms_within_the_bounds(eng, link, name, p):
    b = br.bounds(link, name)
    for b0, offset in variants(name):
        d = br.Design(link, name, p, b0=b0, offset=offset)
        H, g, ll, w = run_pass(eng, d)
        what = "%s %s p=%d b0=%r offset=%r" % (link, name, p, b0, offset)
        assert np.all(np.isfinite(w)) and np.all(w >= 0.0) and np.all(np.isfinite(g)) and np.all(np.isfinite(ll)), what
        icpt = 1 if b0 is not None else 0
        assert np.array_equal(H, H.T), what
        ratio_w = br.check_rows(link, w, "w", d.eta(), d.y, b, what)
        ratio = br.check_sums(d, b, g=g, Hdiag=np.diag(H)[icpt:].copy(), ll=ll, what=what)
        offd = H[icpt:, icpt:][~np.eye(p, dtype=bool)]
        assert not np.any(offd != 0.0), (what, "nonzero off-diagonal of H")
        key = (link, str(name))
        WORST[key] = (max(WORST.get(key, (0, 0))[0], ratio_w), max(WORST.get(key, (0, 0))[1], ratio))
    print("%s %s p=%d: worst w error / bound %.3f, worst sum error / bound %.3f" % ((link, name, p) + WORST[(link, str(name))]))


def test_cloglog_beyond_the_range_of_y1(eng):
    """eta from 6.6 to 710: the y = 0 rows within the bounds (l = -mu), the y = 1 rows without a NaN (l = -e^-mu -> -0, r = w = 0 once
    e^-mu is 0); mu = inf (eta > 709.78): l = -inf for y = 0, zeros for y = 1"""
    g = br.grid("cloglog", "beyond")
    b = br.bounds("cloglog", "beyond")
    n = g.size
    for y in (0.0, 1.0):
        H, gr, ll, w = eng.cloglog_pass(dev(g[:, None].copy()), dev(np.full(n, y)), dev(np.ones(1)), want_H=True, want_w=True)
        w, ll, gr, H = w.cpu().numpy(), float(ll.item()), float(gr.item()), float(H.item())
        assert not np.any(np.isnan(w)) and not math.isnan(ll) and not math.isnan(gr) and not math.isnan(H)
        if y == 0.0:
            br.check_rows("cloglog", w, "w", g, np.zeros(n), b, "cloglog beyond y=0")
        else:
            assert np.all(w[g > 6.7] == 0.0) and np.all(w >= 0.0)
    big = np.array([709.79, 710.0, 720.0, 1e6])
    for y, want_ll in ((1.0, 0.0), (0.0, -math.inf)):
        _, gr, ll, w = eng.cloglog_pass(dev(big[:, None].copy()), dev(np.full(4, y)), dev(np.ones(1)), want_H=False, want_w=True)
        assert float(ll.item()) == want_ll, (y, float(ll.item()))
        if y == 1.0:
            assert not w.cpu().numpy().any() and float(gr.item()) == 0.0


def test_probit_beyond_1e154(eng):
    """|z| beyond 1e154: z * z overflows; l = -inf for z < 0 and -0 for z > 0, w and r finite, no NaN"""
    z = np.array([1.1e154, 1.4e154, 1e200, 1e300])
    for y, want_ll in ((1.0, 0.0), (0.0, -math.inf)):
        _, gr, ll, w = eng.probit_pass(dev(z[:, None].copy()), dev(np.full(4, y)), dev(np.ones(1)), want_H=False, want_w=True)
        w = w.cpu().numpy()
        assert float(ll.item()) == want_ll and not np.any(np.isnan(w)) and np.all(w >= 0.0)
        if y == 1.0:
            assert not w.any()
        else:
            assert np.all(np.abs(w - 1.0) <= 1e-15)             # lambda K -> a (1 / a) = 1
