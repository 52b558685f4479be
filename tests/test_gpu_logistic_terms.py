"""GPU: every kernel that evaluates the logistic row terms (csrc/logistic.h; its hand-scheduled copy in irls_pass.hip; OhLogitRow
in onehot.hip) held to ulps over the WHOLE range of eta, against 50-digit values on designs whose eta is known exactly
(tests/logistic_reference.py -- reference, designs and the derivation of every bound; tests/test_logistic_reference_cpu.py shows
that the bounds can be met and that they reject the mutants they are there for).

Per route: w per row on the full grid within B_w ulps AND bit-identical to the w of the p = 1 register-load call on the same eta;
on each of the 22 regimes (a whole call inside one tail, the branch switch, the subnormals, the clamp) g, loglik and -- where the
route has one -- H within the derived sum bounds, relative to their OWN size, with exact zeros where no row contributes.
Routes are asserted by name where the library reports one (gram_last_kernel()).

Not reached here (no entry takes a given beta for them): the ICPT fused pass, the BF lock-step pass, the BORDER form and
irls_small.hip, which run only inside a fit.

Measured on an MI355X: w is bit-identical on every route, worst error 3.503 ulp at eta = 0.19181244953509236 (the plain numpy
evaluation: E_w = 3.26, E_mu = 2.12, E_sp = 1.20 on the same grid, so B_w = 6.52, B_mu = 4.24, B_sp = 4); the worst sum sits at
0.39 of its bound (g of the register-load pass, p >= 260), loglik at 0.13, the fused pass's H and g at 0.20.  DESIGN.md section 4.2
has the table."""
import numpy as np
import pytest

import logistic_reference as lr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIGURES = {}      # route -> worst ulp error of w seen (printed by every test; collected for the last one)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_design(d, pad=0):
    """the design's rows on the device (pad: as columns 1 .. p of a buffer with p + pad columns, a view without a copy)"""
    big = torch.zeros((d.n, d.p + pad), dtype=torch.float64, device="cuda")
    X = big[:, 1:1 + d.p] if pad else big
    X[torch.arange(d.n, device="cuda"), dev(d.col)] = dev(d.x)
    return X, dev(d.y), dev(d.beta_full())


_base = {}


def base_w(eng, eta):
    """w of the p = 1 register-load call (logit_kernel<1, 8, false>) on the same eta: x = eta, beta = 1"""
    key = eta.tobytes()
    if key not in _base:
        w, _, _ = eng.logit_pass(dev(eta[:, None]), dev(np.zeros(eta.size)), dev(np.ones(1)), want_g=False, want_loglik=False)
        _base[key] = w
    return _base[key]


def note(route, ulp, eta):
    if route not in FIGURES or ulp > FIGURES[route][0]:
        FIGURES[route] = (ulp, eta)


def check_w(eng, d, w, route, what):
    """per-row w: within B_w of the 50-digit value, and the bits of the p = 1 call"""
    eta = d.eta()
    ulp, at = lr.check_rows(w.cpu().numpy(), "w", eta, lr.bounds(d.name), what=what)
    note(route, ulp, at)
    wb = base_w(eng, eta)
    if not torch.equal(w, wb):
        i = int(torch.nonzero(w != wb)[0])
        raise AssertionError("%s: w differs from the p = 1 call at eta = %r: %s vs %s" % (
            what, float(eta[i]), float(w[i]).hex(), float(wb[i]).hex()))


def regime_cases():
    return [(c, lr.regime_centre(c)) for c in lr.REGIMES]


# ---------------------------------------------------------------------------------------------------------------- logit_kernel
@pytest.mark.parametrize("p", [1, 7, 8, 129, 130, 257, 260, 513, 600, 1025, 1030])
def test_register_load_logit_pass(eng, p):
    """logit_kernel<NC, RB, VEC> for NC = 1, 2, 4, 8, 16; even p on the vector loads, odd p on the scalar ones; both with the
    implicit intercept too"""
    route = "logit_kernel p=%d" % p
    for b0 in (None, 0.0):
        d = lr.Design("full", 4099, p, b0=b0)
        X, y, beta = dev_design(d)
        w, g, ll = eng.logit_pass(X, y, beta, fit_intercept=b0 is not None)
        assert np.all(np.isfinite(g.cpu().numpy())) and np.isfinite(float(ll))
        check_w(eng, d, w, route, "%s full b0=%r" % (route, b0))
    worst = 0.0
    for c, centre in regime_cases():
        for n in (67, 3001):
            for b0 in (None, centre):
                d = lr.Design(c, n, p, b0=b0)
                X, y, beta = dev_design(d)
                w, g, ll = eng.logit_pass(X, y, beta, fit_intercept=b0 is not None)
                what = "%s regime %s n=%d b0=%r" % (route, c, n, b0)
                check_w(eng, d, w, route, what)
                worst = max(worst, lr.check_sums(d, lr.bounds(c), g=g.cpu().numpy(), ll=ll.cpu().numpy(), what=what))
    print("%s: worst w %.3f ulp at eta = %r; worst sum error / bound %.3f" % ((route,) + FIGURES[route] + (worst,)))


@pytest.mark.parametrize("p,pad", [(130, 3), (130, 2), (8, 3)])
def test_register_load_logit_pass_even_width_on_the_scalar_loads(eng, p, pad):
    """an even p takes the scalar loads only through the rows' pitch (odd) or base (8 bytes off a 16-byte boundary)"""
    route = "logit_kernel p=%d scalar loads (pad %d)" % (p, pad)
    d = lr.Design("full", 4099, p)
    X, y, beta = dev_design(d, pad=pad)
    assert X.stride(0) == p + pad and X.stride(1) == 1 and (pad != 2 or X.data_ptr() % 16 == 8)
    w, g, ll = eng.logit_pass(X, y, beta)
    check_w(eng, d, w, route, route + " full")
    for c, centre in regime_cases():
        d = lr.Design(c, 67, p, b0=centre)
        X, y, beta = dev_design(d, pad=pad)
        w, g, ll = eng.logit_pass(X, y, beta, fit_intercept=True)
        check_w(eng, d, w, route, "%s regime %s" % (route, c))
        lr.check_sums(d, lr.bounds(c), g=g.cpu().numpy(), ll=ll.cpu().numpy(), what="%s regime %s" % (route, c))
    print("%s: worst w %.3f ulp at eta = %r" % ((route,) + FIGURES[route]))


# ---------------------------------------------------------------------------------------------------------------- the ring
N_RING = 8219


@pytest.mark.parametrize("p", [49, 52, 64, 100, 112, 120, 119])
def test_ring_logit_pass(eng, p):
    """irls_pass_narrow_kernel<*, false, ...>: short rows (p <= 80) two workgroups per CU, longer ones one; with w and without"""
    route = "ring p=%d" % p
    d = lr.Design("full", N_RING, p)
    X, y, beta = dev_design(d)
    w, g, ll = eng.logit_pass(X, y, beta)
    assert eng.gram_last_kernel()[0].startswith("irls_pass_narrow_kernel<true,false"), eng.gram_last_kernel()
    check_w(eng, d, w, route, route + " full")
    worst = 0.0
    for c, _ in regime_cases():
        d = lr.Design(c, N_RING, p)
        X, y, beta = dev_design(d)
        w, g, ll = eng.logit_pass(X, y, beta)
        assert eng.gram_last_kernel()[0].startswith("irls_pass_narrow_kernel<true,false"), eng.gram_last_kernel()
        what = "%s regime %s" % (route, c)
        check_w(eng, d, w, route, what)
        worst = max(worst, lr.check_sums(d, lr.bounds(c), g=g.cpu().numpy(), ll=ll.cpu().numpy(), what=what))
        _, g2, ll2 = eng.logit_pass(X, y, beta, want_w=False)
        assert eng.gram_last_kernel()[0].startswith("irls_pass_narrow_kernel<false,false"), eng.gram_last_kernel()
        worst = max(worst, lr.check_sums(d, lr.bounds(c), g=g2.cpu().numpy(), ll=ll2.cpu().numpy(), what=what + " (no w)"))
    print("%s: worst w %.3f ulp at eta = %r; worst sum error / bound %.3f" % ((route,) + FIGURES[route] + (worst,)))


# ---------------------------------------------------------------------------------------------------------------- the fused pass
@pytest.mark.parametrize("p", [49, 64, 99, 100, 104, 112, 116, 119, 120])
def test_fused_newton_pass(eng, p):
    """irls_pass_narrow_kernel<*, true, ...>: BATCH + VC (p <= 100), PIN only (104, 112), not PIN (116, 120), odd packed rows (49,
    99, 119); with w written and without"""
    route = "fused p=%d" % p
    d = lr.Design("full", N_RING, p)
    X, y, beta = dev_design(d)
    H, g, ll, w = eng.irls_pass(X, y, beta, want_w=True)
    assert eng.gram_last_kernel()[0].startswith("irls_pass_narrow_kernel<true,true"), eng.gram_last_kernel()
    check_w(eng, d, w, route, route + " full")
    worst = 0.0
    for c, _ in regime_cases():
        d = lr.Design(c, N_RING, p)
        X, y, beta = dev_design(d)
        what = "%s regime %s" % (route, c)
        H, g, ll, w = eng.irls_pass(X, y, beta, want_w=True)
        assert eng.gram_last_kernel()[0].startswith("irls_pass_narrow_kernel<true,true"), eng.gram_last_kernel()
        check_w(eng, d, w, route, what)
        worst = max(worst, lr.check_sums(d, lr.bounds(c), g=g.cpu().numpy(), H=H.cpu().numpy(), ll=ll.cpu().numpy(), what=what))
        H2, g2, ll2, _ = eng.irls_pass(X, y, beta)
        assert eng.gram_last_kernel()[0].startswith("irls_pass_narrow_kernel<false,true"), eng.gram_last_kernel()
        worst = max(worst, lr.check_sums(d, lr.bounds(c), g=g2.cpu().numpy(), H=H2.cpu().numpy(), ll=ll2.cpu().numpy(), what=what + " (no w)"))
    print("%s: worst w %.3f ulp at eta = %r; worst sum error / bound %.3f" % ((route,) + FIGURES[route] + (worst,)))


# ---------------------------------------------------------------------------------------------------------------- the IMG form
@pytest.mark.parametrize("p", [122, 130, 300])
def test_wide_newton_pass(eng, p):
    """logit_kernel<NC, RB, VEC, false, true> (the pass that also writes the bf16 images; H_approx, a preconditioner, is not
    checked here), with the implicit intercept too"""
    n = 32771
    route = "wide (IMG) p=%d" % p
    for b0 in (None, 0.0):
        d = lr.Design("full", n, p, b0=b0)
        X, y, beta = dev_design(d)
        _, g, ll, w = eng.newton_wide_pass(X, y, beta, fit_intercept=b0 is not None, want_w=True)
        check_w(eng, d, w, route, "%s full b0=%r" % (route, b0))
    worst = 0.0
    for c, centre in regime_cases():
        for b0 in (None, centre):
            d = lr.Design(c, n, p, b0=b0)
            X, y, beta = dev_design(d)
            _, g, ll, w = eng.newton_wide_pass(X, y, beta, fit_intercept=b0 is not None, want_w=True)
            what = "%s regime %s b0=%r" % (route, c, b0)
            check_w(eng, d, w, route, what)
            worst = max(worst, lr.check_sums(d, lr.bounds(c), g=g.cpu().numpy(), ll=ll.cpu().numpy(), what=what))
    print("%s: worst w %.3f ulp at eta = %r; worst sum error / bound %.3f" % ((route,) + FIGURES[route] + (worst,)))


# ---------------------------------------------------------------------------------------------------------------- loglik
SCALES = (1.0, -0.5, 2.0, -0.25, -1.0, 0.5, -2.0, 0.25)


@pytest.mark.parametrize("p", [8, 130, 1030])
@pytest.mark.parametrize("ncol", [3, 8])
def test_loglik_columns(eng, p, ncol):
    """loglik_kernel C = 4 (c = 3) and C = 8, the column split beyond p = 1024; column j of par is s_j beta with s_j a power of two
    (the products stay exact), so its eta is s_j times the design's.  B_* of the full grid: a scaled regime is another regime."""
    n = 67
    s = np.array(SCALES[:ncol])
    worst = 0.0
    for c, centre in regime_cases():
        for b0 in (None, centre):
            d = lr.Design(c, n, p, b0=b0)
            X, y, _ = dev_design(d)
            par = d.beta[:, None] * s[None, :]
            if b0 is not None:
                par = np.vstack([b0 * s[None, :], par])
            out = eng.loglik(X, y, dev(par), fit_intercept=b0 is not None).cpu().numpy()
            for j in range(ncol):
                worst = max(worst, lr.check_sums(d, lr.bounds("full"), ll=out[j], scale=float(s[j]), b0=None if b0 is None else float(b0 * s[j]),
                                                 what="loglik p=%d c=%d regime %s b0=%r column %d" % (p, ncol, c, b0, j)))
    print("loglik p=%d c=%d: worst sum error / bound %.3f" % (p, ncol, worst))


# ---------------------------------------------------------------------------------------------------------------- one-hot
def _numeric_plan(eng, p):
    return eng.OnehotPlan(p, [1] * p, list(range(p)), [0.0] * p, [1.0] * p, list(range(p)), [], [])


def test_onehot_logit_pass_eta_through_numeric_columns(eng):
    """OhLogitRow (exp_neg and rcp_newton of logistic.h, the library's log1p): eta through numeric columns"""
    route = "onehot numeric"
    p = 2
    plan = _numeric_plan(eng, p)
    d = lr.Design("full", 4099, p)
    X, y, beta = dev_design(d)
    w, g, ll = eng.onehot_logit_pass(plan, X, None, y, beta)
    check_w(eng, d, w, route, route + " full")
    worst = 0.0
    for c, _ in regime_cases():
        d = lr.Design(c, 4099, p)
        X, y, beta = dev_design(d)
        w, g, ll = eng.onehot_logit_pass(plan, X, None, y, beta)
        check_w(eng, d, w, route, "%s regime %s" % (route, c))
        worst = max(worst, lr.check_sums(d, lr.bounds(c), g=g.cpu().numpy(), ll=ll.cpu().numpy(), what="%s regime %s" % (route, c)))
    print("%s: worst w %.3f ulp at eta = %r; worst sum error / bound %.3f" % ((route,) + FIGURES[route] + (worst,)))


def test_onehot_logit_pass_eta_through_level_coefficients(eng):
    """a pure gather: one factor, level k's coefficient is grid point k, no numeric column (x = 1 in every term of g).  A plan
    holds at most 2048 columns, so the full grid's 4099 rows go in three calls of <= 1400 levels each."""
    route = "onehot gather"
    worst = 0.0
    for name in ("full",) + lr.REGIMES:
        base = lr.Design(name, 4099, 1)
        eta_k = np.ascontiguousarray(lr.grid(name))
        for lo in range(0, base.G, 1400):
            hi = min(base.G, lo + 1400)
            rows = np.nonzero((base.k >= lo) & (base.k < hi))[0]
            L = hi - lo
            plan = eng.OnehotPlan(L, [], [], [], [], [], [L], list(range(L)))
            codes = (base.k[rows] - lo).astype(np.int32)[:, None]
            yv = base.y[rows]
            w, g, ll = eng.onehot_logit_pass(plan, None, dev(codes), dev(yv), dev(eta_k[lo:hi]))
            sub = lr.GatherDesign(name, eta_k[lo:hi], base.k[rows] - lo, yv)
            check_w(eng, sub, w, route, "%s %s levels %d..%d" % (route, name, lo, hi))
            if name != "full":
                worst = max(worst, lr.check_sums(sub, lr.bounds(name), g=g.cpu().numpy(), ll=ll.cpu().numpy(), what="%s regime %s" % (route, name)))
    print("%s: worst w %.3f ulp at eta = %r; worst sum error / bound %.3f" % ((route,) + FIGURES[route] + (worst,)))


def test_device_w_against_the_emulation_of_logistic_h(eng):
    """How far the operation-by-operation emulation (exact fma, the rcp seed modelled as the fp32-rounded reciprocal) stands for
    the device: its mu and softplus figures are quoted where the device has no per-row output to measure.  The two may differ
    only through the seed; after two Newton steps that is at most an ulp of 1 / (1 + e), which enters w = e inv inv twice."""
    eta = np.ascontiguousarray(lr.full_grid())
    w = base_w(eng, eta).cpu().numpy()
    em = lr.emulate_logistic_h(eta)["w"]
    diff = np.abs(w - em) / lr.sp(em)
    print("device w == emulated w on %d of %d points of the full grid; worst difference %.1f ulp at eta = %r" % (
        int(np.sum(w == em)), eta.size, diff.max(), float(eta[int(np.argmax(diff))])))
    assert diff.max() <= 3.0            # two ulps of inv (it enters twice) and one more for the roundings they move


def test_zz_figures(eng):
    """the per-route figures in one place (DESIGN.md quotes them): worst ulp error of w per route, and the bounds they met"""
    b = lr.bounds("full")
    print("plain fp64 evaluation on the full grid: E_w %.2f E_mu %.2f E_sp %.2f -> B_w %.2f B_mu %.2f B_sp %.2f" % (
        b.E["w"], b.E["mu"], b.E["sp"], b.B["w"], b.B["mu"], b.B["sp"]))
    for route in sorted(FIGURES):
        print("%-45s w worst %.3f ulp at eta = %r" % ((route,) + FIGURES[route]))
    assert all(v[0] <= b.B["w"] for v in FIGURES.values())
