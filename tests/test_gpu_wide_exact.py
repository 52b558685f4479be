"""GPU: the bf16 Hessian of the wide Newton pass (csrc/irls_wide.hip: wide_syrk_kernel, wide_reduce_kernel; the IMG form of
csrc/logit.hip: logit_image) on designs whose answer it must reproduce exactly -- tests/exact_designs.py, whose mutants
(tests/test_exact_designs_cpu.py: a row or a 16-row chunk dropped, a row doubled, two rows of a batch with each other's weight, a
tile transposed, columns shifted, the intercept left last) every check below rejects.  tests/test_gpu_wide.py holds H~ to 2e-3 of
the diagonal scale, which passes the first four.

  tier A  integer rows, beta = 0: w = 1/4 on every row, H~ = [1 | X]'[1 | X] / 4 BIT FOR BIT; g = [1 | X]'(y - 1/2) too.  Every
          column-block count, odd chunk counts, ragged tails, row counts that wrap the LDS ring, strided / odd-pitch / NaN-padded rows.
  tier B  the probe design: per-row weights from eta = -6 .. 6, H~ BIT FOR BIT from the device's own w, zeros included.
  tier C  Gaussian rows: H~ against S'S of the host model of the image, S built from the device's own w; what is left is the
          fp32 accumulation, bounded per entry by m 2^-23 |S|'|S| (exact_designs.wide_bound; m rows per accumulator).  Nothing in
          the bound is measured.  Worst fractions seen (pytest -s prints them): DESIGN.md section 6.

Assumed of the device and checked where it can be: float(w) == 0.25 at eta = 0 (asserted), sqrtf correctly rounded (a 1-ulp miss
would flip a bf16 value once in 2^16 and show as a bit difference in tier B), the image scaled by ONE fp32 multiply before ONE
rounding to bf16, no flushing (the smallest product here is 2^-4 * 2.4e-3)."""
import functools

import numpy as np
import pytest

import exact_designs as ed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=2)
def tier_a_rows(p, n):
    """(X on the device, y, its exact Gram with the ones column first, [1 | X]'(y - 1/2)); the Gram by rocBLAS in fp64 -- exact in
    any order, and none of the code under test"""
    X = dev(ed.wide_a_design(p, n))
    y = dev((np.random.default_rng(p + n).random(n) < 0.5).astype(np.float64))
    R = torch.cat([torch.ones((n, 1), dtype=torch.float64, device="cuda"), X], dim=1)
    return X, y, R.T @ R, R.T @ (y - 0.5)


def check_tier_a(eng, X, y, G, g1, icpt, what):
    n, p = X.shape
    pe = p + icpt
    beta = torch.zeros(pe, dtype=torch.float64, device="cuda")
    H, g, ll, w = eng.newton_wide_pass(X, y, beta, fit_intercept=icpt, want_w=True)
    assert bool((w.float() == 0.25).all()), what                  # s = sqrtf(1/4) = 1/2: the image is x / 2, three bits
    lo = 0 if icpt else 1
    ed.assert_bits(H, G[lo:, lo:] / 4, "%s: H~ against X'X / 4" % (what,))
    ed.assert_bits(g[None, :], g1[None, lo:], "%s: g against X'(y - 1/2)" % (what,))
    # loglik = -n log 2: n equal terms, each within an ulp or two of log 2, summed in some order
    assert abs(float(ll) + n * np.log(2.0)) <= (n + 4) * 2.0 ** -53 * n * np.log(2.0), what


@pytest.mark.parametrize("p,icpt,n", ed.WIDE_A_CASES)
def test_tier_a_uniform_weight_bit_exact(eng, p, icpt, n):
    X, y, G, g1 = tier_a_rows(p, n)
    check_tier_a(eng, X, y, G, g1, icpt, (p, icpt, n))


@pytest.mark.parametrize("p", ed.WIDE_A_VIEW_WIDTHS)
@pytest.mark.parametrize("view", ["strided", "odd pitch", "nan pitch"])
def test_tier_a_views_bit_exact(eng, p, view):
    """partition_id = i % 3 views (the other rows are NaN), an odd row pitch (rows at odd multiples of 8 bytes: the scalar-load
    form) and an even one, NaN beyond column p: eight rows per wave (p = 128) and four (p = 200)"""
    n = ed.WIDE_A_VIEW_ROWS
    X, y, G, g1 = tier_a_rows(p, n)
    if view == "strided":
        buf = torch.full((3 * n, p), float("nan"), dtype=torch.float64, device="cuda")
        buf[1::3] = X
        V = buf[1::3]
        assert V.stride(0) == 3 * p
    else:
        ld = p + (3 if view == "odd pitch" else 6)
        buf = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :p] = X
        V = buf[:, :p]
        assert V.stride(0) % 2 == (1 if view == "odd pitch" else 0)
    for icpt in (False, True):
        check_tier_a(eng, V, y, G, g1, icpt, (p, view, icpt))


@pytest.mark.parametrize("p", ed.WIDE_B_WIDTHS)
def test_tier_b_probe_design_bit_exact(eng, p):
    n = ed.WIDE_B_ROWS
    chunks = ed.probe_chunks(n, p)
    X, beta = ed.probe_design(n, p, chunks, 7)
    y = (np.random.default_rng(p).random(n) < 0.5).astype(np.float64)
    H, g, ll, w = eng.newton_wide_pass(dev(X), dev(y), dev(beta), want_w=True)
    wh = w.cpu().numpy()
    rows = ed.probe_rows(n, chunks)
    assert np.max(np.abs(wh[rows] - ed.logistic_weights(X, beta)[rows])) < 1e-14 and wh[rows].min() < 0.02
    ed.assert_bits(H, ed.probe_reference(X, wh), "probe design p=%d" % p)


@pytest.mark.parametrize("p,icpt", ed.WIDE_C_CASES)
def test_tier_c_gaussian_rows_within_the_accumulation_bound(eng, p, icpt):
    n, pe = ed.WIDE_C_ROWS, p + icpt
    X, y, beta = ed.gaussian_design(n, p, 21, icpt)
    H, g, ll, w = eng.newton_wide_pass(dev(X), dev(y), dev(beta), fit_intercept=icpt, want_w=True)
    wh = w.cpu().numpy()
    assert np.max(np.abs(wh - ed.logistic_weights(X, beta, icpt))) < 1e-14
    S, Href, A = ed.bf16_image(X, wh, icpt)
    Hn = H.cpu().numpy()
    frac = ed.within(Hn, Href, ed.wide_bound(n, pe, A))
    print("tier C p=%d icpt=%d m=%d: worst fraction of the bound %.4f (diagonal %.4f)"
          % (p, icpt, ed.wide_rows_per_accumulator(n, pe), float(frac.max()), float(np.diag(frac).max())))
    worst = ed.assert_within(Hn, Href, ed.wide_bound(n, pe, A), "tier C p=%d icpt=%d" % (p, icpt))
    assert worst > 0.0                                       # (fp32 sums of 2000 chunks do round: 0 would mean nothing was compared)
    assert np.array_equal(Hn, Hn.T)
