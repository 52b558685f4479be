"""GPU: the fp32 Gram kernels -- the panel kernel of csrc/gram.hip with T = float, csrc/gram_wide.hip, the fp64-summed
dlsa_gram_f32_acc64 -- and dlsa_xtv_stats_f32 on integer designs (tests/exact_designs.py: rows from {+-1, +-2, +-3}, weights from
{1/4, 1/2, 1}), where every partial sum of X' diag(w) X is a multiple of 1/4 below 2^24 / 4: fp32 accumulators give the exact result
in ANY order, so every comparison here is bit for bit.  tests/test_gpu_kernels.py and tests/test_gpu_linear.py hold these kernels
to 2e-5 / 2e-6 of the largest entry, which one row missing from one tile passes (the mutants of tests/test_exact_designs_cpu.py).
The fp64 kernels run the same designs, one width per kernel: exact tile coverage where a 1e-12 norm is all the other files assert.

References: an fp64 matmul on the device (rocBLAS: none of the code under test; exact in any order, and checked against an int64
matmul in the CPU file)."""
import functools

import numpy as np
import pytest

import exact_designs as ed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PANEL, WIDE = "gram_kernel<float,", "gram_wide_f32_kernel<"


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=1)
def design(n, p):
    """the integer design on the device in fp64: X, w, H0, X'wX, X'X"""
    X, w, H0 = (dev(a) for a in ed.integer_design(n, p, 11, weights=True))
    return X, w, H0, ed.gram_reference(X, w), ed.gram_reference(X)


def nan_pitch(X, pad):
    buf = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), dtype=X.dtype, device=X.device)
    buf[:, :X.shape[1]] = X
    return buf[:, :X.shape[1]]


def check_gram(eng, n, p, dtype, kernel, pad=0):
    """weighted, unweighted, accumulated into H0 (the kernel's name asserted each time); pad: a row pitch of p + pad, NaN beyond p"""
    X64, w64, H0, refw, ref1 = design(n, p)
    X, w = X64.to(dtype), w64.to(dtype)
    if pad:
        X = nan_pitch(X, pad)
    for wt, ref, tag in ((w, refw, "weighted"), (None, ref1, "unweighted")):
        H = eng.gram(X, wt)
        name = eng.gram_last_kernel()[0]
        assert kernel is None or name.startswith(kernel), (n, p, name)
        assert H.dtype == dtype
        ed.assert_bits(H.double(), ref, "%s n=%d p=%d pad=%d %s" % (name, n, p, pad, tag))
        out = H0.to(dtype, copy=True)
        eng.gram(X, wt, out=out, accumulate=True)
        assert kernel is None or eng.gram_last_kernel()[0].startswith(kernel)
        ed.assert_bits(out.double(), ref + H0, "%s n=%d p=%d pad=%d %s, accumulated" % (name, n, p, pad, tag))
    return name


@pytest.mark.parametrize("n,p", ed.GRAM_F32_PANEL)
def test_f32_panel_kernel_bit_exact(eng, n, p):
    check_gram(eng, n, p, torch.float32, PANEL)


def test_f32_panel_kernel_bit_exact_where_the_wide_kernel_would_run(eng):
    n, p = ed.GRAM_F32_PANEL_FORCED
    with eng.kernel_options(gram_wide_f32=False):
        check_gram(eng, n, p, torch.float32, PANEL)


def test_f32_panel_kernel_bit_exact_in_a_nan_padded_pitch(eng):
    check_gram(eng, 2000, 500, torch.float32, PANEL, pad=3)
    check_gram(eng, 3001, 100, torch.float32, PANEL, pad=4)


@pytest.mark.parametrize("n,p", ed.GRAM_F32_WIDE)
def test_f32_wide_kernel_bit_exact(eng, n, p):
    """a ragged last 16-row stage (16391, 20011, 70001), a ragged last 64-column group (772, 1000, 2052, 1028), the quarter unit"""
    check_gram(eng, n, p, torch.float32, WIDE)


def test_f32_wide_kernel_bit_exact_in_a_nan_padded_pitch(eng):
    check_gram(eng, 16391, 772, torch.float32, WIDE, pad=4)


@pytest.mark.parametrize("n,p", ed.GRAM_ACC64)
def test_f32_rows_fp64_sums_bit_exact(eng, n, p):
    X64, w64, H0, refw, ref1 = design(n, p)
    X, w = X64.float(), w64.float()
    for wt, ref in ((w, refw), (None, ref1)):
        H = eng.gram_acc64(X, wt)
        assert H.dtype == torch.float64
        ed.assert_bits(H, ref, "gram_acc64 n=%d p=%d" % (n, p))
        # two ragged halves accumulated into a sub-block view of a bigger matrix that holds H0; the border stays exactly 0
        big = torch.zeros((p + 1, p + 1), dtype=torch.float64, device="cuda")
        big[1:, 1:] = H0
        cut = n // 2 + 3
        eng.gram_acc64(X[:cut], None if wt is None else wt[:cut].contiguous(), out=big[1:, 1:], accumulate=True)
        eng.gram_acc64(X[cut:], None if wt is None else wt[cut:].contiguous(), out=big[1:, 1:], accumulate=True)
        ed.assert_bits(big[1:, 1:], ref + H0, "gram_acc64 n=%d p=%d, two halves into a view" % (n, p))
        assert not bool(big[0].any()) and not bool(big[:, 0].any())
        fresh = torch.full((p + 1, p + 1), float("nan"), dtype=torch.float64, device="cuda")
        eng.gram_acc64(X, wt, out=fresh[1:, 1:])
        ed.assert_bits(fresh[1:, 1:], ref, "gram_acc64 n=%d p=%d, stored over NaN" % (n, p))
        assert bool(fresh[0].isnan().all()) and bool(fresh[:, 0].isnan().all())


@pytest.mark.parametrize("n,p", [(20001, 999), (30011, 2000), (5000, 37), (3, 256)])
def test_xtv_stats_f32_rows_bit_exact(eng, n, p):
    """g = X'v, the column sums and [v'v, sum v] of fp32 rows with an integer v: fp64 sums of small integers, exact in any order"""
    X64, w64, H0, refw, ref1 = design(n, p)
    X = X64.float()
    v64 = dev(np.random.default_rng(n + p).integers(-4, 5, size=n).astype(np.float64))
    v = v64.float()
    g, cs, st = eng.xtv_stats(X, v, want_colsum=True)
    ed.assert_bits(g[None], (X64.T @ v64)[None], "xtv_stats g n=%d p=%d" % (n, p))
    ed.assert_bits(cs[None], X64.sum(0)[None], "xtv_stats column sums n=%d p=%d" % (n, p))
    ed.assert_bits(st[None], torch.stack([v64 @ v64, v64.sum()])[None], "xtv_stats stats n=%d p=%d" % (n, p))
    cut = n // 3
    g2, _, st2 = eng.xtv_stats(X[:cut], v[:cut].contiguous())
    eng.xtv_stats(X[cut:], v[cut:].contiguous(), g=g2, stats=st2, accumulate=True)
    assert torch.equal(g2, g) and torch.equal(st2, st)


@pytest.mark.parametrize("n,p", ed.GRAM_F64)
def test_f64_kernels_bit_exact(eng, n, p):
    """the row-split kernel (p = 100), the plan kernel (260, 572) and the cyclic kernel (500) at the row count that selects them,
    and whatever serves the width at 8209 rows"""
    name = check_gram(eng, n, p, torch.float64, ed.GRAM_F64_KERNEL[p] if n >= 65536 or p == 100 else None)
    print("fp64 n=%d p=%d: %s" % (n, p, name))
    check_gram(eng, n, p, torch.float64, None, pad=2)
