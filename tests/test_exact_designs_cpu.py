"""tests/exact_designs.py against itself: its references are what it says they are, the preconditions of the exact claims hold at
every shape of tests/test_gpu_wide_exact.py and tests/test_gpu_gram_exact.py, and -- the point of those files -- every structural
mutant of a reference is REJECTED at every one of those shapes:

    one row dropped, one row doubled, one 16-row chunk dropped, two rows of a batch swapping weights, one off-diagonal 32 x 32
    tile transposed, columns shifted by one, the intercept column left last.

assert_bits must fail for every mutant on the integer designs and on the probe design (the weight swap needs per-row weights, the
intercept mutant an intercept: nothing else is left out); assert_within with the tier-C bound (exact_designs.wide_bound: nothing
measured) must fail for every mutant on the Gaussian cases.  The present tolerance of tests/test_gpu_wide.py (2e-3 of the
diagonal scale) passes the first four.

No GPU, no library."""
import numpy as np
import pytest

import exact_designs as ed


def rejected_bits(H, ref):
    try:
        ed.assert_bits(H, ref, "mutant")
    except AssertionError:
        return True
    return False


def rejected_within(H, ref, bound):
    try:
        ed.assert_within(H, ref, bound, "mutant")
    except AssertionError:
        return True
    return False


def wsum(R, w=None):
    return ed.gram_reference(R, w)


def mutants(H, R, w, r, chunk, icpt=False, swap=None):
    """{name: mutated H} of H = R' diag(w) R: row r, the 16-row chunk `chunk`; swap = (a, b, rows a and b as they stand in R
    with each other's weight [2, pe], their weights [2] or None) or None"""
    one = lambda rows, ww: wsum(R[rows], None if ww is None else ww[rows])
    out = {}
    out["row dropped"] = H - one(slice(r, r + 1), w)
    out["row doubled"] = H + one(slice(r, r + 1), w)
    out["chunk dropped"] = H - one(slice(16 * chunk, 16 * chunk + 16), w)
    if swap is not None:
        a, b, new, wnew = swap
        assert a // 8 == b // 8, "the two rows share a batch"
        out["weights swapped"] = H - one([a, b], w) + wsum(new, wnew)
    t = H.copy()
    t[0:32, 32:64] = H[0:32, 32:64].T
    t[32:64, 0:32] = t[0:32, 32:64].T
    out["tile transposed"] = t
    out["columns shifted"] = np.roll(H, 1, axis=(0, 1))
    if icpt:
        out["intercept last"] = np.roll(H, -1, axis=(0, 1))
    return out


def integer_swap(X, w, first):
    """two rows of the batch of 8 at `first` with different weights: w_b x_a x_a' + w_a x_b x_b'"""
    rows = np.arange(first, first + 8)
    a = rows[0]
    b = rows[np.flatnonzero(w[rows] != w[a])[0]]
    return a, b, X[[a, b]], w[[b, a]]


# ------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True])
def test_blas_reference_equals_an_integer_matmul(weights):
    X, w, H0 = ed.integer_design(4000, 300, 1, weights)
    Xi = X.astype(np.int64)
    Hi = Xi.T @ (Xi if w is None else Xi * (4 * w).astype(np.int64)[:, None])
    ed.assert_bits(ed.gram_reference(X, w) * (4 if weights else 1), Hi.astype(np.float64), "fp64 BLAS against int64")
    assert set(np.unique(X)) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert w is None or set(np.unique(w)) == {0.25, 0.5, 1.0}
    assert np.array_equal(H0, np.round(H0)) and not np.array_equal(H0, H0.T)
    # distinct columns, and no transposition of column blocks leaves X'X alone
    H = ed.gram_reference(X, w)
    assert len({tuple(c) for c in X.T}) == X.shape[1]
    assert not np.array_equal(H[0:32, 32:64], H[0:32, 32:64].T) and not np.array_equal(H, np.roll(H, 1, axis=(0, 1)))


def test_integer_design_refuses_rows_that_overflow_fp32():
    with pytest.raises(AssertionError):
        ed.integer_design(2 ** 24 // 36 + 1, 2, 0)
    biggest = max(n for n, _ in ed.GRAM_F32_PANEL + ed.GRAM_F32_WIDE + ed.GRAM_ACC64 + ed.GRAM_F64 + [ed.GRAM_F32_PANEL_FORCED])
    assert 36 * max(biggest, max(n for _, _, n in ed.WIDE_A_CASES)) < 2 ** 24


def test_bf16_rounding_two_ways():
    rng = np.random.default_rng(5)
    f = np.concatenate([rng.standard_normal(100000) * 10.0 ** rng.integers(-6, 6, 100000), [0.0, 1.0, 1.00390625, 1.01171875, 0.5, -3.0]]).astype(np.float32)
    assert np.array_equal(ed.bf16_round(f), ed.bf16_round_bits(f))
    assert ed.bf16_round(np.float32([1.00390625]))[0] == 1.0 and ed.bf16_round(np.float32([1.01171875]))[0] == 1.015625     # ties to even, both ways


def test_wide_geometry_tables():
    assert [ed.wide_groups(pe) for pe in (121, 256, 257, 512)] == [256, 256, 128, 128]
    assert [ed.wide_ring_stages(pe) for pe in (128, 129, 256, 257, 384, 385, 512)] == [16, 16, 16, 13, 13, 10, 10]
    assert sorted({ed.wide_nb(p + i) for p, i in ed.WIDE_A_WIDTHS}) == list(range(4, 17))
    for p, icpt, n in ed.WIDE_A_CASES:
        assert n >= 32768 and 121 <= p + icpt <= 512
    for p, icpt in ed.WIDE_A_WIDTHS:
        rows = ed.wide_a_rows(p + icpt)
        assert ((rows[1] + 15) // 16) % 2 == 1 and rows[2] % 16 == 7 and rows[3] % 16 == 15
        assert (rows[4] + 15) // 16 > ed.wide_groups(p + icpt) * (ed.wide_ring_stages(p + icpt) + 2)


def test_image_model_on_a_hand_made_case():
    X = np.array([[1.0, 3.0], [2.0, -1.0], [1.0 + 2.0 ** -10, 0.1]])
    w = np.array([0.25, 0.0625, 0.2])
    S, H, A = ed.bf16_image(X, w, intercept=True)
    assert S.shape == (16, 3) and not S[3:].any()
    assert np.array_equal(S[:2], [[0.5, 0.5, 1.5], [0.25, 0.5, -0.25]])
    s2 = np.sqrt(np.float32(0.2))
    assert S[2, 0] == ed.bf16_round_bits(np.float32([s2]))[0]
    assert S[2, 1] == ed.bf16_round_bits(np.float32([np.float32(1.0 + 2.0 ** -10) * s2]))[0]
    assert np.array_equal(H, S.T @ S) and np.array_equal(A, np.abs(S).T @ np.abs(S))


# ------------------------------------------------------------------------------------------------------------------------------
# tier B: the probe design's preconditions, and its mutants
# ------------------------------------------------------------------------------------------------------------------------------
def probe_case(p):
    n = ed.WIDE_B_ROWS
    chunks = ed.probe_chunks(n, p)
    X, beta = ed.probe_design(n, p, chunks, 7)
    w = ed.logistic_weights(X, beta)
    return n, chunks, X, beta, w


@pytest.mark.parametrize("p", ed.WIDE_B_WIDTHS)
def test_probe_design_preconditions(p):
    n, chunks, X, beta, w = probe_case(p)
    nchunks = (n + 15) // 16
    assert {0, 1, nchunks - 2, nchunks - 1} <= set(chunks) and n % 16 != 0
    g = ed.wide_groups(p)
    assert len({c % g for c in chunks}) == len(chunks)                       # one probe chunk per fp32 accumulator
    rows = ed.probe_rows(n, chunks)
    assert np.array_equal(np.flatnonzero(np.any(X != 0, axis=1)), rows)
    eta = X[rows] @ beta
    assert eta.min() < -3.0 and eta.max() > 3.0 and np.max(np.abs(eta)) <= 6.0 + 1e-9
    assert w[rows].min() > 2.4e-3 and w[rows].min() < 0.02 and w[rows].max() > 0.2       # far from fp32 denormals
    mant, _ = np.frexp(X[X != 0])
    assert np.all(np.abs(mant) == 0.5) and np.abs(X).max() == 4.0 and np.abs(X[X != 0]).min() == 0.25
    # row i of a chunk owns the columns i mod 16: one non-zero product per MFMA and entry
    rr, cc = np.nonzero(X)
    assert np.all(rr % 16 == cc % 16) and np.count_nonzero(X) == sum(np.count_nonzero(np.arange(p) % 16 == r % 16) for r in rows)
    # a power of two commutes with both roundings: the image is x * bf16(sqrtf(float(w)))
    S, H, A = ed.bf16_image(X, w)
    b = ed.bf16_round(np.sqrt(w.astype(np.float32)))
    assert np.array_equal(S[:n], X * b[:, None])
    # every product fits fp32; the sum over the groups is exact in fp64: in units of 2^-28 everything is an integer below 2^53
    Href = ed.probe_reference(X, w)
    ed.assert_bits(Href, H, "probe formula against S'S")
    T = (S[:n][rows] * 2.0 ** 14)
    assert np.array_equal(T, np.round(T))
    Ti = T.astype(np.int64)
    ed.assert_bits(Href * 2.0 ** 28, (Ti.T @ Ti).astype(np.float64), "probe reference against integers")
    prod = (S[:n][rows][:, :, None] * S[:n][rows][:, None, :])
    assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)
    # zeros exactly where no row owns both columns
    same = (np.arange(p)[:, None] % 16) == (np.arange(p)[None, :] % 16)
    assert not Href[~same].any() and np.all(Href[same] != 0)


@pytest.mark.parametrize("p", ed.WIDE_B_WIDTHS)
def test_probe_design_rejects_every_mutant(p):
    n, chunks, X, beta, w = probe_case(p)
    S, H, A = ed.bf16_image(X, w)
    first = 16 * chunks[2]
    batch = np.arange(first, first + 8)
    a = batch[0]
    b = batch[np.argmax(np.abs(w[batch] - w[a]))]
    sw = w.copy(); sw[[a, b]] = w[[b, a]]
    new = ed.bf16_image(X[[a, b]], sw[[a, b]])[0][:2]
    m = mutants(H, S, None, 16 * chunks[3] + 5, chunks[-1], swap=(a, b, new, None))
    assert set(m) == {"row dropped", "row doubled", "chunk dropped", "weights swapped", "tile transposed", "columns shifted"}
    ed.assert_bits(H, ed.probe_reference(X, w), "the reference itself")
    for name, Hm in m.items():
        assert rejected_bits(Hm, H), (p, name)


# ------------------------------------------------------------------------------------------------------------------------------
# tier A and the Gram designs: mutants against assert_bits
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,icpt,n", ed.WIDE_A_CASES)
def test_uniform_weight_design_rejects_every_mutant(p, icpt, n):
    """(uniform weight: two rows swapping weights change nothing -- tier B has that mutant)"""
    X = ed.wide_a_design(p, n)
    R = ed.with_ones(X) if icpt else X
    w = np.full(n, 0.25)
    H = wsum(R, w)
    ed.assert_bits(H, wsum(R) / 4, "X'X / 4")
    m = mutants(H, R, w, n // 3, (n + 15) // 16 - 1, icpt=icpt)               # (the last chunk: the ragged one where there is one)
    assert len(m) == 5 + icpt
    for name, Hm in m.items():
        assert rejected_bits(Hm, H), (p, icpt, n, name)


GRAM_SHAPES = sorted(set(ed.GRAM_F32_PANEL + [ed.GRAM_F32_PANEL_FORCED] + ed.GRAM_F32_WIDE + ed.GRAM_ACC64 + ed.GRAM_F64))


@pytest.mark.parametrize("n,p", GRAM_SHAPES)
def test_integer_design_rejects_every_mutant(n, p):
    X, w, H0 = ed.integer_design(n, p, 11, weights=True)
    H = wsum(X, w)
    m = mutants(H, X, w, n // 3, (n + 15) // 16 - 1, swap=integer_swap(X, w, 8 * (n // 24)))
    assert len(m) == 6
    for name, Hm in m.items():
        assert rejected_bits(Hm, H), (n, p, name)
        assert rejected_bits(Hm + H0, H + H0), (n, p, name, "accumulate")
    # unweighted: the same, less the swap
    H1 = wsum(X)
    for name, Hm in mutants(H1, X, None, n // 3, (n + 15) // 16 - 1).items():
        assert rejected_bits(Hm, H1), (n, p, name, "unweighted")


# ------------------------------------------------------------------------------------------------------------------------------
# tier C: mutants against the derived bound
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,icpt", ed.WIDE_C_CASES)
def test_gaussian_image_rejects_every_mutant_within_the_bound(p, icpt):
    n, pe = ed.WIDE_C_ROWS, p + icpt
    X, y, beta = ed.gaussian_design(n, p, 21, icpt)
    w = ed.logistic_weights(X, beta, icpt)
    S, H, A = ed.bf16_image(X, w, icpt)
    bound = ed.wide_bound(n, pe, A)
    assert ed.assert_within(H, H, bound) == 0.0
    assert ed.assert_within(H + 0.5 * bound, H, bound) <= 1.0 and rejected_within(H + 1.01 * bound, H, bound)
    first = 8 * (n // 24)
    batch = np.arange(first, first + 8)
    a = batch[0]
    b = batch[np.argmax(np.abs(w[batch] - w[a]))]
    sw = w.copy(); sw[[a, b]] = w[[b, a]]
    new = ed.bf16_image(X[[a, b]], sw[[a, b]], icpt)[0][:2]
    m = mutants(H, S, None, n // 3, (n + 15) // 16 - 1, icpt=icpt, swap=(a, b, new, None))
    assert len(m) == 6 + icpt
    for name, Hm in m.items():
        frac = float(ed.within(Hm, H, bound).max())
        print("mutant p=%d icpt=%d %s: %.2f x the bound" % (p, icpt, name, frac))
        assert rejected_within(Hm, H, bound), (p, icpt, name, frac)
    # ... and the plain rounding of the image stays far inside the tolerance these tests replace, while the first four mutants pass it
    d = np.sqrt(np.diag(H))
    for name in ("row dropped", "row doubled", "chunk dropped", "weights swapped"):
        assert np.max(np.abs(m[name] - H) / np.outer(d, d)) < 2e-3, name
