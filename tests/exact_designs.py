"""Designs whose Gram matrices the reduced-precision kernels must reproduce BIT FOR BIT, the host model of the bf16 image for the
designs where that is impossible, and the two comparators -- shared by tests/test_gpu_wide_exact.py, tests/test_gpu_gram_exact.py
and tests/test_exact_designs_cpu.py (which checks this file against itself: every mutant of a reference must be rejected).

  * integer_design: rows from {+-1, +-2, +-3}, weights from {1/4, 1/2, 1}.  Every product and every partial sum of X' diag(w) X is
    a multiple of 1/4 below 2^24 / 4, so fp32 and fp64 accumulators give the same bits in ANY summation order; so does the bf16
    image of the wide Newton pass at beta = 0 (w = 1/4, sqrt(w) = 1/2, and x / 2 has three significant bits).
  * probe_design: per-row weights through the bf16 image, exactly.  Rows are zero except in a few 16-row chunks; there row i of the
    chunk owns the columns j = i mod 16 with entries +-2^e.  A power of two commutes with both roundings of the image
    (bf16(float(x) * s) = x * bf16(s)), every MFMA sees ONE non-zero product per entry, every fp32 accumulator one non-zero chunk
    (the probe chunks are distinct modulo both group counts), and the fp64 sum over the groups adds a handful of 16-bit values
    whose exponents span far less than 53 bits.
  * bf16_image: s = sqrtf(float(w)), f = float(x) * s in fp32, round to nearest even to bf16 (csrc/logit.hip, logit_image), the
    intercept's ones column (s itself) FIRST as wide_reduce_kernel stores it.  H = S'S in fp64 is what the kernel would give with
    exact accumulation; A = |S|'|S| scales the bound on its fp32 sums (wide_bound).

Plain numpy / torch on the host; no GPU, no library."""
import numpy as np
import torch

TILE = 32


# ------------------------------------------------------------------------------------------------------------------------------
# the wide pass's geometry (csrc/irls_wide.hip): column blocks of 32, one fp32 accumulator set per GROUP of workgroups, chunk c of
# 16 rows goes to group c mod groups
# ------------------------------------------------------------------------------------------------------------------------------
def wide_nb(pe):
    return (pe + 31) // 32


def wide_groups(pe):
    """256 workgroups, one per group up to 8 column blocks (4 waves own the triangle), two per group beyond"""
    return 256 if (wide_nb(pe) + 1) // 2 <= 4 else 128


def wide_ring_stages(pe):
    """LDS ring stages of wide_syrk_kernel: 160 KiB of 4 * ceil(NB / 4) KiB stages, 16 at the most"""
    return min(16, 160 // (4 * ((wide_nb(pe) + 3) // 4)))


def wide_rows_per_accumulator(n, pe):
    nchunks = (n + 15) // 16
    g = wide_groups(pe)
    return 16 * ((nchunks + g - 1) // g)


def wide_bound(n, pe, A):
    """Per-entry bound on H~ - S'S: an fp32 accumulator adds m = 16 ceil(nchunks / groups) exact products (bf16 x bf16 has 16
    bits), each add rounds -- or truncates, hence 2^-23 and not 2^-24 -- a partial sum that is at most A[i][j] in size; the fp64
    sum over the groups costs 2^-53 a term, nothing on this scale."""
    return wide_rows_per_accumulator(n, pe) * 2.0 ** -23 * A


# ------------------------------------------------------------------------------------------------------------------------------
# designs
# ------------------------------------------------------------------------------------------------------------------------------
def integer_design(n, p, seed, weights=False):
    """(X [n, p] fp64 from {+-1, +-2, +-3}, w [n] from {1/4, 1/2, 1} or None, H0 [p, p] small integers to accumulate into).
    36 n < 2^24: X'wX in units of 1/4 stays below 2^24, so an fp32 accumulator holds every partial sum exactly."""
    assert 36 * n < 2 ** 24, "integer_design: %d rows overflow an fp32 accumulator" % n
    rng = np.random.default_rng([seed, n, p])
    X = rng.integers(1, 4, size=(n, p)).astype(np.float64)
    X *= rng.integers(0, 2, size=(n, p)) * 2.0 - 1.0
    w = 0.25 * 2.0 ** rng.integers(0, 3, size=n) if weights else None
    H0 = rng.integers(-9, 10, size=(p, p)).astype(np.float64)
    return X, w, H0


def gram_reference(X, w=None):
    """X' diag(w) X in fp64 (numpy arrays or torch tensors, host or device): exact on integer_design in any order"""
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64))
        w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)) if w is not None else None
        return (X.T @ (X if w is None else w[:, None] * X)).numpy()
    X = X.double()
    return X.T @ (X if w is None else w.double()[:, None] * X)


def with_ones(X):
    return np.hstack([np.ones((X.shape[0], 1)), X])


def probe_chunks(n, pe):
    """chunk 0, chunk 1, two in the middle, the last full chunk and the ragged last one; pairwise distinct modulo 128 and 256"""
    nchunks = (n + 15) // 16
    assert n % 16, "probe_chunks: the last chunk should be ragged"
    return [0, 1, 300 + wide_nb(pe), 1100 + 3 * wide_nb(pe), nchunks - 2, nchunks - 1]


def probe_design(n, p, chunks, seed):
    """(X [n, p], beta [p]): zero rows except in the listed 16-row chunks, where row i owns the columns j = i mod 16 with
    x = +-2^e, e in -2 .. 2.  beta is scaled so that the probe rows' eta reaches +-6: w from 1/4 down to 2.5e-3."""
    nchunks = (n + 15) // 16
    assert len(chunks) == len(set(chunks)) and all(0 <= c < nchunks for c in chunks)
    for mod in (128, 256):
        assert len(set(c % mod for c in chunks)) == len(chunks), "probe chunks collide modulo %d groups" % mod
    rng = np.random.default_rng([seed, n, p])
    X = np.zeros((n, p))
    cols = np.arange(p)
    for c in chunks:
        for i in range(16):
            r = 16 * c + i
            if r >= n:
                break
            own = cols[cols % 16 == i]
            X[r, own] = 2.0 ** rng.integers(-2, 3, size=own.size) * (rng.integers(0, 2, size=own.size) * 2.0 - 1.0)
    beta = rng.standard_normal(p)
    eta = X @ beta
    beta *= 6.0 / np.max(np.abs(eta))
    return X, beta


def probe_rows(n, chunks):
    return np.array([16 * c + i for c in chunks for i in range(16) if 16 * c + i < n])


def bf16_round(f32):
    """float32 -> bf16 (round to nearest even) -> float64"""
    return torch.from_numpy(np.ascontiguousarray(f32, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def bf16_round_bits(f32):
    """the same on the uint32 view: add 0x7fff + the lowest kept bit, drop 16 bits (finite values only)"""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def probe_reference(X, w):
    """H~ of a probe design from the device's own w: sum over the probe rows of b_r^2 x_ri x_rj, b_r = bf16(sqrtf(float(w_r)));
    exact in fp64 (16-bit values times powers of two, a few per entry), exactly 0 where no row owns both columns."""
    p = X.shape[1]
    H = np.zeros((p, p))
    b = bf16_round(np.sqrt(np.asarray(w, dtype=np.float64).astype(np.float32)))
    for r in np.flatnonzero(np.any(X != 0, axis=1)):
        own = np.flatnonzero(X[r])
        H[np.ix_(own, own)] += (b[r] * b[r]) * np.outer(X[r, own], X[r, own])
    return H


def bf16_image(X, w, intercept=False):
    """Host model of logit_image: (S [16 ceil(n / 16), pe] as fp64, H = S'S, A = |S|'|S|); rows past n are zero, the ones column
    (s itself) first."""
    n, p = X.shape
    s = np.sqrt(np.asarray(w, dtype=np.float64).astype(np.float32))                     # correctly rounded, as sqrtf
    assert s.dtype == np.float32
    f = X.astype(np.float32) * s[:, None]                                              # one fp32 multiply
    assert f.dtype == np.float32
    S = np.zeros(((n + 15) // 16 * 16, p + (1 if intercept else 0)))
    if intercept:
        S[:n, 0] = bf16_round(s)
    S[:n, (1 if intercept else 0):] = bf16_round(f)
    St = torch.from_numpy(S)
    return S, (St.T @ St).numpy(), (St.abs().T @ St.abs()).numpy()


def gaussian_design(n, p, seed, intercept=False):
    """(X, y, beta [p + intercept], intercept first): Gaussian rows, eta ~ N(0.25, 1.5^2)"""
    rng = np.random.default_rng([seed, n, p])
    X = rng.standard_normal((n, p))
    beta = rng.standard_normal(p) * (1.5 / np.sqrt(p))
    y = (rng.random(n) < 0.5).astype(np.float64)
    if intercept:
        beta = np.concatenate([[0.25], beta])
    return X, y, beta


def logistic_weights(X, beta, intercept=False):
    """w = mu (1 - mu) on the host (fp64): what the CPU tests build the image from; the GPU tests take the device's own w"""
    eta = X @ (beta[1:] if intercept else beta) + (beta[0] if intercept else 0.0)
    e = np.exp(-np.abs(eta))
    return e / (1.0 + e) ** 2


# ------------------------------------------------------------------------------------------------------------------------------
# the shapes of the GPU tests (the CPU file runs its mutants at every one of them)
# ------------------------------------------------------------------------------------------------------------------------------
# (p, intercept): every column-block count 4 .. 16 of the bf16 Gram kernel
WIDE_A_WIDTHS = [(121, False), (128, False), (128, True), (160, False), (192, False), (200, False), (256, False), (256, True),
                 (320, False), (351, False), (384, False), (400, False), (448, False), (480, False), (500, False), (511, True),
                 (512, False)]


def wide_a_rows(pe):
    """the minimum; an odd chunk count (some groups run an odd number of chunks through the two-per-trip loop); ragged tails of 7
    and 15 rows; and 19 chunks per group + 5 rows: more than ring stages + 2, so the LDS ring wraps"""
    wrap = 16 * wide_groups(pe) * 19 + 5
    assert 19 > wide_ring_stages(pe) + 2
    return [32768, 32769, 32768 + 16 * 3 + 7, 32768 + 16 * 130 + 15, wrap]


WIDE_A_CASES = [(p, icpt, n) for p, icpt in WIDE_A_WIDTHS for n in wide_a_rows(p + icpt)]
WIDE_A_VIEW_WIDTHS = [128, 200]                     # eight rows per wave, four rows per wave
WIDE_A_VIEW_ROWS = 32768 + 16 * 7 + 11
WIDE_B_WIDTHS = [121, 128, 200, 300, 512]
WIDE_B_ROWS = 32768 + 16 * 40 + 9
WIDE_C_CASES = [(p, icpt) for p in (128, 257, 500) for icpt in (False, True)]
WIDE_C_ROWS = 32768 + 9

GRAM_F32_PANEL = [(3001, 100), (2000, 500), (500, 1030), (20011, 1001), (16400, 770)]
GRAM_F32_PANEL_FORCED = (33000, 2000)
GRAM_F32_WIDE = [(16384, 768), (16391, 772), (20011, 1000), (16400, 2052), (70001, 1028)]
GRAM_ACC64 = [(40000, 1024), (9000, 300)]
GRAM_F64 = [(n, p) for p in (100, 260, 500, 572) for n in (8192 + 17, 65536 + 5)]
GRAM_F64_KERNEL = {100: "gram_narrow_kernel", 260: "gram_plan_kernel", 500: "gram_cyclic_kernel", 572: "gram_plan_kernel"}


def wide_a_design(p, n):
    """tier A design of width p, n rows: seed by width"""
    return integer_design(n, p, 4000 + p)[0]


# ------------------------------------------------------------------------------------------------------------------------------
# comparators
# ------------------------------------------------------------------------------------------------------------------------------
def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def assert_bits(H, ref, what=""):
    """H == ref entry for entry (NaN never equal; +0 == -0).  On failure: the first differing (row, column), its 32 x 32 tile and
    how much of it differs, and how many tiles differ at all."""
    H, ref = _host(H), _host(ref)
    assert H.shape == ref.shape, "%s: shape %s, expected %s" % (what, H.shape, ref.shape)
    bad = ~(H == ref)
    if not bad.any():
        return
    r, c = (int(v) for v in np.argwhere(bad)[0])
    I, J = r // TILE, c // TILE
    tile = bad[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE]
    nt = (bad.shape[0] + TILE - 1) // TILE, (bad.shape[1] + TILE - 1) // TILE
    tiles = sum(bool(bad[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE].any()) for a in range(nt[0]) for b in range(nt[1]))
    raise AssertionError("%s: %d of %d entries differ, in %d of %d tiles; first at (%d, %d): got %r, expected %r; its tile (%d, %d) "
                         "differs in %d of %d entries, rows %s, columns %s"
                         % (what, int(bad.sum()), bad.size, tiles, nt[0] * nt[1], r, c, H[r, c], ref[r, c], I, J, int(tile.sum()),
                            tile.size, _span(np.flatnonzero(tile.any(1)) + I * TILE), _span(np.flatnonzero(tile.any(0)) + J * TILE)))


def _span(idx):
    return "%d..%d (%d)" % (idx[0], idx[-1], idx.size)


def within(H, ref, bound):
    """worst |H - ref| / bound over the entries (inf where an entry with bound 0 differs, or is not finite)"""
    H, ref, bound = _host(H), _host(ref), _host(bound)
    assert H.shape == ref.shape == bound.shape
    err = np.abs(H - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / bound)
    frac[~np.isfinite(H)] = np.inf
    return frac


def assert_within(H, ref, bound, what=""):
    """|H - ref| <= bound entry by entry; returns the worst fraction of the bound"""
    frac = within(H, ref, bound)
    worst = float(frac.max())
    if not worst <= 1.0:
        r, c = (int(v) for v in np.unravel_index(int(np.argmax(frac)), frac.shape))
        raise AssertionError("%s: %d entries beyond their bound; worst at (%d, %d), tile (%d, %d): got %r, expected %r, bound %.3e "
                             "(%.2f x)" % (what, int((frac > 1.0).sum()), r, c, r // TILE, c // TILE, _host(H)[r, c],
                                           _host(ref)[r, c], _host(bound)[r, c], worst))
    return worst
