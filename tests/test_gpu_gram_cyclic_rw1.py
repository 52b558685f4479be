"""GPU: the four-waves-per-SIMD shape of the cyclic Gram kernel (gram_cyclic.hip, one tile row per wave) against its two-wave twin
(gram_variant bit 16: gram_cyclic_rw2_kernel, the same tiles in the same k-step order, so the same bits) and against the pinned
oracle, at the kernel's floor of rows and one row above it.

n = 65 536: 64 slabs of 1024 rows = 128 chunks.  n = 65 537: rows_per_slab = 1032 = 129 chunks, not a multiple of the four stages;
the last slab has 521 rows, its last chunk holds one row and zero-filled chunks follow.

Every case is launched once (default, default again, variant 16, accumulate) and the tests below read those results."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_gram_plan import _against_oracle, _oracle_case      # noqa: E402  (the 1e-12 bounds of the neighbouring file)

WIDTHS = [(481, 0), (496, 0), (497, 1), (500, 1), (502, 2), (505, 3), (508, 3)]        # p -> tail groups G
ROWS = [65536, 65537]
CASES = [(p, G, n, weighted) for p, G in WIDTHS for n in ROWS for weighted in (True, False)]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _launches(p, n, weighted):
    from dlsa_amd import engine as eng
    X, wd, ref, d = _oracle_case(eng, n, p, 3000 + p + (n & 1), weighted, nan_pitch=(p % 2 == 0))
    H = eng.gram(X, wd)
    name = eng.gram_last_kernel()[0]
    again = eng.gram(X, wd)
    with eng.kernel_options(gram_variant=16):
        twin = eng.gram(X, wd)
        twin_name = eng.gram_last_kernel()[0]
    acc = eng.gram(X, wd, out=H.clone(), accumulate=True)
    return dict(H=H.cpu(), name=name, again=again.cpu(), twin=twin.cpu(), twin_name=twin_name, acc=acc.cpu(), ref=ref, d=d)


@pytest.mark.parametrize("p,G,n,weighted", CASES)
def test_four_wave_shape_has_the_bits_of_the_two_wave_twin(eng, p, G, n, weighted):
    r = _launches(p, n, weighted)
    hw = "true" if weighted else "false"
    assert r["name"] == "gram_cyclic_kernel<%s,%d>" % (hw, G), r["name"]
    assert r["twin_name"] == "gram_cyclic_rw2_kernel<%s,%d>" % (hw, G), r["twin_name"]
    assert not torch.isnan(r["H"]).any()
    assert torch.equal(r["H"], r["twin"])


@pytest.mark.parametrize("p,G,n,weighted", CASES)
def test_four_wave_shape_matches_oracle(eng, p, G, n, weighted):
    r = _launches(p, n, weighted)
    _against_oracle(r["H"], r["ref"], r["d"], (p, n, weighted))                         # exact symmetry + the two 1e-12 bounds
    _against_oracle(r["acc"] * 0.5, r["ref"], r["d"], (p, n, weighted, "accumulate"))


@pytest.mark.parametrize("p,G,n,weighted", CASES)
def test_two_launches_give_the_same_bits(eng, p, G, n, weighted):
    r = _launches(p, n, weighted)
    assert torch.equal(r["H"], r["again"])


@pytest.mark.parametrize("p", [497, 500])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("weighted", [True, False])
def test_corner_block_of_tile_row_31(eng, p, n, weighted):
    """H[496:, 496:] comes from the tail MFMAs of the tile-row-31 wave alone (its 8 big MFMAs are dummies).  H is positive
    semidefinite, so |H_ij| <= sqrt(H_ii H_jj) <= the block's largest entry: the entrywise 1e-12 bound of _against_oracle on the
    block's own scale."""
    r = _launches(p, n, weighted)
    Hc, refc = r["H"].numpy()[496:p, 496:p], r["ref"][496:p, 496:p]
    assert Hc.shape == (p - 496, p - 496) and np.all(np.diag(Hc) > 0)
    assert np.array_equal(Hc, Hc.T)
    assert np.max(np.abs(Hc - refc)) < 1e-12 * np.max(np.abs(refc))
    assert np.array_equal(Hc, r["twin"].numpy()[496:p, 496:p])
