"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs, against the committed golden fixtures, and -- at BASELINE.json's full per-GPU
size -- through size-independent properties.  Run with `pytest -m gpu` on an MI355X."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import pytest

from golden_inputs import lars_case

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_KERNEL = 1e-12   # fp64 kernels vs numpy/BLAS on identical inputs (summation order only)
TOL_MLE = 1e-10      # north star: theta-hat within 1e-10 relative l_inf of the exact MLE


def rel_inf(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dlsa_amd import engine
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import dlsa_oracle
    return dlsa_oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------
def test_synth_rows_bit_identical_to_oracle(eng, orc):
    for (n, p, row0, ones) in [(257, 9, 0, False), (1000, 50, 12345678901, False), (64, 7, 5, True)]:
        X, y = eng.synth(20260101, row0, n, p, kind=eng.SYNTH_UNIFORM, ones_col=ones)
        Xo, yo = orc.synth_logistic(20260101, row0, n, p, orc.SYNTH_UNIFORM)
        Xg = X.cpu().numpy()
        if ones:
            assert np.all(Xg[:, 0] == 1.0)
            Xg = Xg[:, 1:]
        assert np.array_equal(Xg, Xo)                       # integer pipeline: bit exact
        # labels go through exp(): allow a label flip only where u is within 1e-12 of prob
        assert np.mean(y.cpu().numpy() != yo) < 1e-3
    G, _ = eng.synth(7, 0, 200000, 6, kind=eng.SYNTH_GAUSSIAN, labels=False)
    g = G.cpu().numpy()
    assert abs(g.std() - (1 / 12) ** 0.5) < 2e-3 and abs(g.mean()) < 2e-3


GRAM_CASES = [(1, 1), (15, 3), (1000, 5), (777, 17), (5000, 50), (4099, 100), (3000, 129),
              (2048, 250), (3001, 500), (1500, 513), (40000, 64), (700, 1000)]


@pytest.mark.parametrize("n,p", GRAM_CASES)
@pytest.mark.parametrize("weighted", [True, False])
def test_gram_matches_oracle(eng, orc, n, p, weighted):
    rng = np.random.default_rng(n * 1000 + p)
    X = rng.random((n, p)) - 0.5            # asymmetric operands: catches transposed C writes
    w = rng.random(n) * 0.25 if weighted else None
    H = eng.gram(dev(X), dev(w) if weighted else None).cpu().numpy()
    Ho = orc.gram(X, w)
    assert rel_inf(H, Ho) < TOL_KERNEL
    assert np.array_equal(H, H.T)           # both triangles written, exactly symmetric


def test_gram_strided_rows_and_accumulate(eng, orc):
    rng = np.random.default_rng(3)
    n, p, ld = 999, 37, 41                  # odd leading dimension -> unaligned (scalar-load) path
    buf = rng.random((n, ld)) - 0.5
    Xd = dev(buf)[:, :p]
    w = rng.random(n)
    H0 = rng.random((p, p))
    H = dev(H0.copy())
    eng.gram(Xd, dev(w), out=H, accumulate=True)
    assert rel_inf(H.cpu().numpy(), H0 + orc.gram(buf[:, :p], w)) < 1e-11


@pytest.mark.parametrize("n,p,ld", [(5000, 36, 40), (777, 500, 512), (20000, 130, 256), (33, 2, 6), (100000, 64, 64)])
def test_gram_dma_path_with_row_pitch(eng, orc, n, p, ld):
    """Even p and even leading dimension > p: the direct global->LDS DMA path with a row pitch that
    differs from p (buffer descriptor bounds, column masking, slab tails)."""
    rng = np.random.default_rng(n + p)
    buf = rng.random((n, ld)) - 0.5
    buf[:, p:] = np.nan                      # anything read beyond column p would poison the result
    Xd = dev(buf)[:, :p]
    w = rng.random(n) * 0.25
    H = eng.gram(Xd, dev(w)).cpu().numpy()
    assert np.all(np.isfinite(H))
    assert rel_inf(H, orc.gram(buf[:, :p], w)) < TOL_KERNEL
    H1 = eng.gram(Xd).cpu().numpy()
    assert rel_inf(H1, orc.gram(buf[:, :p])) < TOL_KERNEL


@pytest.mark.parametrize("n,p,ld", [(8192, 50, 50), (20001, 100, 100), (100003, 100, 104), (9000, 64, 70), (50000, 112, 112),
                                    (33333, 98, 128), (8200, 80, 80), (262144 + 17, 100, 100)])
def test_gram_narrow_row_split_kernel(eng, orc, n, p, ld):
    """49 <= p <= 112, even p, >= 8192 rows: the row-split kernel (every wave owns the whole triangle; LDS-DMA ring;
    partial triangles meet in LDS).  Ragged row counts, row pitch != p (NaN padding), weighted and unweighted,
    accumulate, and agreement with the tile-list kernel (dlsa_kernel_options.gram_variant = 64)."""
    rng = np.random.default_rng(n + p)
    buf = rng.random((n, ld)) - 0.5
    buf[:, p:] = np.nan
    Xd = dev(buf)[:, :p]
    w = rng.random(n) * 0.25
    Ho = orc.gram(buf[:, :p], w)
    H = eng.gram(Xd, dev(w))
    assert torch.equal(H, H.T)
    assert rel_inf(H.cpu().numpy(), Ho) < TOL_KERNEL
    assert rel_inf(eng.gram(Xd).cpu().numpy(), orc.gram(buf[:, :p])) < TOL_KERNEL
    H0 = rng.random((p, p))
    Hacc = dev(H0.copy())
    eng.gram(Xd, dev(w), out=Hacc, accumulate=True)
    assert rel_inf(Hacc.cpu().numpy(), H0 + Ho) < 1e-11
    with eng.kernel_options(gram_variant=64):
        Hl = eng.gram(Xd, dev(w))
    assert rel_inf(H.cpu().numpy(), Hl.cpu().numpy()) < 1e-12


@pytest.mark.parametrize("p", list(range(49, 129)))
def test_gram_narrow_every_width(eng, p):
    """Every width of the row-split kernel (all tile counts x tail groups, one and two k-steps per chunk; round 3: up to 7 tiles +
    2 tail groups = p 120, then 121 .. 124 as the plan kernel's 8 full tiles), weighted and not, against an fp64 matmul.  The weighted case is the one that exposes an operand hazard at the head of the kernel's
    inline-assembly MFMA block: the scaled fragments are VALU results the compiler may place one instruction earlier."""
    n = (16384 if p <= 120 else 32768) + 3 * p               # (the plan kernel serves 32 768 rows and more)
    gen = torch.Generator(device="cuda"); gen.manual_seed(p)
    ld = p + (p & 1)
    buf = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :p] = torch.randn((n, p), dtype=torch.float64, device="cuda", generator=gen)
    X = buf[:, :p]
    w = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    Xc = X.contiguous()
    for wt in (w, None):
        H = eng.gram(X, wt)
        ref = Xc.T @ (Xc if wt is None else Xc * wt[:, None])
        d = ref.diagonal().sqrt()
        assert float(((H - ref).abs() / (d[:, None] * d[None, :])).max()) < 1e-12, (p, wt is None)
    name = eng.gram_last_kernel()[0]
    assert name.startswith("gram_narrow_kernel" if p <= 120 else "gram_plan_kernel"), (p, name)


@pytest.mark.parametrize("n,p,ld", [(9001, 51, 52), (30000, 101, 102), (8192, 111, 112), (4000, 501, 502), (5000, 37, 38),
                                    (12000, 129, 136), (2000, 1, 2), (700, 255, 256)])
def test_gram_odd_p_in_even_row_pitch(eng, orc, n, p, ld):
    """An odd column count inside 16-byte-aligned rows (e.g. the intercept column in front of an even design) takes
    the vector / LDS-DMA staging with p + 1 loaded columns; the pad column holds NaN here and must not reach H."""
    rng = np.random.default_rng(n + p)
    buf = rng.random((n, ld)) - 0.5
    buf[:, p:] = np.nan
    Xd = dev(buf)[:, :p]
    w = rng.random(n) * 0.25
    H = eng.gram(Xd, dev(w))
    assert torch.equal(H, H.T) and bool(torch.isfinite(H).all())
    assert rel_inf(H.cpu().numpy(), orc.gram(buf[:, :p], w)) < TOL_KERNEL
    H1 = eng.gram(Xd).cpu().numpy()
    assert rel_inf(H1, orc.gram(buf[:, :p])) < TOL_KERNEL


def test_aligned_row_helpers(eng):
    X = eng.empty_rows(10, 7)
    assert X.shape == (10, 7) and X.stride(0) == 8 and X.stride(1) == 1
    assert eng.empty_rows(10, 8).is_contiguous()
    Z = torch.rand(5, 4, dtype=torch.float64, device="cuda")
    A = eng.with_ones_column(Z)
    assert A.shape == (5, 5) and A.stride(0) == 6 and bool((A[:, 0] == 1).all()) and torch.equal(A[:, 1:], Z)
    assert eng.row_major(A) is A and eng.row_major(Z.T).is_contiguous()


def test_logit_pass_with_row_pitch(eng, orc):
    rng = np.random.default_rng(17)
    n, p, ld = 3000, 70, 96
    buf = rng.random((n, ld)) - 0.5
    buf[:, p:] = np.nan
    beta = rng.standard_normal(p) * 0.3
    y = (rng.random(n) < 0.5).astype(np.float64)
    w, g, ll = eng.logit_pass(dev(buf)[:, :p], dev(y), dev(beta))
    wo, go, llo = orc.logit_pass(buf[:, :p], y, beta)
    assert rel_inf(w.cpu().numpy(), wo) < TOL_KERNEL and rel_inf(g.cpu().numpy(), go) < 1e-11
    assert abs(ll.item() - llo) < 1e-12 * abs(llo)


def test_gram_and_logit_random_shapes(eng, orc):
    """40 random (n, p, row pitch, weighted?) shapes: every staging mode (scalar / 16-byte / DMA), ragged
    slabs, partial panels and tiles."""
    rng = np.random.default_rng(20260101)
    for case in range(40):
        n = int(rng.integers(1, 6000))
        p = int(rng.integers(1, 620))
        ld = p + int(rng.integers(0, 9))
        buf = rng.random((n, ld)) - 0.5
        buf[:, p:] = np.nan
        Xd = dev(buf)[:, :p]
        X = buf[:, :p]
        w = rng.random(n) * 0.25 if case % 3 else None
        H = eng.gram(Xd, dev(w) if w is not None else None).cpu().numpy()
        assert np.all(np.isfinite(H)), (n, p, ld)
        assert rel_inf(H, orc.gram(X, w)) < 1e-11, (n, p, ld)
        assert np.array_equal(H, H.T)
        beta = rng.standard_normal(p) / np.sqrt(p)
        y = (rng.random(n) < 0.5).astype(np.float64)
        wv, g, ll = eng.logit_pass(Xd, dev(y), dev(beta))
        wo, go, llo = orc.logit_pass(X, y, beta)
        assert rel_inf(wv.cpu().numpy(), wo) < 1e-11, (n, p, ld)
        assert np.max(np.abs(g.cpu().numpy() - go)) < 1e-10 * max(1.0, np.max(np.abs(go))), (n, p, ld)
        assert abs(ll.item() - llo) < 1e-11 * abs(llo), (n, p, ld)


def test_gram_identity_operand_layout(eng):
    """A = I check with asymmetric B (guide section 3): X = [I_p ; B] rows -> X'X = I + B'B."""
    p = 48
    B = np.arange(p * p, dtype=np.float64).reshape(p, p) / (p * p)
    X = np.vstack([np.eye(p), B])
    H = eng.gram(dev(X)).cpu().numpy()
    assert rel_inf(H, np.eye(p) + B.T @ B) < 1e-13


def test_gram_f32(eng):
    rng = np.random.default_rng(9)
    for (n, p) in [(3000, 100), (2000, 500), (500, 1030)]:
        X = (rng.random((n, p)) - 0.5).astype(np.float32)
        w = (rng.random(n) * 0.25).astype(np.float32)
        H = eng.gram(dev(X), dev(w)).cpu().numpy()
        Ho = X.astype(np.float64).T @ (w.astype(np.float64)[:, None] * X.astype(np.float64))
        assert rel_inf(H, Ho) < 2e-5          # fp32 accumulate over n rows


@pytest.mark.parametrize("n,p,hasw", [(16384, 768, True), (20011, 1000, False), (33000, 2000, True),
                                      (16400, 2052, True), (70001, 1028, True)])
def test_gram_f32_wide_panels(eng, n, p, hasw):
    """dlsa_gram_f32 takes the 256-column-panel kernel (gram_wide.hip) for p >= 768: ragged last chunk,
    ragged last panel, with and without weights; must agree with the 128-column kernel as well."""
    import os
    rng = np.random.default_rng(p + n)
    X = (rng.random((n, p), dtype=np.float32) - 0.5)
    w = (rng.random(n, dtype=np.float32) * 0.25) if hasw else None
    Xd, wd = dev(X), (dev(w) if hasw else None)
    H = eng.gram(Xd, wd).cpu().numpy()
    X64 = X.astype(np.float64)
    Ho = X64.T @ ((w.astype(np.float64)[:, None] if hasw else 1.0) * X64)
    assert rel_inf(H, Ho) < 2e-5
    assert np.array_equal(H, H.T)
    with eng.kernel_options(gram_wide_f32=False):
        H2 = eng.gram(Xd, wd).cpu().numpy()
    assert rel_inf(H2, Ho) < 2e-5


LOGIT_CASES = [(1, 1), (13, 3), (1000, 5), (4099, 100), (5000, 128), (3000, 129), (2048, 250),
               (3001, 500), (1500, 513), (700, 1000), (300, 2000)]


@pytest.mark.parametrize("n,p", LOGIT_CASES)
def test_logit_pass_matches_oracle(eng, orc, n, p):
    rng = np.random.default_rng(n + 7 * p)
    X = rng.random((n, p)) - 0.5
    beta = rng.standard_normal(p) * (3.0 / np.sqrt(p))
    y = (rng.random(n) < 0.5).astype(np.float64)
    w, g, ll = eng.logit_pass(dev(X), dev(y), dev(beta))
    wo, go, llo = orc.logit_pass(X, y, beta)
    assert rel_inf(w.cpu().numpy(), wo) < TOL_KERNEL
    assert rel_inf(g.cpu().numpy(), go) < 1e-11
    assert abs(ll.item() - llo) < 1e-12 * abs(llo)


def test_logit_pass_extreme_eta(eng, orc):
    X = np.array([[800.0, 0.0], [-800.0, 0.0], [0.0, 0.0], [30.0, 1.0]])
    y = np.array([1.0, 0.0, 1.0, 0.0])
    beta = np.array([1.0, 1.0])
    w, g, ll = eng.logit_pass(dev(X), dev(y), dev(beta))
    wo, go, llo = orc.logit_pass(X, y, beta)
    assert np.all(np.isfinite(w.cpu().numpy())) and np.isfinite(ll.item())
    # the reference forms prob*(1-prob) (models.py:130), which cancels for |eta| >~ 30; the kernel's
    # e/(1+e)^2 is the accurate value, so compare on the absolute scale of the weights (<= 1/4)
    assert np.allclose(w.cpu().numpy(), wo, rtol=1e-12, atol=1e-16)
    exact = np.exp(-31.0) / (1 + np.exp(-31.0)) ** 2
    assert abs(w.cpu().numpy()[3] - exact) < 1e-14 * exact
    assert abs(ll.item() - llo) < 1e-12 * abs(llo)


def test_spd_solve(eng):
    rng = np.random.default_rng(1)
    for p in (1, 7, 64, 65, 200, 500):
        A = rng.standard_normal((p + 5, p))
        S = A.T @ A + 0.1 * np.eye(p)
        v = rng.standard_normal(p)
        th = eng.spd_solve(dev(S), dev(v)).cpu().numpy()
        assert rel_inf(th, np.linalg.solve(S, v)) < 1e-9
    from dlsa_amd._lib import DlsaError
    with pytest.raises(DlsaError):
        eng.spd_solve(dev(np.array([[1.0, 2.0], [2.0, 1.0]])), dev(np.array([1.0, 1.0])))
    # p = 65 (two full blocks and a block of one row): a non-positive pivot in the second block is NOT_SPD, a NaN entry is NAN
    S = np.eye(65) + 0.01 * np.cos(np.add.outer(np.arange(65.0), np.arange(65.0)))
    S[40, 40] -= 2.0
    with pytest.raises(DlsaError) as e:
        eng.spd_solve(dev(S), dev(np.ones(65)))
    assert e.value.code == 4
    S[40, 40] += 2.0
    S[64, 63] = S[63, 64] = np.nan
    with pytest.raises(DlsaError) as e:
        eng.spd_solve(dev(S), dev(np.ones(65)))
    assert e.value.code == 6


# ---------------------------------------------------------------------------------------
F1 = sorted(os.path.basename(f)[3:-8] for f in glob.glob(os.path.join(GOLDEN, "F1_*_mle.npz")))


def _inputs(orc, z, name):
    if name.startswith("synth"):
        return orc.synth_logistic(int(z["seed"]), 0, int(z["n"]), int(z["p"]), orc.SYNTH_UNIFORM)
    g = np.load(os.path.join(GOLDEN, "games_expand_input.npz"))
    return g["X"].astype(np.float64), g["y"].astype(np.float64)


@pytest.mark.parametrize("name", F1)
def test_irls_fit_matches_reference_golden(eng, orc, name):
    """HIP map step vs the reference's own logistic_model output (tol=1e-15 tier)."""
    z = np.load(os.path.join(GOLDEN, "F1_%s_mle.npz" % name))
    X, y = _inputs(orc, z, name)
    K, icpt = int(z["K"]), bool(z["fit_intercept"])
    parts = orc.partition_rows(X.shape[0], K)
    order = np.concatenate(parts)
    Xp = X[order]
    if icpt:
        Xp = np.column_stack([np.ones(Xp.shape[0]), Xp])
    offs = np.concatenate([[0], np.cumsum([len(q) for q in parts])])
    r = eng.irls_fit(dev(Xp), dev(y[order]), offs)
    assert r["status"] == [0] * K
    assert rel_inf(r["coef"].cpu().numpy(), z["coef"]) < TOL_MLE
    assert rel_inf(r["Sig_inv"].cpu().numpy(), z["Sig_inv"]) < TOL_MLE
    assert rel_inf(r["Sig_invMcoef"].cpu().numpy(), z["Sig_invMcoef"]) < TOL_MLE
    msg = eng.sum_blocks(r["coef"], r["Sig_invMcoef"], r["Sig_inv"])
    p = Xp.shape[1]
    S = msg[: p * p].view(p, p)
    theta = eng.spd_solve(S, msg[p * p: p * p + p]).cpu().numpy()
    assert rel_inf(S.cpu().numpy(), z["Sig_inv_sum"]) < TOL_MLE
    assert rel_inf(theta, z["beta_byOLS"]) < TOL_MLE
    assert rel_inf((msg[p * p + p:] / K).cpu().numpy(), z["beta_byONESHOT"]) < TOL_MLE


def test_irls_fit_matches_oracle_p500(eng, orc):
    """The metric's column count with ragged partitions and an empty one."""
    n, p = 24000, 500
    X, y = orc.synth_logistic(20260101, 0, n, p, orc.SYNTH_UNIFORM)
    offs = [0, 9000, 9000, 16001, n]
    r = eng.irls_fit(dev(X), dev(y), offs)
    assert r["status"] == [0, 4, 0, 0]
    assert float(r["Sig_inv"][1].abs().max()) == 0.0 and float(r["coef"][1].abs().max()) == 0.0
    for k in (0, 2, 3):
        c, smc, sig = orc.logistic_model_block(X[offs[k]:offs[k + 1]], y[offs[k]:offs[k + 1]])
        assert rel_inf(r["coef"][k].cpu().numpy(), c) < TOL_MLE
        assert rel_inf(r["Sig_inv"][k].cpu().numpy(), sig) < TOL_MLE
        assert rel_inf(r["Sig_invMcoef"][k].cpu().numpy(), smc) < TOL_MLE


def test_irls_separable_data_reports_not_converged_or_spd(eng):
    X = np.array([[-2.0], [-1.0], [1.0], [2.0]] * 8)
    y = (X[:, 0] > 0).astype(np.float64)
    r = eng.irls_fit(dev(X), dev(y), [0, X.shape[0]], max_iter=25)
    assert r["status"][0] in (1, 2, 3)      # perfectly separable: no finite MLE, must not claim OK


F3 = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "F3_*.npz")))
F3I = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "F3i_*.npz")))


def _check_path(beta, z, tol=1e-8):
    """beta path vs an F3 fixture (the p = 250 fixtures hold every 10th row)."""
    if "beta" in z.files:
        assert beta.shape == z["beta"].shape
        assert rel_inf(beta, z["beta"]) < tol
    else:
        assert beta.shape[0] - 1 == int(z["steps"])
        assert rel_inf(beta[z["beta_rows"]], z["beta_sub"]) < tol


@pytest.mark.parametrize("name", F3)
def test_lars_path_matches_reference_golden(eng, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    typ = "lasso" if name.endswith("lasso") else "lar"
    S, b, n = lars_case(z)
    r = eng.lars_path(dev(S), dev(b), False, float(n), type=typ)
    beta = r["beta"].cpu().numpy()
    _check_path(beta, z)
    assert rel_inf(r["AIC"].cpu().numpy(), z["AIC"]) < 1e-8
    assert rel_inf(r["BIC"].cpu().numpy(), z["BIC"]) < 1e-8
    assert float(r["beta0"].abs().max()) == 0.0


@pytest.mark.parametrize("name", F3I)
def test_lars_intercept_branch_matches_reference_golden(eng, name):
    """lsa.py:98-104,194-204 -- the reference's intercept branch runs when called with n = p (defect D4); its beta,
    beta0, AIC and BIC (with log(p)) for that call are the golden."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    typ = "lasso" if name.endswith("lasso") else "lar"
    r = eng.lars_path(dev(z["Sigma"]), dev(z["b"]), True, float(z["n"]), type=typ)
    assert r["beta"].shape == z["beta"].shape
    assert rel_inf(r["beta"].cpu().numpy(), z["beta"]) < 1e-8
    assert np.max(np.abs(r["beta0"].cpu().numpy() - z["beta0"])) < 1e-8 * max(1.0, np.max(np.abs(z["beta0"])))
    assert rel_inf(r["AIC"].cpu().numpy(), z["AIC"]) < 1e-8
    assert rel_inf(r["BIC"].cpu().numpy(), z["BIC"]) < 1e-8


def test_lars_intercept_matches_oracle(eng, orc):
    rng = np.random.default_rng(5)
    p, n = 30, 2000
    X = np.column_stack([np.ones(n), rng.random((n, p - 1)) - 0.5])
    S = X.T @ (rng.random(n)[:, None] * 0.25 * X)
    b = orc.true_beta(p) + 0.05 * rng.standard_normal(p)
    ro = orc.lars_lsa(S, b, True, n)
    r = eng.lars_path(dev(S), dev(b), True, n)
    assert rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-8
    assert rel_inf(r["beta0"].cpu().numpy(), ro["beta0"]) < 1e-8
    assert rel_inf(r["BIC"].cpu().numpy(), ro["BIC"]) < 1e-8


def _correlated_lsa_problem(p, rho, seed):
    rng = np.random.default_rng(seed)
    n = 6 * p
    L = rng.standard_normal((3, p))
    X = np.sqrt(1 - rho) * rng.standard_normal((n, p)) + np.sqrt(rho) * (rng.standard_normal((n, 3)) @ L)
    S = X.T @ ((rng.random(n) * 0.25)[:, None] * X)
    return S, rng.standard_normal(p), n


@pytest.mark.parametrize("p,rho,seed,intercept", [(120, 0.98, 5, False), (257, 0.97, 11, False), (120, 0.98, 5, True)])
def test_lars_lasso_drops_wide_matches_oracle(eng, orc, p, rho, seed, intercept):
    """lsa.py:164-186 at sizes where the factor spans several row groups of the device mat-vecs: lasso drops
    (the factor, R^{-T} s and Gi1 are rebuilt), an odd column count (padded row stride) and the intercept."""
    S, b, n = _correlated_lsa_problem(p, rho, seed)
    ro = orc.lars_lsa(S, b, intercept, n, type="lasso")
    assert ro["beta"].shape[0] > (p - int(intercept)) + 1          # the path has drops
    r = eng.lars_path(dev(S), dev(b), intercept, float(n), type="lasso")
    assert r["beta"].shape == ro["beta"].shape
    assert rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7
    assert rel_inf(r["beta0"].cpu().numpy(), ro["beta0"]) < 1e-7 or not intercept
    assert rel_inf(r["AIC"].cpu().numpy(), ro["AIC"]) < 1e-7


def test_lars_grid_barrier_timeout_falls_back_to_one_workgroup(eng, orc, kopt):
    """The grid kernel's hand-rolled barrier is bounded: a workgroup that waits longer than the timeout aborts the
    launch, every workgroup leaves, and the host reruns the path on the single-workgroup kernel.  With a timeout of one tick every
    wait is 'too long', so the rerun is what produces the result here -- same path as the oracle's; nothing hangs."""
    from dlsa_amd import _lib
    kopt.set(lars_q=0)         # (p = 300 would otherwise run on lars_q.hip's single workgroup)
    lib = _lib.load()
    S, b, n = _correlated_lsa_problem(300, 0.9, 3)
    ro = orc.lars_lsa(S, b, False, n, type="lasso")
    before = lib.dlsa_lars_grid_barrier_timeout(1e-9)
    try:
        r = eng.lars_path(dev(S), dev(b), False, float(n), type="lasso")
        after = lib.dlsa_lars_grid_barrier_timeout(0.0)
    finally:
        lib.dlsa_lars_grid_barrier_timeout(0.0)
    assert after > before                                          # the grid launch was given up and rerun
    assert r["beta"].shape == ro["beta"].shape
    assert rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7
    r2 = eng.lars_path(dev(S), dev(b), False, float(n), type="lasso")      # default timeout again: the grid kernel completes
    assert lib.dlsa_lars_grid_barrier_timeout(0.0) == after
    assert rel_inf(r2["beta"].cpu().numpy(), r["beta"].cpu().numpy()) < 1e-7


@pytest.mark.parametrize("wgs", [1, 5, 16, 32])
def test_lars_grid_kernel_matches_single_workgroup_and_golden(eng, orc, kopt, wgs):
    """The multi-workgroup path kernel (cooperative launch, grid barriers) and the single-workgroup one walk the
    same path: reference goldens incl. drops, wide lasso paths with drops, the intercept."""
    kopt.set(lars_wgs=wgs, lars_q=0)         # lars.hip's kernels (the default for these widths is lars_q.hip, tested below)
    _lars_reference_cases(eng, orc)


def test_lars_q_clusters_barrier_timeout_falls_back_and_counts_agree(eng, orc, kopt):
    """m > 200: a few workgroups share the fused pass of lars_q.hip and meet at the same bounded grid barrier; a launch that gives
    up there is rerun on one workgroup.  Any workgroup count walks the oracle's path (p = 300 with drops, p = 700 on the 1024-thread
    build against lars.hip)."""
    from dlsa_amd import _lib
    lib = _lib.load()
    S, b, n = _correlated_lsa_problem(300, 0.9, 3)
    ro = orc.lars_lsa(S, b, False, n, type="lasso")
    for wgs in ("1", "3", "8"):
        kopt.set(lars_q_wgs=int(wgs))
        r = eng.lars_path(dev(S), dev(b), False, float(n), type="lasso")
        assert r["beta"].shape == ro["beta"].shape and rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7, wgs
        assert rel_inf(r["BIC"].cpu().numpy(), ro["BIC"]) < 1e-7
    kopt.clear("lars_q_wgs")
    before = lib.dlsa_lars_grid_barrier_timeout(1e-9)
    try:
        r = eng.lars_path(dev(S), dev(b), False, float(n), type="lasso")
        after = lib.dlsa_lars_grid_barrier_timeout(0.0)
    finally:
        lib.dlsa_lars_grid_barrier_timeout(0.0)
    assert after > before
    assert r["beta"].shape == ro["beta"].shape and rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7
    S, b, n = _correlated_lsa_problem(700, 0.9, 19)
    kopt.set(lars_q=1)                       # (lars_q.hip up to 1020 variables: since round 6 the column-split kernel takes m > 448 by default)
    rq = eng.lars_path(dev(S), dev(b), True, float(n), type="lasso")
    kopt.clear("lars_q")
    rc = eng.lars_path(dev(S), dev(b), True, float(n), type="lasso")         # the default at this width: lars_c.hip
    assert rc["beta"].shape == rq["beta"].shape and rel_inf(rc["beta"].cpu().numpy(), rq["beta"].cpu().numpy()) < 1e-7
    kopt.set(lars_q=0)
    r0 = eng.lars_path(dev(S), dev(b), True, float(n), type="lasso")
    assert rq["beta"].shape == r0["beta"].shape
    assert rel_inf(rq["beta"].cpu().numpy(), r0["beta"].cpu().numpy()) < 1e-7
    assert rel_inf(rq["beta0"].cpu().numpy(), r0["beta0"].cpu().numpy()) < 1e-7


@pytest.mark.parametrize("threads,lds", [(256, 1), (512, 1), (512, 0), (1024, 0)])
def test_lars_q_kernel_variants_match_golden_and_oracle(eng, orc, kopt, threads, lds):
    """lars_q.hip (carried Cholesky rows, the default up to m = 400) in its four builds -- Q and RT in LDS or in global memory,
    256 / 512 / 1024 threads -- on the reference goldens incl. drops, wide lasso paths with drops, the intercept; and the width
    where it hands over to lars.hip."""
    kopt.set(lars_q_threads=threads, lars_q_lds=lds)
    _lars_reference_cases(eng, orc)
    S, b, n = _correlated_lsa_problem(400, 0.9, 17)
    r = eng.lars_path(dev(S), dev(b), False, float(n), type="lasso")
    kopt.set(lars_q=0)
    r0 = eng.lars_path(dev(S), dev(b), False, float(n), type="lasso")
    assert r["beta"].shape == r0["beta"].shape
    assert rel_inf(r["beta"].cpu().numpy(), r0["beta"].cpu().numpy()) < 1e-7
    assert rel_inf(r["BIC"].cpu().numpy(), r0["BIC"].cpu().numpy()) < 1e-7


@pytest.mark.parametrize("p,intercept", [(1, False), (2, False), (2, True), (3, True)])
def test_lars_tiny_problems_match_oracle(eng, orc, p, intercept):
    """One and two penalised variables (m = p - intercept = 1, 2): the shortest paths the kernels' layouts must survive."""
    S, b, n = _correlated_lsa_problem(p, 0.5, 70 + p)
    for typ in ("lar", "lasso"):
        ro = orc.lars_lsa(S, b, intercept, n, type=typ)
        r = eng.lars_path(dev(S), dev(b), intercept, float(n), type=typ)
        assert r["beta"].shape == ro["beta"].shape
        assert rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-8
        assert rel_inf(r["BIC"].cpu().numpy(), ro["BIC"]) < 1e-8
        if intercept:
            assert rel_inf(r["beta0"].cpu().numpy(), ro["beta0"]) < 1e-8


def _lars_reference_cases(eng, orc):
    for name in F3:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        typ = "lasso" if name.endswith("lasso") else "lar"
        S, b, n = lars_case(z)
        r = eng.lars_path(dev(S), dev(b), False, float(n), type=typ)
        _check_path(r["beta"].cpu().numpy(), z)
        assert rel_inf(r["BIC"].cpu().numpy(), z["BIC"]) < 1e-8, name
    for name in F3I:                       # the reference's own intercept branch (callable with n = p)
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        r = eng.lars_path(dev(z["Sigma"]), dev(z["b"]), True, float(z["n"]), type="lasso" if name.endswith("lasso") else "lar")
        assert rel_inf(r["beta"].cpu().numpy(), z["beta"]) < 1e-8, name
        assert float((r["beta0"].cpu() - torch.from_numpy(z["beta0"])).abs().max()) < 1e-8, name
    for p, rho, seed, intercept in [(120, 0.98, 5, False), (257, 0.97, 11, False), (120, 0.98, 5, True)]:
        S, b, n = _correlated_lsa_problem(p, rho, seed)
        ro = orc.lars_lsa(S, b, intercept, n, type="lasso")
        r = eng.lars_path(dev(S), dev(b), intercept, float(n), type="lasso")
        assert r["beta"].shape == ro["beta"].shape
        assert rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7
        assert rel_inf(r["beta0"].cpu().numpy(), ro["beta0"]) < 1e-7 or not intercept
        assert rel_inf(r["AIC"].cpu().numpy(), ro["AIC"]) < 1e-7


def test_loglik_columns(eng, orc):
    rng = np.random.default_rng(8)
    n, p = 5000, 60
    X, y = orc.synth_logistic(3, 0, n, p)
    par = rng.standard_normal((p, 4)) * 0.3
    out = eng.loglik(dev(X), dev(y), dev(par)).cpu().numpy()
    assert rel_inf(out, orc.logistic_loglik(X, y, par)) < 1e-12


# ---------------------------------------------------------------------------------------
def test_full_size_properties_p500(eng):
    """BASELINE config 3's per-GPU shard (2.5e7 x 500 fp64 = 100 GB): size-independent checks.
    linearity over row blocks, exact symmetry, and trace(H) = sum_i w_i |x_i|^2 computed by an
    independent (torch elementwise) path in chunks."""
    from conftest import need_hbm
    n, p = 25_000_000, 500
    need_hbm(115e9)            # the 100 GB shard + w + chunk temporaries: asserted, never shrunk
    X, _ = eng.synth(20260101, 0, n, p, kind=eng.SYNTH_GAUSSIAN, labels=False)
    w = torch.rand(n, dtype=torch.float64, device="cuda") * 0.25
    H = eng.gram(X, w)
    assert torch.equal(H, H.T)
    half = (n // 2 // 7) * 7 + 3
    H1 = eng.gram(X[:half], w[:half])
    H2 = eng.gram(X[half:], w[half:])
    scale = float(H.abs().max())
    assert float((H1 + H2 - H).abs().max()) < 1e-11 * scale
    tr = 0.0
    diag = torch.zeros(p, dtype=torch.float64, device="cuda")
    step = 1_000_000
    for r in range(0, n, step):
        xs = X[r:r + step]
        diag += (xs * xs * w[r:r + step, None]).sum(0)
    assert float((diag - torch.diagonal(H)).abs().max()) < 1e-11 * scale
    # one off-diagonal band through an independent path
    col = torch.zeros(p, dtype=torch.float64, device="cuda")
    for r in range(0, n, step):
        xs = X[r:r + step]
        col += (xs * (xs[:, 3] * w[r:r + step])[:, None]).sum(0)
    assert float((col - H[3]).abs().max()) < 1e-11 * scale


@pytest.mark.parametrize("seed", range(24))
def test_lars_randomised_problems_match_oracle(eng, orc, seed):
    """Seeded random LSA problems (p 2..90, three correlation structures, lar / lasso, with and without the intercept
    branch): the whole path, beta0, AIC, BIC and the step count against the oracle's restatement of lsa.py:90-212."""
    rng = np.random.default_rng(9000 + seed)
    p = int(rng.integers(2, 91))
    intercept = bool(rng.random() < 0.4) and p > 2
    typ = "lasso" if rng.random() < 0.5 else "lar"
    rho = float(rng.choice([0.0, 0.5, 0.9, 0.97]))
    S, b, n = _correlated_lsa_problem(p, rho, 9100 + seed)
    if rng.random() < 0.3:                                        # sparse truth: some coefficients near zero enter late
        b[rng.random(p) < 0.5] *= 1e-3
    ro = orc.lars_lsa(S, b, intercept, n, type=typ)
    r = eng.lars_path(dev(S), dev(b), intercept, float(n), type=typ)
    assert r["beta"].shape == ro["beta"].shape, (p, typ, intercept, rho)
    assert rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7
    assert rel_inf(r["AIC"].cpu().numpy(), ro["AIC"]) < 1e-7 and rel_inf(r["BIC"].cpu().numpy(), ro["BIC"]) < 1e-7
    if intercept:
        assert rel_inf(r["beta0"].cpu().numpy(), ro["beta0"]) < 1e-7


def test_cooperative_launch_option_walks_the_same_paths():
    """dlsa_kernel_options.cooperative = 1: the multi-workgroup kernels (lars.hip's grid, lars_q.hip's clusters, the one-launch IRLS
    kernel's clusters) launched with hipLaunchCooperativeKernel give the results of the plain launches.  In a child process: streams
    created after a process's first cooperative launch serialise on this runtime (profiles/r05_coop_streams.txt), which is why the
    option is off by default -- and why this test keeps it out of the test process."""
    import subprocess
    import sys
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
from dlsa_amd import engine
rng = np.random.default_rng(5)
out = []
for p, opts in ((300, {}), (300, {"lars_q": 0}), (700, {})):
    n = 40 * p
    X = rng.random((n, p)) - 0.5
    S = torch.from_numpy(X.T @ ((rng.random(n) * 0.25)[:, None] * X)).cuda()
    b = torch.from_numpy(np.where(np.arange(p) < 0.4 * p, 1.0, 0.0) + 0.05 * rng.standard_normal(p)).cuda()
    with engine.kernel_options(**opts):
        r0 = engine.lars_path(S, b, False, float(n), type="lasso")
    with engine.kernel_options(cooperative=True, **opts):
        r1 = engine.lars_path(S, b, False, float(n), type="lasso")
    assert r0["beta"].shape == r1["beta"].shape and torch.equal(r0["beta"], r1["beta"]) and torch.equal(r0["BIC"], r1["BIC"]), (p, opts)
X, y = engine.synth(3, 0, 20 * 6000, 50, kind=engine.SYNTH_GAUSSIAN)
offs = [6000 * k for k in range(21)]
a = engine.irls_fit(X, y, offs)
with engine.kernel_options(cooperative=True):
    c = engine.irls_fit(X, y, offs)
assert engine.irls_last_fit_path() == engine.IRLS_PATH_SMALL and a["status"] == c["status"] == [0] * 20
assert torch.equal(a["coef"], c["coef"]) and torch.equal(a["Sig_inv"], c["Sig_inv"])
print("cooperative ok")
''' % (ROOT,)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cooperative ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("p,rho,seed,intercept,typ", [(1030, 0.9, 3, True, "lasso"), (1101, 0.97, 11, False, "lasso"), (1536, 0.5, 5, False, "lar"),
                                                      (2000, 0.9, 7, True, "lasso"), (2045, 0.5, 9, True, "lar")])
def test_lars_column_split_kernel_matches_the_grid_kernel(eng, orc, kopt, p, rho, seed, intercept, typ):
    """lsa.py:90-212 for 1021 .. 2044 penalised variables: lars_c.hip (round 6: the carried Cholesky rows, the pass split by columns
    over up to 64 workgroups) walks the same path as lars.hip's R^{-1} form on the same problem -- lasso paths with drops, an odd
    variable count (padded row stride), the intercept branch, the widest problem it takes (p = 2045 with the intercept) -- and as the
    oracle where the oracle finishes in seconds (p = 1030)."""
    S, b, n = _correlated_lsa_problem(p, rho, seed)
    Sd, bd = dev(S), dev(b)
    r = eng.lars_path(Sd, bd, intercept, float(n), type=typ)
    kopt.set(lars_q=0)                       # lars.hip's grid kernel (what these widths ran on up to round 5)
    r0 = eng.lars_path(Sd, bd, intercept, float(n), type=typ)
    assert r["beta"].shape == r0["beta"].shape
    if typ == "lasso" and rho > 0.8:
        assert r["beta"].shape[0] > (p - int(intercept)) + 1          # the path has drops
    for key in ("beta", "AIC", "BIC") + (("beta0",) if intercept else ()):
        assert rel_inf(r[key].cpu().numpy(), r0[key].cpu().numpy()) < 1e-7, key
    if p <= 1030:
        ro = orc.lars_lsa(S, b, intercept, n, type=typ)
        assert r["beta"].shape == ro["beta"].shape
        assert rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7 and rel_inf(r["BIC"].cpu().numpy(), ro["BIC"]) < 1e-7
        assert rel_inf(r["beta0"].cpu().numpy(), ro["beta0"]) < 1e-7


def test_lars_column_split_kernel_on_reference_cases_and_narrow_widths(eng, orc, kopt):
    """lars_c.hip forced onto every width it can take (lars_q = 2): the reference goldens incl. drops and the intercept (m = 64 .. 260),
    and the widths around the hand-over from lars_q.hip (m = 449 by default) against the oracle"""
    kopt.set(lars_q=2)
    _lars_reference_cases(eng, orc)
    kopt.clear("lars_q")
    for p, intercept in ((449, False), (450, True), (520, True)):
        S, b, n = _correlated_lsa_problem(p, 0.95, 100 + p)
        ro = orc.lars_lsa(S, b, intercept, n, type="lasso")
        r = eng.lars_path(dev(S), dev(b), intercept, float(n), type="lasso")
        assert r["beta"].shape == ro["beta"].shape and rel_inf(r["beta"].cpu().numpy(), ro["beta"]) < 1e-7, p
        assert rel_inf(r["BIC"].cpu().numpy(), ro["BIC"]) < 1e-7 and rel_inf(r["beta0"].cpu().numpy(), ro["beta0"]) < 1e-7


@pytest.mark.parametrize("wgs", [2, 17, 33, 64])
def test_lars_column_split_kernel_any_workgroup_count(eng, kopt, wgs):
    """the workgroup count decides which columns a workgroup owns and how many row groups sum them, never the path"""
    S, b, n = _correlated_lsa_problem(1101, 0.97, 11)
    Sd, bd = dev(S), dev(b)
    r0 = eng.lars_path(Sd, bd, True, float(n), type="lasso")
    kopt.set(lars_wgs=wgs)
    r = eng.lars_path(Sd, bd, True, float(n), type="lasso")
    assert r["beta"].shape == r0["beta"].shape
    assert rel_inf(r["beta"].cpu().numpy(), r0["beta"].cpu().numpy()) < 1e-8 and rel_inf(r["beta0"].cpu().numpy(), r0["beta0"].cpu().numpy()) < 1e-8


def test_lars_column_split_barrier_timeout_falls_back_to_one_workgroup(eng, kopt):
    """a grid barrier of lars_c.hip that times out aborts the launch; the host reruns the path on lars.hip's single-workgroup kernel"""
    from dlsa_amd import _lib
    lib = _lib.load()
    S, b, n = _correlated_lsa_problem(1040, 0.5, 2)
    Sd, bd = dev(S), dev(b)
    r0 = eng.lars_path(Sd, bd, False, float(n), type="lar")
    before = lib.dlsa_lars_grid_barrier_timeout(1e-9)
    try:
        r = eng.lars_path(Sd, bd, False, float(n), type="lar")
        after = lib.dlsa_lars_grid_barrier_timeout(0.0)
    finally:
        lib.dlsa_lars_grid_barrier_timeout(0.0)
    assert after > before
    assert r["beta"].shape == r0["beta"].shape and rel_inf(r["beta"].cpu().numpy(), r0["beta"].cpu().numpy()) < 1e-7


def test_lars_column_split_kernel_is_bit_reproducible(eng):
    """every workgroup of lars_c.hip reads rows other workgroups wrote (behind one grid barrier per append): a stale read would show
    as run-to-run differences.  Twelve runs of a lasso path with drops at the default count and at 29 workgroups: bit-identical."""
    S, b, n = _correlated_lsa_problem(1101, 0.97, 11)
    Sd, bd = dev(S), dev(b)
    from dlsa_amd import engine
    for wgs in (None, 29):
        with engine.kernel_options(lars_wgs=wgs) if wgs else engine.kernel_options():
            r0 = eng.lars_path(Sd, bd, True, float(n), type="lasso")
            for _ in range(11):
                r = eng.lars_path(Sd, bd, True, float(n), type="lasso")
                assert torch.equal(r["beta"], r0["beta"]) and torch.equal(r["BIC"], r0["BIC"]) and torch.equal(r["beta0"], r0["beta0"])
