"""GPU: the Cox proportional-hazards map step (csrc/cox.hip) against the numpy Breslow reference (tests/cox_reference.py):
the pass at a fixed beta (loglik, score, information), the per-partition fit, strided partitions, reproducibility, the
end-to-end DLSA combine and the frame-level cox_model."""
import numpy as np
import pytest

import cox_reference as cr
import newton_reference as nw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


def _data(seed, n, p, ties=None, censor=0.3, scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p)) * scale
    beta = np.where(np.arange(p) < max(1, int(0.4 * p)), 1.0, 0.0)
    t = rng.exponential(1.0, n) / np.exp(X @ beta / max(1.0, scale))
    if ties:
        q = np.quantile(t, np.linspace(0, 1, ties + 1)[1:])
        t = q[np.minimum(np.searchsorted(q, t), ties - 1)]
    ev = (rng.random(n) >= censor).astype(np.float64)
    return X, t, ev


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _pass(eng, X, t, ev, beta):
    Xd, td, ed, bd = _dev(X, t, ev, beta)
    order = torch.from_numpy(np.argsort(-t, kind="stable").astype(np.int64)).cuda()
    H, g, ll, w = eng.cox_pass(Xd, td, ed, order, bd, want_w=True)
    return H.cpu().numpy(), g.cpu().numpy(), float(ll.item()), w.cpu().numpy()


def _check_pass(eng, X, t, ev, beta, tol=1e-12):
    H, g, ll, _ = _pass(eng, X, t, ev, beta)
    form = cr.breslow_loop if X.shape[0] <= 2000 else cr.breslow_cumsum
    llr, Ur, Hr = form(X, t, ev, beta)
    assert abs(ll - llr) <= tol * max(1.0, abs(llr)), (ll, llr)
    assert np.max(np.abs(g - Ur)) <= tol * max(1.0, np.abs(X).sum(0).max()), np.max(np.abs(g - Ur))
    # (one row: H = x x' - x x' = 0; the scale is that of the terms)
    assert np.max(np.abs(H - Hr)) <= tol * max(np.max(np.abs(Hr)), np.max(X * X)), rel(H, Hr)


@pytest.mark.parametrize("p", [1, 5, 50, 100, 130, 500])
@pytest.mark.parametrize("n", [1, 7, 300, 5000])
def test_pass_matches_reference(eng, p, n):
    X, t, ev = _data(10 + p + n, n, p, ties=None if n % 2 else 20)
    ev[0] = 1.0
    beta = np.linspace(-0.5, 0.5, p)
    _check_pass(eng, X, t, ev, beta)


@pytest.mark.parametrize("p", [5, 100])
def test_pass_large_and_tied(eng, p):
    X, t, ev = _data(20 + p, 200_000, p, ties=20)
    _check_pass(eng, X, t, ev, np.linspace(-0.3, 0.3, p))


@pytest.mark.parametrize("case", ["all_tied", "no_censoring", "single_event", "eta_range"])
def test_pass_edge_cases(eng, case):
    n, p = 2000, 6          # (the loop form of the reference: one max per risk set, any eta range)
    X, t, ev = _data(30, n, p)
    beta = np.linspace(-0.5, 0.5, p)
    if case == "all_tied":
        t[:] = 1.0
    elif case == "no_censoring":
        ev[:] = 1.0
    elif case == "single_event":
        ev[:] = 0.0
        ev[n // 2] = 1.0
    else:
        # eta spans more than 700 (exp overflows): a binary column with coefficient 800 -- the risk sets that hold such rows
        # are dominated by them, and the information stays well-conditioned in the other columns
        X[:, 0] = (np.random.default_rng(31).random(n) < 0.3).astype(np.float64)
        beta[0] = 800.0
        assert np.ptp(X @ beta) > 700
    _check_pass(eng, X, t, ev, beta)


def _fit(eng, X, t, ev, offs, **kw):
    Xd, td, ed = _dev(X, t, ev)
    order = np.concatenate([offs[k] + np.argsort(-t[offs[k]:offs[k + 1]], kind="stable") for k in range(len(offs) - 1)])
    return eng.cox_fit(Xd, td, ed, torch.from_numpy(order.astype(np.int64)).cuda(), offs, **kw)


@pytest.mark.parametrize("p,ties", [(3, None), (20, 20), (100, None)])
def test_fit_matches_reference(eng, p, ties):
    n, K = 40_000, 4
    X, t, ev = _data(40 + p, n, p, ties=ties)
    offs = [k * n // K for k in range(K + 1)]
    r = _fit(eng, X, t, ev, offs)
    assert r["status"] == [0] * K, r["status"]
    for k in range(K):
        sl = slice(offs[k], offs[k + 1])
        b, H, ll = cr.fit(X[sl], t[sl], ev[sl])
        assert rel(r["coef"][k].cpu().numpy(), b) <= 1e-10
        assert rel(r["Sig_inv"][k].cpu().numpy(), H) <= 1e-10
        assert rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b) <= 1e-10
        assert abs(r["loglik"][k] - ll) <= 1e-10 * abs(ll)


# Only the host loop is under test: one partition of 600 rows, p = 3.  The generator's times with the first column's effect
# sharpened from 1 to 8: the undamped reference then needs 6 evaluations from beta = 0, so max_iter + 1 <= 4 never suffices.
# (No halving case here: no Cox case of this suite overshoots, and none was found at this size; the safeguard's Cox rules are
# checked on scripted sequences in test_newton_fit_cpu.py.)
@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_budget_stops_at_the_evaluated_iterate(eng, max_iter):
    n, p = 600, 3
    X, t, ev = _data(70, n, p)
    t = t * np.exp(-7.0 * X[:, 0])
    evals, bs, lls = nw.undamped(lambda b: cr.breslow_cumsum(X, t, ev, b), np.zeros(p), 1e-13)
    assert evals is not None and evals > max_iter + 1 and nw.monotone(lls[:max_iter + 1])       # no halving in the budget
    r = _fit(eng, X, t, ev, [0, n], max_iter=max_iter)
    assert r["status"] == [1] and r["rc"] == 5
    assert r["n_iter"] == [max_iter + 1]
    # max_iter steps were taken; the last evaluation's step was not: coef is where H, g and loglik were evaluated
    coef = r["coef"][0].cpu().numpy()
    assert rel(coef, bs[max_iter]) <= 1e-10
    assert abs(r["loglik"][0] - lls[max_iter]) <= 1e-10 * abs(lls[max_iter])
    H, _, _, _ = _pass(eng, X, t, ev, coef)
    assert rel(r["Sig_inv"][0].cpu().numpy(), H) <= 1e-12
    assert rel(r["Sig_invMcoef"][0].cpu().numpy(), H @ coef) <= 1e-12


def test_fit_empty_and_all_censored_partitions(eng):
    n, p = 6000, 4
    X, t, ev = _data(50, n, p)
    ev[2000:4000] = 0.0
    offs = [0, 2000, 4000, 4000, n]
    r = _fit(eng, X, t, ev, offs)
    assert r["status"] == [0, 4, 4, 0], r["status"]
    for k in (1, 2):
        assert not r["Sig_inv"][k].any() and not r["coef"][k].any() and not r["Sig_invMcoef"][k].any()


def test_fit_offset_column(eng):
    n, p = 20_000, 4
    X, t, ev = _data(60, n, p)
    X[:, 1] = 50.0 + np.random.default_rng(61).standard_normal(n)
    r = _fit(eng, X, t, ev, [0, n])
    assert r["status"] == [0]
    b, H, _ = cr.fit(X, t, ev)
    assert rel(r["coef"][0].cpu().numpy(), b) <= 1e-10
    assert rel(r["Sig_inv"][0].cpu().numpy(), H) <= 1e-10


def test_strided_partitions_equal_contiguous_copies(eng):
    import dlsa_amd
    n, p, K = 30_000, 8, 5
    X, t, ev = _data(70, n, p, ties=50)
    Xd, td, ed = _dev(X, t, ev)
    a = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=K)
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    Xc, tc, ec = _dev(X[perm], t[perm], ev[perm])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    b = dlsa_amd.fit_cox_partitions(Xc, tc, ec, part_offsets=offs)
    assert a.status == [0] * K and b.status == [0] * K
    assert rel(a.coef.cpu().numpy(), b.coef.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_inv.cpu().numpy(), b.Sig_inv.cpu().numpy()) <= 1e-13


def test_fit_is_bit_reproducible(eng):
    import dlsa_amd
    X, t, ev = _data(80, 50_000, 30, ties=100)
    Xd, td, ed = _dev(X, t, ev)
    a = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=3)
    b = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=3)
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K = 80_000, 10, 8
    X, t, ev = _data(90, n, p, ties=200)
    Xd, td, ed = _dev(X, t, ev)
    mb = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=K)
    assert mb.status == [0] * K
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [cr.fit(X[k::K], t[k::K], ev[k::K]) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[1] @ b[0] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = dlsa_amd.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


def test_cox_model_frame(eng):
    import dlsa_amd
    df = dlsa_amd.simulate_cox(5000, 6, 1, seed=7, censor_rate=0.3, tie_levels=40)
    part = df.drop(columns=["partition_id"])
    out = dlsa_amd.cox_model(part, "time", "event")
    names = ["x%d" % i for i in range(6)]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (6, 9)
    X = part[names].to_numpy()
    mb = dlsa_amd.fit_cox_partitions(*_dev(X, part["time"].to_numpy(), part["event"].to_numpy()))
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    b, H, _ = cr.fit(X, part["time"].to_numpy(), part["event"].to_numpy())
    assert rel(out["coef"].to_numpy(), b) <= 1e-10


def test_full_size_partition(eng):
    import dlsa_amd
    n, p = 10_000_000, 100
    X, _ = eng.synth(123, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: int(0.4 * p)] = 1.0
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.empty(n, dtype=torch.float64, device="cuda").exponential_(generator=g) / torch.exp(X @ beta)
    ev = (torch.rand(n, dtype=torch.float64, device="cuda", generator=g) > 0.3).to(torch.float64)
    mb = dlsa_amd.fit_cox_partitions(X, t, ev)
    assert mb.status == [0]
    coef = mb.coef[0]
    order = torch.sort(-t, stable=True).indices
    H, U, _, _ = eng.cox_pass(X, t, ev, order, coef)
    scale = float(X.abs().sum(0).max())
    assert float(U.abs().max()) <= 1e-9 * scale
    Hn = H.cpu().numpy()
    assert np.array_equal(Hn, Hn.T) and np.all(np.linalg.eigvalsh(Hn) > 0)
    assert rel(Hn, mb.Sig_inv[0].cpu().numpy()) <= 1e-10
    # a 2e5-row slice against the cumsum reference
    m = 200_000
    Xs, ts, es = X[:m].cpu().numpy(), t[:m].cpu().numpy(), ev[:m].cpu().numpy()
    _check_pass(eng, Xs, ts, es, coef.cpu().numpy())
