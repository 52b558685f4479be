"""GPU: Efron's approximation for tied event times in the Cox map step (csrc/cox.hip, ties="efron") against the numpy reference
(tests/cox_efron_reference.py): the pass at a fixed beta on tied inputs, the edge cases of the tie bookkeeping, A rows over
more than one chunk, the forwarding of the Breslow entries, the per-partition fit, strided partitions, reproducibility, the
frame-level cox_model and the end-to-end DLSA combine.  Bars as in tests/test_gpu_cox.py."""
import ctypes

import numpy as np
import pytest

import cox_efron_cases as cases
import cox_efron_reference as er
import cox_reference as cr

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


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _pass(eng, X, t, ev, beta, ties="efron"):
    Xd, td, ed, bd = _dev(X, t, ev, beta)
    order = torch.from_numpy(np.argsort(-t, kind="stable").astype(np.int64)).cuda()
    H, g, ll, w = eng.cox_pass(Xd, td, ed, order, bd, want_w=True, ties=ties)
    return H.cpu().numpy(), g.cpu().numpy(), float(ll.item()), w.cpu().numpy()


def _check_pass(eng, X, t, ev, beta, tol=1e-12, form=None):
    H, g, ll, w = _pass(eng, X, t, ev, beta)
    form = form or (er.efron_loop if X.shape[0] <= 2000 else er.efron_cumsum)
    llr, Ur, Hr = form(X, t, ev, beta)
    print("efron pass n=%d p=%d: loglik %.2e  score %.2e  H %.2e" % (
        X.shape[0], X.shape[1], abs(ll - llr) / max(1.0, abs(llr)), np.max(np.abs(g - Ur)) / max(1.0, np.abs(X).sum(0).max()),
        np.max(np.abs(H - Hr)) / max(np.max(np.abs(Hr)), np.max(X * X))))
    assert abs(ll - llr) <= tol * max(1.0, abs(llr)), (ll, llr)
    assert np.max(np.abs(g - Ur)) <= tol * max(1.0, np.abs(X).sum(0).max()), np.max(np.abs(g - Ur))
    assert np.max(np.abs(H - Hr)) <= tol * max(np.max(np.abs(Hr)), np.max(X * X)), rel(H, Hr)
    assert np.all(w >= 0)                       # c >= h1 >= h2


@pytest.mark.parametrize("p", cases.PASS_P)
@pytest.mark.parametrize("n", cases.PASS_N)
def test_pass_matches_reference(eng, p, n):
    _check_pass(eng, *cases.pass_case(p, n))


@pytest.mark.parametrize("case", cases.EDGE_CASES)
def test_pass_edge_cases(eng, case):
    X, t, ev, beta = cases.edge_case(case)
    _check_pass(eng, X, t, ev, beta, form=er.efron_loop)


def test_a_rows_across_chunks(eng):
    """p = 500: an A chunk holds 256 MB / 4000 B = 67108 rows; more groups with events than that, so that the rows of the
    groups (two for a group of two events or more) spread over more than one chunk and some group's pair straddles the cut"""
    n, p = 200_000, 500
    X, t, ev = cases.data(140, n, p, ties=90_000)
    groups = len(np.unique(t[ev != 0]))
    assert groups > 67_108, groups
    beta = np.linspace(-0.3, 0.3, p)
    H, g, ll, _ = _pass(eng, X, t, ev, beta)
    llr, Ur, Hr, rows = er.efron_cumsum(X, t, ev, beta, return_rows=True)
    assert rows > groups
    assert abs(ll - llr) <= 1e-12 * abs(llr), (ll, llr)
    assert np.max(np.abs(g - Ur)) <= 1e-12 * np.abs(X).sum(0).max()
    assert np.max(np.abs(H - Hr)) <= 1e-12 * np.max(np.abs(Hr)), rel(H, Hr)


def _order(t, offs):
    return np.concatenate([offs[k] + np.argsort(-t[offs[k]:offs[k + 1]], kind="stable") for k in range(len(offs) - 1)]).astype(np.int64)


def _fit(eng, X, t, ev, offs, ties="efron"):
    Xd, td, ed = _dev(X, t, ev)
    return eng.cox_fit(Xd, td, ed, torch.from_numpy(_order(t, offs)).cuda(), offs, ties=ties)


def test_breslow_through_the_new_entries_is_bit_equal_to_the_old_entries(eng):
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _rowmajor, _stream, _workspace
    lib = _lib.load()
    n, p = 20_000, 12
    X, t, ev = cases.data(150, n, p, ties=30)
    beta = np.linspace(-0.4, 0.4, p)
    Xd, td, ed, bd = _dev(X, t, ev, beta)
    order = torch.from_numpy(np.argsort(-t, kind="stable").astype(np.int64)).cuda()
    # the old pass entry, called as the binding called it before the tie method existed
    H = torch.empty((p, p), dtype=torch.float64, device="cuda")
    g = torch.empty(p, dtype=torch.float64, device="cuda")
    ll = torch.empty(1, dtype=torch.float64, device="cuda")
    w = torch.empty(n, dtype=torch.float64, device="cuda")
    ws = _workspace(lib.dlsa_cox_workspace_bytes(n, p), Xd.device)
    _lib.check(lib.dlsa_cox_pass_f64(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), _ptr(order), n, p, _ptr(bd), _ptr(H), p, _ptr(g),
                                     _ptr(ll), _ptr(w), _ptr(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    H2, g2, ll2, w2 = eng.cox_pass(Xd, td, ed, order, bd, want_w=True, ties="Breslow")
    assert torch.equal(H, H2) and torch.equal(g, g2) and torch.equal(ll, ll2) and torch.equal(w, w2)
    H3, g3, ll3, w3 = eng.cox_pass(Xd, td, ed, order, bd, want_w=True)
    assert torch.equal(H, H3) and torch.equal(g, g3) and torch.equal(ll, ll3) and torch.equal(w, w3)
    # and it is Breslow: not Efron's value on these tied rows
    llr, _, Hr = cr.breslow_cumsum(X, t, ev, beta)
    assert abs(float(ll) - llr) <= 1e-12 * abs(llr) and rel(H.cpu().numpy(), Hr) <= 1e-12
    # the fit
    K = 2
    offs = [0, n // 2, n]
    od = torch.from_numpy(_order(t, offs)).cuda()
    coef = torch.empty((K, p), dtype=torch.float64, device="cuda")
    smc = torch.empty((K, p), dtype=torch.float64, device="cuda")
    sig = torch.empty((K, p, p), dtype=torch.float64, device="cuda")
    ws = _workspace(lib.dlsa_cox_workspace_bytes(n // 2, p), Xd.device)
    c_offs = (ctypes.c_int64 * (K + 1))(*offs)
    n_iter, status, llh = (ctypes.c_int * K)(), (ctypes.c_int * K)(), (ctypes.c_double * K)()
    rc = lib.dlsa_cox_fit_f64(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), _ptr(od), c_offs, K, p, 1e-13, 100, _ptr(coef), _ptr(sig),
                              _ptr(smc), n_iter, status, llh, _ptr(ws), ws.numel(), _stream())
    assert rc == 0 and list(status) == [0, 0]
    r = eng.cox_fit(Xd, td, ed, od, offs, ties="breslow")
    assert torch.equal(coef, r["coef"]) and torch.equal(sig, r["Sig_inv"]) and torch.equal(smc, r["Sig_invMcoef"])
    assert list(llh) == r["loglik"] and list(n_iter) == r["n_iter"]


def test_efron_is_breslow_on_untied_data(eng):
    n, p = 20_000, 12
    X, t, ev = cases.data(151, n, p)
    assert len(np.unique(t)) == n
    beta = np.linspace(-0.4, 0.4, p)
    Hb, gb, lb, wb = _pass(eng, X, t, ev, beta, ties="breslow")
    He, ge, le, we = _pass(eng, X, t, ev, beta, ties="efron")
    assert abs(le - lb) <= 1e-13 * abs(lb)
    assert np.max(np.abs(ge - gb)) <= 1e-13 * np.abs(X).sum(0).max()
    assert rel(He, Hb) <= 1e-13 and rel(we, wb) <= 1e-13


@pytest.mark.parametrize("p,levels", [(3, 5), (20, 20), (100, 200)])
def test_fit_matches_reference(eng, p, levels):
    n, K = 40_000, 4
    X, t, ev = cases.data(160 + p, n, p, ties=levels)
    offs = [k * n // K for k in range(K + 1)]
    r = _fit(eng, X, t, ev, offs)
    assert r["status"] == [0] * K, r["status"]
    for k in range(K):
        sl = slice(offs[k], offs[k + 1])
        b, H, ll = er.fit(X[sl], t[sl], ev[sl])
        print("efron fit p=%d levels=%d k=%d: coef %.2e  Sig_inv %.2e  loglik %.2e" % (
            p, levels, k, rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H), abs(r["loglik"][k] - ll) / abs(ll)))
        assert rel(r["coef"][k].cpu().numpy(), b) <= 1e-10
        assert rel(r["Sig_inv"][k].cpu().numpy(), H) <= 1e-10
        assert rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b) <= 1e-10
        assert abs(r["loglik"][k] - ll) <= 1e-10 * abs(ll)
    # Breslow's fit is another one on these rows
    bb, _, _ = cr.fit(X[:offs[1]], t[:offs[1]], ev[:offs[1]])
    assert rel(r["coef"][0].cpu().numpy(), bb) > 1e-4


def test_fit_empty_and_all_censored_partitions(eng):
    n, p = 6000, 4
    X, t, ev = cases.data(170, n, p, ties=20)
    ev[2000:4000] = 0.0
    offs = [0, 2000, 4000, 4000, n]
    r = _fit(eng, X, t, ev, offs)
    assert r["status"] == [0, 4, 4, 0], r["status"]
    for k in (1, 2):
        assert not r["Sig_inv"][k].any() and not r["coef"][k].any() and not r["Sig_invMcoef"][k].any()
    b, H, _ = er.fit(X[4000:], t[4000:], ev[4000:])
    assert rel(r["coef"][3].cpu().numpy(), b) <= 1e-10 and rel(r["Sig_inv"][3].cpu().numpy(), H) <= 1e-10


def test_strided_partitions_equal_contiguous_copies(eng):
    import dlsa_amd
    n, p, K = 30_000, 8, 5
    X, t, ev = cases.data(180, n, p, ties=50)
    Xd, td, ed = _dev(X, t, ev)
    a = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=K, ties="efron")
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    Xc, tc, ec = _dev(X[perm], t[perm], ev[perm])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    b = dlsa_amd.fit_cox_partitions(Xc, tc, ec, part_offsets=offs, ties="efron")
    assert a.status == [0] * K and b.status == [0] * K
    assert rel(a.coef.cpu().numpy(), b.coef.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_inv.cpu().numpy(), b.Sig_inv.cpu().numpy()) <= 1e-13


def test_fit_is_bit_reproducible(eng):
    import dlsa_amd
    X, t, ev = cases.data(190, 50_000, 30, ties=100)
    Xd, td, ed = _dev(X, t, ev)
    a = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=3, ties="efron")
    b = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=3, ties="efron")
    assert a.status == [0] * 3
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik


def test_cox_model_frame(eng):
    import dlsa_amd
    df = dlsa_amd.simulate_cox(5000, 6, 1, seed=7, censor_rate=0.3, tie_levels=40)
    part = df.drop(columns=["partition_id"])
    out = dlsa_amd.cox_model(part, "time", "event", ties="efron")
    names = ["x%d" % i for i in range(6)]
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (6, 9)
    X = part[names].to_numpy()
    tt, ee = part["time"].to_numpy(), part["event"].to_numpy()
    mb = dlsa_amd.fit_cox_partitions(*_dev(X, tt, ee), ties="efron")
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    b, H, ll = er.fit(X, tt, ee)
    assert rel(out["coef"].to_numpy(), b) <= 1e-10
    assert rel(out[names].to_numpy(), H) <= 1e-10
    assert abs(mb.loglik[0] - ll) <= 1e-10 * abs(ll)          # the log partial likelihood of the chosen method


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K = 80_000, 10, 8
    X, t, ev = cases.data(200, n, p, ties=200)
    Xd, td, ed = _dev(X, t, ev)
    mb = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=K, ties="efron")
    assert mb.status == [0] * K
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [er.fit(X[k::K], t[k::K], ev[k::K]) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[1] @ b[0] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = dlsa_amd.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


def test_bad_tie_methods(eng):
    import dlsa_amd
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _rowmajor, _stream, _workspace
    n, p = 500, 3
    X, t, ev = cases.data(210, n, p, ties=10)
    Xd, td, ed = _dev(X, t, ev)
    with pytest.raises(ValueError, match="ties"):
        dlsa_amd.fit_cox_partitions(Xd, td, ed, ties="exact")
    lib = _lib.load()
    order = torch.from_numpy(np.argsort(-t, kind="stable").astype(np.int64)).cuda()
    bd = torch.zeros(p, dtype=torch.float64, device="cuda")
    H = torch.empty((p, p), dtype=torch.float64, device="cuda")
    ws = _workspace(lib.dlsa_cox_ties_workspace_bytes(n, p, 1), Xd.device)

    def call(ties):
        return lib.dlsa_cox_pass_ties_f64(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), _ptr(order), n, p, ties, _ptr(bd), _ptr(H), p,
                                          None, None, None, _ptr(ws), ws.numel(), _stream())
    assert call(7) == 1 and "ties" in _lib.last_error()
    assert call(1) == 0                                     # a following valid call works
    torch.cuda.synchronize()
    _, _, Hr = er.efron_loop(X, t, ev, np.zeros(p))
    assert rel(H.cpu().numpy(), Hr) <= 1e-12
