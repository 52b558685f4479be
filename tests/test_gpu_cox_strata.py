"""GPU: strata in the Cox map step (csrc/cox.hip, one baseline hazard per stratum, one common beta) against the numpy reference
applied stratum by stratum (tests/cox_strata_reference.py) and, on matched pairs, against the closed form of conditional
logistic regression: the pass at a fixed beta over the stratum layouts, the edge cases of the restarts, segments longer than
64 positions, unchanged bits without strata, the per-partition fit, strided partitions, reproducibility, the frame-level
cox_model and the end-to-end DLSA combine.  Bars and normalisations as in tests/test_gpu_cox_efron.py: 1e-12 for a pass,
1e-10 for a fit, 1e-13 where two GPU paths must agree without being the same code."""
import ctypes
import functools

import numpy as np
import pytest

import cox_efron_cases as ec
import cox_efron_reference as er
import cox_reference as cr
import cox_strata_cases as cases
import cox_strata_reference as sr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TIES = ["breslow", "efron"]
LOOP = {"breslow": cr.breslow_loop, "efron": er.efron_loop}
CUMSUM = {"breslow": cr.breslow_cumsum, "efron": er.efron_cumsum}


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


def _pass(eng, X, t, ev, beta, strata, ties):
    Xd, td, ed, bd = _dev(X, t, ev, beta)
    order = torch.from_numpy(cases.sort_order(t, strata)).cuda()
    sd = _dev(strata)[0] if strata is not None else None
    H, g, ll, w = eng.cox_pass(Xd, td, ed, order, bd, want_w=True, ties=ties, strata=sd)
    return H.cpu().numpy(), g.cpu().numpy(), float(ll.item()), w.cpu().numpy()


def _check(tag, X, got, ref, tol=1e-12):
    H, g, ll, w = got
    llr, Ur, Hr = ref
    print("%s n=%d p=%d: loglik %.2e  score %.2e  H %.2e" % (
        tag, X.shape[0], X.shape[1], abs(ll - llr) / max(1.0, abs(llr)), np.max(np.abs(g - Ur)) / max(1.0, np.abs(X).sum(0).max()),
        np.max(np.abs(H - Hr)) / max(np.max(np.abs(Hr)), np.max(X * X))))
    assert abs(ll - llr) <= tol * max(1.0, abs(llr)), (ll, llr)
    assert np.max(np.abs(g - Ur)) <= tol * max(1.0, np.abs(X).sum(0).max()), np.max(np.abs(g - Ur))
    assert np.max(np.abs(H - Hr)) <= tol * max(np.max(np.abs(Hr)), np.max(X * X)), rel(H, Hr)
    assert np.all(w >= 0)


def _check_pass(eng, X, t, ev, beta, strata, ties, form=None):
    form = form or (LOOP if X.shape[0] <= 2000 else CUMSUM)[ties]
    _check("%s strata pass" % ties, X, _pass(eng, X, t, ev, beta, strata, ties), sr.stratified(form, X, t, ev, strata, beta))


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("name", cases.LAYOUTS)
@pytest.mark.parametrize("p", cases.PASS_P)
@pytest.mark.parametrize("n", cases.PASS_N)
def test_pass_matches_reference(eng, n, p, name, ties):
    _check_pass(eng, *cases.pass_case(p, n, name), ties)


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("name", ["random7", None])
def test_pass_widest_rows(eng, name, ties):
    """p = 1025: the widest row kernels (nine column chunks run as sixteen, one row per step) with scalar loads (odd p), which
    PASS_P does not reach; at n = 300 alone, where the loop form is cheap, with strata and without"""
    X, t, ev, beta, strata = cases.pass_case(1025, 300, name or "random7")
    if name is None:
        _check("%s widest pass" % ties, X, _pass(eng, X, t, ev, beta, None, ties), LOOP[ties](X, t, ev, beta))
    else:
        _check_pass(eng, X, t, ev, beta, strata, ties)


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("case", cases.EDGE_CASES)
def test_pass_edge_cases(eng, case, ties):
    X, t, ev, beta, strata = cases.edge_case(case)
    _check_pass(eng, X, t, ev, beta, strata, ties, form=LOOP[ties])


@functools.lru_cache(maxsize=None)
def _long():
    return cases.long_case()


@pytest.mark.parametrize("ties", TIES)
def test_segments_longer_than_64(eng, ties):
    """n = 300 000: L = 76 positions per segment, so the w pass takes two steps per segment, the second one partly filled"""
    X, t, ev, beta, strata = _long()
    _check_pass(eng, X, t, ev, beta, strata, ties, form=CUMSUM[ties])


def _fit(eng, X, t, ev, offs, strata, ties):
    Xd, td, ed = _dev(X, t, ev)
    sd = _dev(strata)[0] if strata is not None else None
    return eng.cox_fit(Xd, td, ed, torch.from_numpy(cases.sort_order(t, strata, offs)).cuda(), offs, ties=ties, strata=sd)


@pytest.mark.parametrize("ties", TIES)
def test_null_strata_are_bit_equal_to_the_old_entries(eng, ties):
    """The `_ties` and the oldest entries forward to the new ones with strata = NULL, so this checks the forwarding (arguments in
    the right places, the workspace of the old queries still enough) and that null strata select the unstratified model.  It
    cannot compare with the results of the build before strata existed."""
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _rowmajor, _stream, _workspace
    lib = _lib.load()
    code = eng.cox_ties(ties)
    n, p = 20_000, 12
    X, t, ev = ec.data(150, n, p, ties=30)
    beta = np.linspace(-0.4, 0.4, p)
    Xd, td, ed, bd = _dev(X, t, ev, beta)
    order = torch.from_numpy(np.argsort(-t, kind="stable").astype(np.int64)).cuda()

    def out():
        return (torch.empty((p, p), dtype=torch.float64, device="cuda"), torch.empty(p, dtype=torch.float64, device="cuda"),
                torch.empty(1, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"))
    # the `_ties` pass entry, called as the binding called it before strata existed
    H, g, ll, w = out()
    ws = _workspace(lib.dlsa_cox_ties_workspace_bytes(n, p, code), Xd.device)
    _lib.check(lib.dlsa_cox_pass_ties_f64(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), _ptr(order), n, p, code, _ptr(bd), _ptr(H), p,
                                          _ptr(g), _ptr(ll), _ptr(w), _ptr(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    H2, g2, ll2, w2 = eng.cox_pass(Xd, td, ed, order, bd, want_w=True, ties=ties)                   # the new entry, null strata
    assert torch.equal(H, H2) and torch.equal(g, g2) and torch.equal(ll, ll2) and torch.equal(w, w2)
    H3, g3, ll3, w3 = eng.cox_pass(Xd, td, ed, order, bd, want_w=True, ties=ties, strata=None)
    assert torch.equal(H, H3) and torch.equal(g, g3) and torch.equal(ll, ll3) and torch.equal(w, w3)
    if ties == "breslow":                                                                            # the oldest entry
        H4, g4, ll4, w4 = out()
        ws = _workspace(lib.dlsa_cox_workspace_bytes(n, p), Xd.device)
        _lib.check(lib.dlsa_cox_pass_f64(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), _ptr(order), n, p, _ptr(bd), _ptr(H4), p, _ptr(g4),
                                         _ptr(ll4), _ptr(w4), _ptr(ws), ws.numel(), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(H, H4) and torch.equal(g, g4) and torch.equal(ll, ll4) and torch.equal(w, w4)
    # and it is the unstratified model
    llr, _, Hr = CUMSUM[ties](X, t, ev, beta)
    assert abs(float(ll) - llr) <= 1e-12 * abs(llr) and rel(H.cpu().numpy(), Hr) <= 1e-12
    # the fit
    K = 2
    offs = [0, n // 2, n]
    od = torch.from_numpy(cases.sort_order(t, None, offs)).cuda()
    c_offs = (ctypes.c_int64 * (K + 1))(*offs)

    def old_fit(entry, wsb, *method):
        coef = torch.empty((K, p), dtype=torch.float64, device="cuda")
        smc = torch.empty((K, p), dtype=torch.float64, device="cuda")
        sig = torch.empty((K, p, p), dtype=torch.float64, device="cuda")
        ws = _workspace(wsb, Xd.device)
        n_iter, status, llh = (ctypes.c_int * K)(), (ctypes.c_int * K)(), (ctypes.c_double * K)()
        rc = entry(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), _ptr(od), c_offs, K, p, *method, 1e-13, 100, _ptr(coef), _ptr(sig),
                   _ptr(smc), n_iter, status, llh, _ptr(ws), ws.numel(), _stream())
        assert rc == 0 and list(status) == [0, 0]
        return coef, sig, smc, list(llh), list(n_iter)
    fits = [old_fit(lib.dlsa_cox_fit_ties_f64, lib.dlsa_cox_ties_workspace_bytes(n // 2, p, code), code)]
    if ties == "breslow":
        fits.append(old_fit(lib.dlsa_cox_fit_f64, lib.dlsa_cox_workspace_bytes(n // 2, p)))
    r = eng.cox_fit(Xd, td, ed, od, offs, ties=ties)
    for coef, sig, smc, llh, n_iter in fits:
        assert torch.equal(coef, r["coef"]) and torch.equal(sig, r["Sig_inv"]) and torch.equal(smc, r["Sig_invMcoef"])
        assert llh == r["loglik"] and n_iter == r["n_iter"]


@pytest.mark.parametrize("ties", TIES)
def test_one_constant_code_is_the_unstratified_model(eng, ties):
    n, p = 20_000, 12
    X, t, ev = ec.data(151, n, p, ties=30)
    beta = np.linspace(-0.4, 0.4, p)
    Hu, gu, lu, wu = _pass(eng, X, t, ev, beta, None, ties)
    Hs, gs, ls, ws = _pass(eng, X, t, ev, beta, np.full(n, -5, dtype=np.int64), ties)
    assert abs(ls - lu) <= 1e-13 * abs(lu)
    assert np.max(np.abs(gs - gu)) <= 1e-13 * np.abs(X).sum(0).max()
    assert rel(Hs, Hu) <= 1e-13 and rel(ws, wu) <= 1e-13


@functools.lru_cache(maxsize=None)
def _pairs():
    X, t, ev, beta, strata = cases.pairs_case()
    return X, t, ev, beta, strata, sr.clogit_pairs(X, ev, strata, beta), sr.clogit_pairs_fit(X, ev, strata)


@pytest.mark.parametrize("ties", TIES)
def test_matched_pairs_against_the_closed_form(eng, ties):
    X, t, ev, beta, strata, ref, (b, H, ll) = _pairs()
    _check("%s pairs pass" % ties, X, _pass(eng, X, t, ev, beta, strata, ties), ref)
    r = _fit(eng, X, t, ev, [0, len(t)], strata, ties)
    assert r["status"] == [0], r["status"]
    print("%s pairs fit: coef %.2e  Sig_inv %.2e  loglik %.2e  iterations %d" % (
        ties, rel(r["coef"][0].cpu().numpy(), b), rel(r["Sig_inv"][0].cpu().numpy(), H), abs(r["loglik"][0] - ll) / abs(ll), r["n_iter"][0]))
    assert rel(r["coef"][0].cpu().numpy(), b) <= 1e-10
    assert rel(r["Sig_inv"][0].cpu().numpy(), H) <= 1e-10
    assert rel(r["Sig_invMcoef"][0].cpu().numpy(), H @ b) <= 1e-10
    assert abs(r["loglik"][0] - ll) <= 1e-10 * abs(ll)


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("p", [3, 20])
def test_fit_matches_reference(eng, p, ties):
    n, K = 20_000, 2
    X, t, ev, strata = cases.fit_case(p, n)
    offs = [0, n // 2, n]
    r = _fit(eng, X, t, ev, offs, strata, ties)
    assert r["status"] == [0] * K, r["status"]
    for k in range(K):
        sl = slice(offs[k], offs[k + 1])
        b, H, ll = sr.fit(X[sl], t[sl], ev[sl], strata[sl], form=CUMSUM[ties])
        print("%s strata fit p=%d k=%d: coef %.2e  Sig_inv %.2e  loglik %.2e" % (
            ties, p, k, rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H), abs(r["loglik"][k] - ll) / abs(ll)))
        assert rel(r["coef"][k].cpu().numpy(), b) <= 1e-10
        assert rel(r["Sig_inv"][k].cpu().numpy(), H) <= 1e-10
        assert rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b) <= 1e-10
        assert abs(r["loglik"][k] - ll) <= 1e-10 * abs(ll)
    # the unstratified fit of the same rows is another one
    u = _fit(eng, X, t, ev, offs, None, ties)
    assert rel(u["coef"][0].cpu().numpy(), r["coef"][0].cpu().numpy()) > 1e-4


def test_partition_whose_strata_all_lack_events_is_empty(eng):
    n, p = 6000, 4
    X, t, ev, strata = cases.fit_case(p, n)
    ev[:3000] = 0.0
    r = _fit(eng, X, t, ev, [0, 3000, n], strata, "efron")
    assert r["status"] == [4, 0], r["status"]
    assert not r["Sig_inv"][0].any() and not r["coef"][0].any() and not r["Sig_invMcoef"][0].any()
    b, H, _ = sr.fit(X[3000:], t[3000:], ev[3000:], strata[3000:])
    assert rel(r["coef"][1].cpu().numpy(), b) <= 1e-10 and rel(r["Sig_inv"][1].cpu().numpy(), H) <= 1e-10


def test_strided_partitions_equal_contiguous_copies(eng):
    import dlsa_amd
    n, p, K = 30_000, 8, 5
    X, t, ev, strata = cases.fit_case(p, n)
    Xd, td, ed, sd = _dev(X, t, ev, strata)
    a = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=K, ties="efron", strata=sd)
    perm = np.concatenate([np.arange(k, n, K) for k in range(K)])
    Xc, tc, ec_, sc = _dev(X[perm], t[perm], ev[perm], strata[perm])
    offs = [0] + list(np.cumsum([len(range(k, n, K)) for k in range(K)]))
    b = dlsa_amd.fit_cox_partitions(Xc, tc, ec_, part_offsets=offs, ties="efron", strata=sc)
    assert a.status == [0] * K and b.status == [0] * K
    assert rel(a.coef.cpu().numpy(), b.coef.cpu().numpy()) <= 1e-13
    assert rel(a.Sig_inv.cpu().numpy(), b.Sig_inv.cpu().numpy()) <= 1e-13
    # and they are the stratified blocks
    bk, Hk, _ = sr.fit(X[0::K], t[0::K], ev[0::K], strata[0::K])
    assert rel(a.coef[0].cpu().numpy(), bk) <= 1e-10 and rel(a.Sig_inv[0].cpu().numpy(), Hk) <= 1e-10


def test_fit_is_bit_reproducible(eng):
    import dlsa_amd
    X, t, ev, strata = cases.fit_case(30, 50_000, S=40)
    Xd, td, ed, sd = _dev(X, t, ev, strata)
    a = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=3, ties="efron", strata=sd)
    b = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=3, ties="efron", strata=sd)
    assert a.status == [0] * 3
    assert torch.equal(a.coef, b.coef) and torch.equal(a.Sig_inv, b.Sig_inv) and torch.equal(a.Sig_invMcoef, b.Sig_invMcoef)
    assert a.loglik == b.loglik


def test_cox_model_frame(eng):
    import dlsa_amd
    df = dlsa_amd.simulate_cox(5000, 6, 1, seed=7, censor_rate=0.3, tie_levels=40, strata=4)
    part = df.drop(columns=["partition_id"])
    names = ["x%d" % i for i in range(6)]
    X = part[names].to_numpy()
    tt, ee, ss = part["time"].to_numpy(), part["event"].to_numpy(), part["stratum"].to_numpy().astype(np.int64)
    out = dlsa_amd.cox_model(part, "time", "event", ties="efron", strata="stratum")
    assert list(out.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out.shape == (6, 9)
    mb = dlsa_amd.fit_cox_partitions(*_dev(X, tt, ee), ties="efron", strata=_dev(ss)[0])
    assert np.array_equal(out["coef"].to_numpy(), mb.coef[0].cpu().numpy())
    assert np.array_equal(out[names].to_numpy(), mb.Sig_inv[0].cpu().numpy())
    b, H, ll = sr.fit(X, tt, ee, ss)
    assert rel(out["coef"].to_numpy(), b) <= 1e-10
    assert rel(out[names].to_numpy(), H) <= 1e-10
    assert abs(mb.loglik[0] - ll) <= 1e-10 * abs(ll)
    bu, _, _ = er.fit(X, tt, ee)
    assert rel(out["coef"].to_numpy(), bu) > 1e-4
    # two columns: the distinct combinations are the strata, and neither column is a feature
    part2 = part.assign(site=np.arange(5000) % 3)
    out2 = dlsa_amd.cox_model(part2, "time", "event", ties="efron", strata=["stratum", "site"])
    assert list(out2.columns) == ["par_id", "coef", "Sig_invMcoef"] + names and out2.shape == (6, 9)
    s2 = ss * 3 + np.arange(5000) % 3
    mb2 = dlsa_amd.fit_cox_partitions(*_dev(X, tt, ee), ties="efron", strata=_dev(s2)[0])
    assert np.array_equal(out2["coef"].to_numpy(), mb2.coef[0].cpu().numpy())
    assert np.array_equal(out2[names].to_numpy(), mb2.Sig_inv[0].cpu().numpy())
    b2, H2, _ = sr.fit(X, tt, ee, s2)
    assert rel(out2["coef"].to_numpy(), b2) <= 1e-10 and rel(out2[names].to_numpy(), H2) <= 1e-10


def test_simulate_cox_strata_column_and_unchanged_default(eng):
    import dlsa_amd
    a = dlsa_amd.simulate_cox(600, 4, 3, seed=11, tie_levels=30)
    b = dlsa_amd.simulate_cox(600, 4, 3, seed=11, tie_levels=30, strata=4)
    assert list(a.columns) == ["partition_id", "time", "event", "x0", "x1", "x2", "x3"]
    assert list(b.columns) == ["partition_id", "time", "event", "stratum", "x0", "x1", "x2", "x3"]
    assert np.array_equal(b["stratum"].to_numpy(), np.arange(600) // 3 % 4)
    assert np.array_equal(a[["x0", "x1", "x2", "x3"]].to_numpy(), b[["x0", "x1", "x2", "x3"]].to_numpy())
    # every partition holds every stratum, and the strata have time scales of their own
    for k in range(3):
        assert set(b["stratum"][b["partition_id"] == k]) == {0.0, 1.0, 2.0, 3.0}
    med = [np.median(b["time"][b["stratum"] == s]) for s in range(4)]
    assert med[3] > 2 * med[0]


def test_end_to_end_dlsa(eng):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    n, p, K = 40_000, 10, 4
    X, t, ev, strata = cases.fit_case(p, n)
    Xd, td, ed, sd = _dev(X, t, ev, strata)
    mb = dlsa_amd.fit_cox_partitions(Xd, td, ed, partition_num=K, ties="efron", strata=sd)
    assert mb.status == [0] * K
    out = dlsa_amd.dlsa_mapred(mb)
    blocks = [sr.fit(X[k::K], t[k::K], ev[k::K], strata[k::K]) for k in range(K)]
    ols, oneshot, S = orc.dlsa_mapred_blocks([b[0] for b in blocks], [b[1] @ b[0] for b in blocks], [b[1] for b in blocks])
    assert rel(out["beta_byOLS"].to_numpy(), ols) <= 1e-10
    assert rel(out["beta_byONESHOT"].to_numpy(), oneshot) <= 1e-10
    assert rel(out.iloc[:, 2:].to_numpy(), S) <= 1e-10
    by_aic, by_bic, _ = orc.dlsa(S, ols, n)
    res = dlsa_amd.dlsa(out.iloc[:, 2:].to_numpy(), out["beta_byOLS"].to_numpy(), n)
    assert rel(res["beta_byBIC"].to_numpy(), by_bic) <= 1e-8
    assert rel(res["beta_byAIC"].to_numpy(), by_aic) <= 1e-8


def test_bad_arguments(eng):
    import dlsa_amd
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _rowmajor, _stream, _workspace
    n, p = 300, 3
    X, t, ev, _, strata = cases.pass_case(p, n, "random7")
    Xd, td, ed, sd = _dev(X, t, ev, strata)
    with pytest.raises(TypeError, match="strata"):
        dlsa_amd.fit_cox_partitions(Xd, td, ed, strata=sd.to(torch.float64))
    with pytest.raises(ValueError, match="strata"):
        dlsa_amd.fit_cox_partitions(Xd, td, ed, strata=sd[:-1])
    with pytest.raises(RuntimeError, match="device"):
        dlsa_amd.fit_cox_partitions(Xd, td, ed, strata=sd.cpu())
    lib = _lib.load()
    order = torch.from_numpy(cases.sort_order(t, strata)).cuda()
    s32 = sd.to(torch.int32)
    bd = torch.zeros(p, dtype=torch.float64, device="cuda")
    H = torch.empty((p, p), dtype=torch.float64, device="cuda")
    ws = _workspace(lib.dlsa_cox_strata_workspace_bytes(n, p, 1, 1), Xd.device)

    def call(ties, s=s32, wsb=None):
        return lib.dlsa_cox_pass_strata_f64(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), _ptr(s), _ptr(order), n, p, ties, _ptr(bd), _ptr(H),
                                            p, None, None, None, _ptr(ws), ws.numel() if wsb is None else wsb, _stream())
    assert call(7) == 1 and "ties" in _lib.last_error()
    assert call(1, wsb=1024) == 3 and "workspace" in _lib.last_error()
    assert call(1) == 0                                     # a following valid call works
    torch.cuda.synchronize()
    _, _, Hr = sr.stratified(er.efron_loop, X, t, ev, strata, np.zeros(p))
    assert rel(H.cpu().numpy(), Hr) <= 1e-12
    uo = torch.from_numpy(cases.sort_order(t, None)).cuda()
    assert lib.dlsa_cox_pass_strata_f64(_ptr(Xd), _rowmajor(Xd), _ptr(td), _ptr(ed), None, _ptr(uo), n, p, 1, _ptr(bd), _ptr(H), p, None,
                                        None, None, _ptr(ws), ws.numel(), _stream()) == 0          # null strata: unstratified
    torch.cuda.synchronize()
    _, _, Hu = er.efron_loop(X, t, ev, np.zeros(p))
    assert rel(H.cpu().numpy(), Hu) <= 1e-12
