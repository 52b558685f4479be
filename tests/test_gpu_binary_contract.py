"""GPU: the memory and the stream contract of the C ABI for the six entries of the family extension header
include/dlsa_hip_binary.h, which no other contract table reads.  The machinery is that of tests/test_gpu_workspace_contract.py and
tests/test_gpu_stream_contract.py -- the guarded workspace, the gates, the recorders, the warm and the gated run -- and the two
proxies are those of tests/test_gpu_ordinal_contract.py, pointed at _lib.BINARY_SIGNATURES and at this header; this file brings the
cases (tests/binary_contract_cases.py) and the runners with the bars of tests/test_gpu_binary.py.

Per link, pass and fit at p = 5 and p = 130: on a body of exactly the query, filled with 0xFF, between guards -- DLSA_OK, intact
guards, the bars, and the bits of a run on a 0x00 body; ws_bytes - 1 and the pointer + 8 -- DLSA_ERR_WORKSPACE with outputs and
guards untouched; ldh = pe + 3 -- the same bits and clean pad columns; on a side stream behind a busy default stream, and with inputs
that arrive late on that side stream."""
import functools

import pytest

import binary_contract_cases as bc
import binary_reference as br
import guarded_workspace as gw
import stream_gate as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_gpu_binary as tgb                               # noqa: E402  (the pass and fit checks and their bars)
import test_gpu_ordinal_contract as base                    # noqa: E402  (the proxies of an extension header)
import test_gpu_stream_contract as tsc                      # noqa: E402  (the warm and the gated run)
import test_gpu_workspace_contract as wct                   # noqa: E402  (the guarded run, the recorders)
from test_gpu_workspace_contract import eng, orc, api       # noqa: E402,F401  (module-scoped fixtures)

BY_ID = {c.id: c for c in bc.CASES}
rel, same_bits, dev = wct.rel, wct.same_bits, wct.dev


@pytest.fixture(scope="module")
def side():
    assert torch.cuda.is_available()
    sg.side_stream(1)
    return sg.side_stream()


class BinaryStreamProxy(tsc.StreamProxy):
    """tsc.StreamProxy that also times, and notes the stream of, the stream-taking entries of this extension header"""

    def __init__(self, lib, before_first=None, after=None):
        super().__init__(lib, before_first, after)
        self._names = self._names | set(bc.stream_entries())


@pytest.fixture(autouse=True)
def _extension_proxies(monkeypatch):
    """base.OrdinalLibProxy looks an entry up in _lib.ORDINAL_SIGNATURES: for this file that table also holds this header's entries;
    the guarded, warm and gated runs of the two contract tests build their proxy by these names"""
    from dlsa_amd import _lib
    monkeypatch.setattr(_lib, "ORDINAL_SIGNATURES", {**_lib.ORDINAL_SIGNATURES, **_lib.BINARY_SIGNATURES})
    monkeypatch.setattr(wct, "LibProxy", base.OrdinalLibProxy)
    monkeypatch.setattr(tsc, "StreamProxy", BinaryStreamProxy)
    for table in (wct.RUN, tsc.RUN):
        monkeypatch.setitem(table, "binary_pass", run_pass)
        monkeypatch.setitem(table, "binary_fit", run_fit)


# ---- the runners: the engine calls and the bars of tests/test_gpu_binary.py ------------------------------------------------------------
def run_pass(c, link, n, p, icpt):
    X, y, o = tgb._data(link, 10 + p, n, p, icpt, True)
    tgb._check_pass(c.eng, link, X, y, o, tgb._away_from_optimum(p + icpt), icpt)           # 1e-12, H bitwise symmetric


@functools.lru_cache(maxsize=None)
def _fit_case(link, rows, K, p, icpt, strided):
    n = rows * K
    X, y, o = tgb._data(link, 40 + p, n, p, icpt, True)
    parts = [slice(k, n, K) for k in range(K)] if strided else [slice(k * rows, (k + 1) * rows) for k in range(K)]
    return X, y, o, [br.newton_fit(link, X[s], y[s], o[s], icpt) for s in parts]


def _check_fit(r, refs, what):
    assert r["status"] == [0] * len(refs) and r["rc"] == 0, r["status"]
    worst = 0.0
    for k, (b, H, Hb, ll) in enumerate(refs):                   # test_fit_matches_reference: 1e-10
        worst = max(worst, rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H), rel(r["Sig_invMcoef"][k].cpu().numpy(), Hb),
                    abs(r["loglik"][k] - ll) / abs(ll))
    print("binary fit %s (%s evaluations): worst relative error %.1e" % (what, r["n_iter"], worst))
    assert worst <= 1e-10, worst


def _fit_call(eng, link, rows, K, icpt, strided):
    first = list(range(K)) if strided else [k * rows for k in range(K)]
    fit = tgb._fit_ex(eng, link)
    return lambda X, y, o: fit(X, y, first, [rows] * K, row_step=K if strided else 1, offset=o, fit_intercept=icpt)


def run_fit(c, link, rows, K, p, icpt, strided):
    X, y, o, refs = _fit_case(link, rows, K, p, icpt, strided)
    r = _fit_call(c.eng, link, rows, K, icpt, strided)(dev(X), dev(y), dev(o))
    _check_fit(r, refs, "%s %dx%d p=%d icpt=%d step=%d" % (link, K, rows, p, icpt, K if strided else 1))


# ---- the memory contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(BY_ID))
def test_contract_at_the_declared_size(eng, orc, api, cid):
    """DLSA_OK, intact guards and the bar on a body of exactly the query filled with 0xFF; the same bits on a body filled with 0x00"""
    from dlsa_amd import _lib
    case, ctx = BY_ID[cid], wct.Ctx(eng, orc, api)
    seen, g = wct._guarded_run(case, ctx, gw.POISON)
    q = getattr(_lib.load(), case.queries[0])
    pr = case.params
    want = q(pr["n"], pr["p"], int(pr["icpt"]), 1) if case.family == "binary_pass" else q(pr["rows"], pr["p"], int(pr["icpt"]), pr["K"] if pr["strided"] else 1)
    assert [b for _, b in g.queries] == [want] and want > 0 and want % 256 == 0
    print("contract %s: %d workspace of %d bytes" % (cid, len(g.allocations), g.queries[0][1]))
    seen0, _ = wct._guarded_run(case, ctx, 0x00)
    assert [name for name, _ in seen] == [name for name, _ in seen0] and len(seen) == 1
    for (name, a), (_, b) in zip(seen, seen0):
        assert same_bits(a, b), "%s: the result depends on what the workspace held before the call" % name


@pytest.mark.parametrize("mode", ["short", "offset"])
@pytest.mark.parametrize("cid", list(BY_ID))
def test_refusals(eng, orc, api, cid, mode):
    """ws_bytes = query - 1, and the body pointer offset by 8: DLSA_ERR_WORKSPACE, the outputs of the call and every guard untouched"""
    from dlsa_amd import _lib, engine
    case, ctx = BY_ID[cid], wct.Ctx(eng, orc, api)
    entry = case.entries[0]
    with pytest.MonkeyPatch.context() as mp:
        g = gw.guarded(mp)
        shim = wct.SentinelTorch()
        proxy = base.OrdinalLibProxy(_lib.load(), mode, only=entry, shim=shim)
        mp.setattr(_lib, "load", lambda: proxy)
        mp.setattr(engine, "torch", shim)
        with pytest.raises(_lib.DlsaError) as e:
            wct.RUN[case.family](ctx, **case.params)
        assert e.value.code == wct.DLSA_ERR_WORKSPACE, str(e.value)
        assert proxy.changed == 1 and proxy.entries == [entry]
        assert shim.target and shim.untouched(), "a refused call wrote into its outputs"
        g.check()


@pytest.mark.parametrize("link", bc.LINKS)
@pytest.mark.parametrize("p,icpt", [(5, 0), (130, 1)])
def test_padded_result_pitch(eng, link, p, icpt):
    """one direct call with ldh = pe + 3 into a sentinel-filled buffer: the pe x pe block equals the ldh = pe result bit for bit and the
    pad columns keep the sentinel"""
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _stream
    lib = _lib.load()
    n = 2001
    X, y, o = tgb._data(link, 10 + p, n, p, bool(icpt), True)
    pe = p + icpt
    Xd, yd, od, bd = dev(X), dev(y), dev(o), dev(tgb._away_from_optimum(pe))
    ws = wct._ws(getattr(lib, "dlsa_%s_workspace_bytes" % link), n, p, icpt, 1)
    g, ll = (torch.empty(s, dtype=torch.float64, device="cuda") for s in (pe, 1))
    entry = getattr(lib, "dlsa_%s_pass_f64" % link)
    wct._pitched_pair(lambda H, ldh: entry(_ptr(Xd), p, _ptr(yd), _ptr(od), _ptr(bd), n, p, icpt, _ptr(H), ldh, _ptr(g), _ptr(ll), None,
                                           _ptr(ws), ws.numel(), _stream()), pe)


# ---- the stream contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(BY_ID))
def test_busy_default_stream(eng, orc, api, side, cid):
    """the warm run on the default stream, then the same calls on the side stream while a gate keeps the DEFAULT stream busy, on a
    zero-filled guarded workspace and NaN-filled outputs: the bar, the guards, the warm run's bits, the side stream handed to every
    entry, and a gate that outlived them all"""
    case, ctx = BY_ID[cid], wct.Ctx(eng, orc, api)
    warm, warm_out, timing = tsc._warm_run(case, ctx)
    assert timing.entries == list(case.entries)
    seconds = min(sg.MAX_GATE_SECONDS, max(tsc.MIN_GATE_SECONDS, 3.0 * timing.seconds + timing.between))
    print("stream contract %s: warm run %d entry calls, %.4f s inside them; gate %.2f s" % (cid, len(timing.entries), timing.seconds, seconds))
    seen, out, proxy = tsc._gated_run(case, ctx, side, seconds)
    assert proxy.entries == list(case.entries) and proxy.streams == {side.cuda_stream}
    assert [name for name, _ in seen] == [name for name, _ in warm] and len(seen) == 1
    for (name, a), (_, b) in zip(seen, warm):
        assert same_bits(a, b), "%s: the side-stream run behind a busy default stream differs from the default-stream run" % name


@pytest.mark.parametrize("link", bc.LINKS)
def test_late_inputs_pass(eng, side, link):
    n, p = 2001, 130
    X, y, o = tgb._data(link, 10 + p, n, p, True, True)
    beta = tgb._away_from_optimum(p + 1)
    want, out = tsc._late(side, dict(X=X, y=y, o=o, beta=beta),
                          lambda X, y, o, beta: tgb._pass(eng, link)(X, y, beta, offset=o, fit_intercept=True, want_w=True))
    assert same_bits(out, want)
    assert bool(torch.isfinite(out[2]).all())


@pytest.mark.parametrize("link", bc.LINKS)
def test_late_inputs_fit(eng, side, link):
    rows, K, p = 1001, 3, 5
    for strided in (False, True):                           # strided partitions: their responses and offsets are gathered on the caller's stream
        X, y, o, refs = _fit_case(link, rows, K, p, True, strided)
        ref, late = tsc._late(side, dict(X=X, y=y, o=o), _fit_call(eng, link, rows, K, True, strided))
        _check_fit(late, refs, "late %s step=%d" % (link, K if strided else 1))
        assert same_bits(late, ref)
