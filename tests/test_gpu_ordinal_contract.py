"""GPU: the memory and the stream contract of the C ABI for the entries of the family extension header
(include/dlsa_hip_ordinal.h), which the frozen tables of tests/test_gpu_workspace_contract.py and
tests/test_gpu_stream_contract.py do not read.  The machinery is theirs -- the guarded workspace, the gates, the recorders, the
warm and the gated run --; this file brings the cases (tests/ordinal_contract_cases.py), the runners with the bars of
tests/test_gpu_ordinal.py, and two small proxies that read _lib.ORDINAL_SIGNATURES and the extension header where the existing
ones read _lib.SIGNATURES and include/dlsa_hip.h.

Pass and fit at (6001, 5, 3) and (6001, 40, 8): on a body of exactly the query, filled with 0xFF, between guards -- DLSA_OK, intact
guards, the bars, and the bits of a run on a 0x00 body; ws_bytes - 1 and the pointer + 8 -- DLSA_ERR_WORKSPACE with outputs and
guards untouched; ldh = d + 3 -- the same bits and clean pad columns; on a side stream behind a busy default stream, and with inputs
that arrive late on that side stream."""
import ctypes
import functools

import numpy as np
import pytest

import guarded_workspace as gw
import ordinal_contract_cases as oc
import ordinal_reference as orf
import stream_gate as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_gpu_ordinal as tgo                              # noqa: E402  (the pass check and its bar)
import test_gpu_stream_contract as tsc                      # noqa: E402  (the warm and the gated run)
import test_gpu_workspace_contract as wct                   # noqa: E402  (the guarded run, the recorders)
from test_gpu_workspace_contract import eng, orc, api       # noqa: E402,F401  (module-scoped fixtures)

BY_ID = {c.id: c for c in oc.CASES}
rel, same_bits, dev = wct.rel, wct.same_bits, wct.dev


@pytest.fixture(scope="module")
def side():
    assert torch.cuda.is_available()
    sg.side_stream(1)
    return sg.side_stream()


# ---- the two proxies ----------------------------------------------------------------------------------------------------------------
class OrdinalLibProxy(wct.LibProxy):
    """wct.LibProxy for the entries _lib.ORDINAL_SIGNATURES binds: records the query and the entries that take a workspace and, for
    the refusals, changes the (ws, ws_bytes) pair on its way in -- "short": ws_bytes - 1; "offset": the pointer + 8"""

    def __getattr__(self, name):
        from dlsa_amd import _lib
        sig = _lib.ORDINAL_SIGNATURES.get(name)
        if sig is None:
            return super().__getattr__(name)
        fn = getattr(self._lib, name)
        if name.endswith("_workspace_bytes"):
            def query(*args):
                self.queries.append(name)
                return fn(*args)
            return query
        at = sig[1].index(_lib.c_sz)

        def entry(*args):
            self.entries.append(name)
            args = list(args)
            if self._mode and name == self._only:
                if self._shim is not None:                      # what the wrapper allocated since the previous entry: this call's outputs
                    self._shim.target = list(self._shim.made[self._shim.mark:])
                if self._mode == "short":
                    assert args[at] > 0
                    args[at] = args[at] - 1
                else:
                    args[at - 1] = ctypes.c_void_p(args[at - 1].value + 8)
                self.changed += 1
            try:
                return fn(*args)
            finally:
                if self._shim is not None:
                    self._shim.mark = len(self._shim.made)
        return entry


class OrdinalStreamProxy(tsc.StreamProxy):
    """tsc.StreamProxy that also times, and notes the stream of, the stream-taking entries of the extension header"""

    def __init__(self, lib, before_first=None, after=None):
        super().__init__(lib, before_first, after)
        self._names = self._names | set(oc.stream_entries())


@pytest.fixture(autouse=True)
def _extension_proxies(monkeypatch):
    """the guarded, warm and gated runs of the two contract tests build their proxy by these names"""
    monkeypatch.setattr(wct, "LibProxy", OrdinalLibProxy)
    monkeypatch.setattr(tsc, "StreamProxy", OrdinalStreamProxy)
    monkeypatch.setitem(wct.RUN, "ordinal_pass", run_ordinal_pass)
    monkeypatch.setitem(wct.RUN, "ordinal_fit", run_ordinal_fit)
    monkeypatch.setitem(tsc.RUN, "ordinal_pass", run_ordinal_pass)
    monkeypatch.setitem(tsc.RUN, "ordinal_fit", run_ordinal_fit)


# ---- the runners: the engine calls and the bars of tests/test_gpu_ordinal.py ------------------------------------------------------------
def run_ordinal_pass(c, n, p, C):
    X, y, theta, ref = tgo._pass_case(n, p, C)
    tgo._check_pass(c.eng, X, y, theta, C, ref)                 # test_pass_matches_reference: 1e-12, H bitwise symmetric


@functools.lru_cache(maxsize=None)
def _fit_case(n, p, C):
    X, y = orf.data(40 + p, n, p, C)
    return X, y, orf.fit(X, y, C)


def _check_fit(r, b, S, ll, what):
    assert r["status"] == [0] and r["rc"] == 0                  # test_fit_matches_reference: 1e-10
    errs = {"coef": rel(r["coef"][0].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][0].cpu().numpy(), S),
            "Sig_invMcoef": rel(r["Sig_invMcoef"][0].cpu().numpy(), S @ b), "ll": abs(r["loglik"][0] - ll) / abs(ll)}
    print("ordinal fit %s: %d evaluations %s" % (what, r["n_iter"][0], " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-10 for v in errs.values()), errs
    Sn = r["Sig_inv"][0].cpu().numpy()
    assert np.array_equal(Sn, Sn.T)


def run_ordinal_fit(c, n, p, C):
    X, y, (b, S, ll, n_iter) = _fit_case(n, p, C)
    r = tgo._fit(c.eng, X, y, [0, n], C)
    _check_fit(r, b, S, ll, "n=%d p=%d C=%d (reference %d evaluations)" % (n, p, C, n_iter))
    assert abs(r["n_iter"][0] - n_iter) <= 1


# ---- the memory contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(BY_ID))
def test_contract_at_the_declared_size(eng, orc, api, cid):
    """DLSA_OK, intact guards and the bar on a body of exactly the query filled with 0xFF; the same bits on a body filled with 0x00"""
    case, ctx = BY_ID[cid], wct.Ctx(eng, orc, api)
    seen, g = wct._guarded_run(case, ctx, gw.POISON)
    n, p, C = (case.params[k] for k in ("n", "p", "C"))
    from dlsa_amd import _lib
    assert [q for _, q in g.queries] == [_lib.load().dlsa_ordinal_workspace_bytes(n, p, C, 1)]
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
        proxy = OrdinalLibProxy(_lib.load(), mode, only=entry, shim=shim)
        mp.setattr(_lib, "load", lambda: proxy)
        mp.setattr(engine, "torch", shim)
        with pytest.raises(_lib.DlsaError) as e:
            wct.RUN[case.family](ctx, **case.params)
        assert e.value.code == wct.DLSA_ERR_WORKSPACE, str(e.value)
        assert proxy.changed == 1 and proxy.entries == [entry]
        assert shim.target and shim.untouched(), "a refused call wrote into its outputs"
        g.check()


@pytest.mark.parametrize("n,p,C", [(6001, 5, 3), (6001, 40, 8), (3001, 257, 5)])
def test_padded_result_pitch(eng, n, p, C):
    """one direct call with ldh = d + 3 into a sentinel-filled buffer: the d x d block equals the ldh = d result bit for bit and the
    pad columns keep the sentinel (the Gram writes at row J, column J of H; the assembly writes the borders and the corner)"""
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _stream
    lib = _lib.load()
    X, y, theta, _ = tgo._pass_case(n, p, C)
    d = C - 1 + p
    Xd, yd, td = dev(X), dev(y), dev(theta)
    ws = wct._ws(lib.dlsa_ordinal_workspace_bytes, n, p, C, 1)
    g, ll = (torch.empty(s, dtype=torch.float64, device="cuda") for s in (d, 1))
    wct._pitched_pair(lambda H, ldh: lib.dlsa_ordinal_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(td), C, n, p, _ptr(H), ldh, _ptr(g), _ptr(ll), None,
                                                               _ptr(ws), ws.numel(), _stream()), d)


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


@pytest.mark.parametrize("n,p,C", [(6001, 5, 3), (6001, 40, 8)])
def test_late_inputs_pass(eng, side, n, p, C):
    X, y, theta, ref = tgo._pass_case(n, p, C)
    want, out = tsc._late(side, dict(X=X, y=y, theta=theta), lambda X, y, theta: eng.ordinal_pass(X, y, theta, C, want_w=True))
    llr, gr, Hr, wr = ref
    errs = [abs(out[2].item() - llr) / abs(llr), rel(out[1].cpu().numpy(), gr), rel(out[0].cpu().numpy(), Hr), rel(out[3].cpu().numpy(), wr)]
    assert max(errs) <= 1e-12, errs
    assert same_bits(out, want)


@pytest.mark.parametrize("n,p,C", [(6001, 5, 3), (6001, 40, 8)])
def test_late_inputs_fit(eng, side, n, p, C):
    X, y, (b, S, ll, _) = _fit_case(n, p, C)
    K = 3
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    whole, out = tsc._late(side, dict(X=X, y=y), lambda X, y: eng.ordinal_fit_ex(X, y, [0], [n], classes=C))
    _check_fit(out, b, S, ll, "late n=%d p=%d C=%d" % (n, p, C))
    assert same_bits(out, whole)
    # strided partitions: their responses are gathered on the caller's stream
    ref, late = tsc._late(side, dict(X=X, y=y), lambda X, y: eng.ordinal_fit_ex(X, y, first, rows, row_step=K, classes=C))
    assert late["status"] == [0] * K and same_bits(late, ref)
