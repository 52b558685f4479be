"""GPU: the memory and the stream contract of the C ABI for the entries of the family extension header
include/dlsa_hip_onehot_ordinal.h, which no other contract table reads.  The machinery is that of
tests/test_gpu_workspace_contract.py and tests/test_gpu_stream_contract.py -- the guarded workspace, the gates, the recorders, the
warm and the gated run -- and the two proxies are those of tests/test_gpu_ordinal_contract.py, pointed at
_lib.ONEHOT_ORDINAL_SIGNATURES and at this header; this file brings the cases (tests/onehot_ordinal_contract_cases.py) and the
runners with the bars of tests/test_gpu_onehot_ordinal.py.

Pass and fit at (6001, 2, (5, 4), C = 3) and (6001, 3, (40, 9), C = 8): on a body of exactly the query, filled with 0xFF, between
guards -- DLSA_OK, intact guards, the bars, and the bits of a run on a 0x00 body; ws_bytes - 1 and the pointer + 8 --
DLSA_ERR_WORKSPACE with outputs and guards untouched; on a side stream behind a busy default stream, and with inputs that arrive
late on that side stream."""
import functools

import pytest

import guarded_workspace as gw
import onehot_ordinal_cases as cs
import onehot_ordinal_contract_cases as oc
import stream_gate as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_gpu_onehot_ordinal as tgo                       # noqa: E402  (the pass and fit checks and their bars)
import test_gpu_ordinal_contract as base                    # noqa: E402  (the proxies of an extension header)
import test_gpu_stream_contract as tsc                      # noqa: E402  (the warm and the gated run)
import test_gpu_workspace_contract as wct                   # noqa: E402  (the guarded run, the recorders)
from test_gpu_onehot import _plan                           # noqa: E402
from test_gpu_workspace_contract import eng, orc, api       # noqa: E402,F401  (module-scoped fixtures)

BY_ID = {c.id: c for c in oc.CASES}
rel, same_bits, dev = wct.rel, wct.same_bits, wct.dev


@pytest.fixture(scope="module")
def side():
    assert torch.cuda.is_available()
    sg.side_stream(1)
    return sg.side_stream()


class OnehotOrdinalStreamProxy(tsc.StreamProxy):
    """tsc.StreamProxy that also times, and notes the stream of, the stream-taking entries of this extension header"""

    def __init__(self, lib, before_first=None, after=None):
        super().__init__(lib, before_first, after)
        self._names = self._names | set(oc.stream_entries())


@pytest.fixture(autouse=True)
def _extension_proxies(monkeypatch):
    """base.OrdinalLibProxy looks an entry up in _lib.ORDINAL_SIGNATURES: for this file that table also holds this header's entries;
    the guarded, warm and gated runs of the two contract tests build their proxy by these names"""
    from dlsa_amd import _lib
    monkeypatch.setattr(_lib, "ORDINAL_SIGNATURES", {**_lib.ORDINAL_SIGNATURES, **_lib.ONEHOT_ORDINAL_SIGNATURES})
    monkeypatch.setattr(wct, "LibProxy", base.OrdinalLibProxy)
    monkeypatch.setattr(tsc, "StreamProxy", OnehotOrdinalStreamProxy)
    for table in (wct.RUN, tsc.RUN):
        monkeypatch.setitem(table, "onehot_ordinal_pass", run_pass)
        monkeypatch.setitem(table, "onehot_ordinal_fit", run_fit)


# ---- the runners: the engine calls and the bars of tests/test_gpu_onehot_ordinal.py ----------------------------------------------------
def run_pass(c, n, q, nlevels, C):
    tgo.test_pass_matches_reference(c.api, c.orc, n, q, nlevels, C, True)         # 1e-12, H bitwise symmetric


@functools.lru_cache(maxsize=None)
def _fit_case(n, q, nlevels, C):
    from oracle import dlsa_oracle
    data = cs.fit_case(dlsa_oracle.design_matrix, n, q, nlevels, n + q, C)
    X, y = data[6], data[7]
    assert set(range(C)) <= set(y.astype(int)) and (X != 0).sum(0).min() >= 5
    return data, cs.fit_counted(X, y, C)


def run_fit(c, n, q, nlevels, C):
    (p, num, codes, desc, nl, level_col, X, y), fit = _fit_case(n, q, nlevels, C)
    plan = _plan(c.api, p, desc, nl, level_col)
    r = c.eng.onehot_ordinal_fit_ex(plan, dev(num), dev(codes), dev(y), [0], [n], classes=C)
    tgo._check_fit(r, [fit], 1, (n, q, nlevels, C))                               # 1e-10, the reference's evaluation count


# ---- the memory contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(BY_ID))
def test_contract_at_the_declared_size(eng, orc, api, cid):
    """DLSA_OK, intact guards and the bar on a body of exactly the query filled with 0xFF; the same bits on a body filled with 0x00"""
    case, ctx = BY_ID[cid], wct.Ctx(eng, orc, api)
    seen, g = wct._guarded_run(case, ctx, gw.POISON)
    assert len(g.queries) == 1 and g.queries[0][1] > 0 and g.queries[0][1] % 256 == 0
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


@pytest.mark.parametrize("n,q,nlevels,C", oc.SHAPES)
def test_late_inputs_pass(api, orc, eng, side, n, q, nlevels, C):
    import ordinal_reference as orf
    plan, num, codes, y, theta, X = tgo._pass_inputs(api, orc, n, q, nlevels, C, True)
    want, out = tsc._late(side, dict(num=num, codes=codes, y=y, theta=theta),
                          lambda num, codes, y, theta: eng.onehot_ordinal_pass(plan, num, codes, y, theta, C, want_w=True))
    _, figs = tgo._figures(out, orf.terms(X, y, theta, C), C - 1)
    assert max(figs.values()) <= cs.TOL_PASS, figs
    assert same_bits(out, want)


@pytest.mark.parametrize("n,q,nlevels,C", oc.SHAPES)
def test_late_inputs_fit(api, eng, side, n, q, nlevels, C):
    (p, num, codes, desc, nl, level_col, X, y), fit = _fit_case(n, q, nlevels, C)
    plan = _plan(api, p, desc, nl, level_col)
    K = 3
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    arrays = dict(num=num, codes=codes, y=y)
    whole, out = tsc._late(side, arrays, lambda num, codes, y: eng.onehot_ordinal_fit_ex(plan, num, codes, y, [0], [n], classes=C))
    tgo._check_fit(out, [fit], 1, ("late", n, q, nlevels, C))
    assert same_bits(out, whole)
    # strided partitions: their responses are gathered on the caller's stream
    ref, late = tsc._late(side, arrays, lambda num, codes, y: eng.onehot_ordinal_fit_ex(plan, num, codes, y, first, rows, row_step=K, classes=C))
    assert late["status"] == [0] * K and same_bits(late, ref)
