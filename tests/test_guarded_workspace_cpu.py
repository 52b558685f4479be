"""CPU: the guarded workspace (tests/guarded_workspace.py) catches what it is there to catch, and the table of the contract
test (tests/workspace_contract_cases.py) names every *_workspace_bytes query include/dlsa_hip.h declares."""
import os
import re

import pytest

import guarded_workspace as gw
import workspace_contract_cases as wc

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _one(monkeypatch, nbytes=1000, fill=gw.POISON):
    from dlsa_amd import engine
    cache = dict(engine._ws_cache)
    g = gw.guarded(monkeypatch, fill=fill)
    body = engine._workspace(nbytes, CPU)                  # what an engine wrapper does
    assert engine._ws_cache == cache                       # the engine's own cache is not touched
    return g, body


def test_body_is_exactly_the_query_aligned_and_poisoned(monkeypatch):
    g, body = _one(monkeypatch, 1000)
    a = g.allocations[0]
    assert body.numel() == 1000 and body.dtype == torch.uint8 and bool((body == 0xFF).all())
    assert gw.GUARD_BYTES >= 1 << 20 and gw.GUARD_BYTES % 256 == 0
    assert a.buf.numel() == 1000 + 2 * gw.GUARD_BYTES and body.data_ptr() == a.buf.data_ptr() + gw.GUARD_BYTES
    assert bool((a.buf[:gw.GUARD_BYTES] == gw.GUARD_BYTE).all()) and bool((a.buf[gw.GUARD_BYTES + 1000:] == gw.GUARD_BYTE).all())
    assert g.queries == [("_one", 1000)]                   # the query value and the caller's name
    # NaN as a double, -1 as an int
    assert bool(torch.isnan(body[:992].view(torch.float64)).all()) and bool((body[:992].view(torch.int32) == -1).all())
    g.check()


def test_zero_fill_is_selectable_and_an_empty_body_works(monkeypatch):
    g, body = _one(monkeypatch, 512, fill=0x00)
    assert bool((body == 0).all())
    from dlsa_amd import engine
    assert engine._workspace(0, CPU).numel() == 0
    g.check()


def test_untouched_and_body_writes_pass(monkeypatch):
    g, body = _one(monkeypatch)
    body.fill_(3)                                          # the whole body is the call's to write
    g.check()


@pytest.mark.parametrize("where,side,offset", [("before", "front", gw.GUARD_BYTES - 1), ("after", "back", 0), ("last", "back", gw.GUARD_BYTES - 1)])
def test_one_damaged_guard_byte_is_reported(monkeypatch, where, side, offset):
    """one byte just before the body, one just after it, and the last guard byte of all"""
    g, body = _one(monkeypatch, 1000)
    buf = g.allocations[0].buf
    at = {"before": gw.GUARD_BYTES - 1, "after": gw.GUARD_BYTES + 1000, "last": buf.numel() - 1}[where]
    buf[at] = 0
    with pytest.raises(gw.GuardDamaged) as e:
        g.check()
    msg = str(e.value)
    assert "%s guard damaged, 1 bytes, first offset %d, last offset %d" % (side, offset, offset) in msg and "query 1000 bytes" in msg


def test_every_allocation_is_checked_and_a_run_of_bytes_gives_first_and_last(monkeypatch):
    from dlsa_amd import engine
    g, _ = _one(monkeypatch, 256)
    engine._workspace(4096, CPU)
    g.allocations[1].buf[gw.GUARD_BYTES + 4096 + 8: gw.GUARD_BYTES + 4096 + 24] = 1
    with pytest.raises(gw.GuardDamaged, match=r"allocation 1 \(.*query 4096 bytes\): back guard damaged, 16 bytes, first offset 8, last offset 23"):
        g.check()


def test_monkeypatch_restores_the_engine(monkeypatch):
    from dlsa_amd import engine
    orig = engine._workspace
    with pytest.MonkeyPatch.context() as mp:
        gw.guarded(mp)
        assert engine._workspace is not orig
    assert engine._workspace is orig


# ---- coverage cannot rot ------------------------------------------------------------------------------------------------------
def _declared_queries():
    with open(os.path.join(ROOT, "include", "dlsa_hip.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"^\s*size_t\s+(dlsa_\w+_workspace_bytes)\s*\(", text, re.M)))


def test_every_declared_query_is_named_by_a_case():
    declared = _declared_queries()
    from dlsa_amd import _lib
    # (the parse finds what the binding binds: a declaration the pattern misses would fail here, not pass unnoticed)
    assert declared == sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")) and len(declared) >= 29
    named = {q for c in wc.CASES for q in c.queries + c.also}
    missing = [q for q in declared if q not in named]
    assert not missing, "no case of tests/workspace_contract_cases.py names %s" % missing
    assert not sorted(named - set(declared)), sorted(named - set(declared))


def test_the_table_is_well_formed():
    from dlsa_amd import _lib
    assert len({c.id for c in wc.CASES}) == len(wc.CASES)
    for c in wc.CASES:
        assert c.entries and c.queries and c.refuse in ("query", "chains1", "need"), c.id
        for e in c.entries:                                # an entry the binding declares, and one that takes a workspace
            assert e in _lib.SIGNATURES and _lib.c_sz in _lib.SIGNATURES[e][1], (c.id, e)
