"""An exactly sized, guarded, poisoned workspace for the engine's calls (a helper, not a conftest).

engine._workspace hands every call at least 1 MiB from a grow-only cache, so a carve that runs past its *_workspace_bytes()
query lands in slack and a region that is read before it is written holds whatever the previous call left.  `guarded(monkeypatch)`
replaces engine._workspace for the length of a test: every request gets its own uint8 tensor

    [ front guard | body: exactly nbytes | back guard ]

and the call sees the body alone, so ws.numel() -- what the engine passes as ws_bytes -- is the query itself.  The guards hold
one byte pattern and are a multiple of 256 bytes of at least 1 MiB each (the slack every call had so far: a call that survives
the suite stays inside the allocation); the body is pre-filled with 0xFF (NaN as a double, -1 as an int, all-ones as a counter)
or, for the bit-for-bit comparison, 0x00.  check() synchronises and reports every damaged guard.  engine._ws_cache is not
touched, and the helper works on CPU tensors (tests/test_guarded_workspace_cpu.py)."""
import sys

import torch

GUARD_BYTES = 1 << 20          # per side; a multiple of 256, so the body keeps the allocation's 256-byte alignment
GUARD_BYTE = 0xA5
POISON = 0xFF

assert GUARD_BYTES % 256 == 0 and GUARD_BYTES >= 1 << 20


class GuardDamaged(AssertionError):
    pass


class Allocation:
    """One request: `buf` the whole tensor, `body` the view the call got, `nbytes` the query value, `caller` the name of the
    function that asked (the engine wrapper)."""

    def __init__(self, buf, body, nbytes, caller):
        self.buf, self.body, self.nbytes, self.caller = buf, body, nbytes, caller

    def damage(self):
        """[(side, first damaged offset, last damaged offset, damaged bytes)]: offsets count from the start of that guard."""
        out = []
        for side, view in (("front", self.buf[:GUARD_BYTES]), ("back", self.buf[GUARD_BYTES + self.nbytes:])):
            bad = torch.nonzero(view != GUARD_BYTE).flatten()
            if bad.numel():
                out.append((side, int(bad[0]), int(bad[-1]), int(bad.numel())))
        return out


class Guarded:
    def __init__(self, fill=POISON):
        self.fill = int(fill)
        self.allocations = []

    def workspace(self, nbytes, device):
        """The replacement of engine._workspace(nbytes, device)."""
        nbytes = int(nbytes)
        buf = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=device)
        body = buf[GUARD_BYTES:GUARD_BYTES + nbytes]
        body.fill_(self.fill)
        assert body.numel() == nbytes and (nbytes == 0 or body.data_ptr() % 256 == buf.data_ptr() % 256)
        self.allocations.append(Allocation(buf, body, nbytes, sys._getframe(1).f_code.co_name))
        return body

    @property
    def queries(self):
        return [(a.caller, a.nbytes) for a in self.allocations]

    def check(self):
        """Synchronise, then assert that every guard byte of every recorded allocation is intact."""
        if any(a.buf.is_cuda for a in self.allocations):
            torch.cuda.synchronize()
        lines = []
        for i, a in enumerate(self.allocations):
            for side, first, last, count in a.damage():
                lines.append("allocation %d (%s, query %d bytes): %s guard damaged, %d bytes, first offset %d, last offset %d%s"
                             % (i, a.caller, a.nbytes, side, count, first, last,
                                " (the front guard ends at offset %d, where the body begins)" % GUARD_BYTES if side == "front"
                                else " (offset 0 is the first byte after the body)"))
        if lines:
            raise GuardDamaged("\n".join(lines))


def guarded(monkeypatch, fill=POISON):
    """Replace dlsa_amd.engine._workspace through pytest's monkeypatch (undone at the end of the test) and return the Guarded
    whose check() the test calls after its engine calls.  fill: the byte the body is pre-filled with (POISON, or 0x00)."""
    from dlsa_amd import engine
    g = Guarded(fill)
    monkeypatch.setattr(engine, "_workspace", g.workspace)
    return g
