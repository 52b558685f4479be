"""Tools of the stream-contract tests (a helper, not a conftest): a gate that keeps a stream busy for a fixed time, a side stream
that provably runs beside the default stream, and an engine.torch stand-in that poisons what the wrappers allocate.

include/dlsa_hip.h promises that every entry point enqueues all its device work on the `stream` it is given and that the entries
which return host scalars synchronise that stream.  On the legacy default stream, with inputs that are ready, a launch on stream 0,
a blocking copy, a fork that does not wait and an early read-back all give the right bits.  They stop doing so when

    gate(default stream, seconds)     a sleeping kernel of fixed length (torch.cuda._sleep, never a spin on a flag) followed by an
                                      event `done`: whatever lands on the default stream now sits behind it,

while the call under test runs on side_stream() and its consumers read at once.  `not done.query()` after the call is the proof
that the gate was still there.  A gate is never longer than MAX_GATE_SECONDS."""
import torch

MAX_GATE_SECONDS = 3.0
CANDIDATES = 8                  # a process has few hardware queues: a new stream may share one with the default stream

_rate = None
_sides, _tried = [], []


def cycles_per_second():
    """torch.cuda._sleep's cycles per second on this device: measured once per session with two events around a short sleep,
    printed, and kept."""
    global _rate
    if _rate is None:
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.cuda._sleep(1000)                                 # (the first launch loads the kernel)
            torch.cuda.synchronize()
            cycles, ms = 2_000_000, 0.0
            for _ in range(8):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda._sleep(cycles)
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
                if ms >= 10.0:
                    break
                cycles *= 4
        assert ms > 0.0, "the sleep kernel took no measurable time"
        _rate = cycles / (ms * 1e-3)
        print("stream_gate: torch.cuda._sleep runs %.4g cycles per second (%d cycles took %.2f ms)" % (_rate, cycles, ms))
    return _rate


def gate(stream, seconds):
    """Enqueue a sleep of `seconds` (at most MAX_GATE_SECONDS) on `stream` and return the event recorded behind it."""
    seconds = min(float(seconds), MAX_GATE_SECONDS)
    assert seconds > 0.0
    cycles = int(seconds * cycles_per_second())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        done = torch.cuda.Event()
        done.record(stream)
    return done


def runs_beside_the_default_stream(side, seconds=0.05):
    """The detector on the test's own buffer, nothing else: with the default stream gated, (1) a fill_(1) queued on the default
    stream is not seen by a clone() on `side`, which completes while the gate is pending, and (2) the same fill queued on `side`
    is seen.  Both are races on `buf` alone; nothing faults.  Returns (unseen, seen): both true for a stream that qualifies."""
    default = torch.cuda.default_stream()
    out = []
    for where in (default, side):
        buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        done = gate(default, seconds)
        with torch.cuda.stream(where):
            buf.fill_(1.0)
        with torch.cuda.stream(side):
            copy = buf.clone()
            side.synchronize()
        pending = not done.query()
        torch.cuda.synchronize()
        want = 0.0 if where is default else 1.0
        out.append(pending and bool((copy == want).all()) and bool((buf == 1.0).all()))
    return tuple(out)


def side_stream(index=0):
    """A torch.cuda.Stream() on which work completes while a gate on the default stream is still running: the first (index 0; the
    second, ...) of up to CANDIDATES new streams that passes runs_beside_the_default_stream().  Too few qualifying is a matter of
    the machine (too few hardware queues for this process): the caller's test fails with this message, it is not worked round."""
    while len(_sides) <= index and len(_tried) < CANDIDATES:
        s = torch.cuda.Stream()
        ok = runs_beside_the_default_stream(s)
        _tried.append(ok)
        if all(ok):
            _sides.append(s)
            print("stream_gate: side stream %d found at candidate %d" % (len(_sides) - 1, len(_tried)))
    assert len(_sides) > index, ("only %d of %d new streams run beside the default stream while it is gated (unseen, seen) = %s: "
                                 "this process has too few hardware queues" % (len(_sides), len(_tried), _tried))
    return _sides[index]


class SideStreamsTorch:
    """`torch` for a module that makes side streams of its own (dlsa_amd.models): torch.cuda.Stream() hands out side_stream(1),
    a stream known to run beside the gated default stream and distinct from the caller's side_stream(0) -- a new stream may share
    its hardware queue with the default stream, and work on it then waits behind the gate however right the code is."""

    class _Cuda:
        def __init__(self, made):
            self._made = made

        def __getattr__(self, name):
            return getattr(torch.cuda, name)

        def Stream(self, *a, **k):
            s = side_stream(1)
            self._made.append(s)
            return s

    def __init__(self):
        self.made = []
        self.cuda = SideStreamsTorch._Cuda(self.made)

    def __getattr__(self, name):
        return getattr(torch, name)


POISON_INT = 77


class PoisonTorch:
    """engine.torch for a gated run: `empty` comes back filled with NaN (floating types) or 77 (integer types), `zeros` stays
    zeros, both filled on the current stream.  An output buffer the allocator hands back would otherwise still hold the identical
    result of the warm run, and a writer that comes late would go unseen."""

    def __init__(self, real=torch):
        self._real = real
        self.made = 0

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *a, **k):
        t = self._real.empty(*a, **k)
        if t.numel():
            t.fill_(float("nan") if t.dtype.is_floating_point else POISON_INT)
        self.made += 1
        return t

    def zeros(self, *a, **k):
        return self._real.zeros(*a, **k)
