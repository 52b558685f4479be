"""GPU: the stream contract of the C ABI (include/dlsa_hip.h: all device work is enqueued on `stream`; functions that return host
scalars synchronise that stream), entry by entry, on a side stream.

Every other GPU test runs on the legacy default stream with inputs that were uploaded and synchronised before the call.  There a
launch or memset on stream 0, a blocking copy where an asynchronous copy and a synchronise of `stream` were meant, a chain stream
that does not wait for the caller's queued work and a host read-back taken before `stream` has finished all give the right bits.

test_busy_default_stream: every selected case of tests/stream_contract_cases.py (the workspace table's cases, thinned of
duplicates, and the entries that table cannot name) runs once on the default stream -- the warm run: results recorded, caches and
plans warmed, its entry calls timed -- and once more on side_stream() while a gate (tests/stream_gate.py) keeps the DEFAULT
stream busy.  Work that lands on the default stream sits behind the gate while its consumers on the side stream run at once, on a
fresh zero-filled guarded workspace and on outputs pre-filled with NaN / 77 (PoisonTorch).  The runner's own bar must pass, the
guards be intact, the bits equal the warm run's where the entry is bit-reproducible, every entry have been handed the side stream,
and the gate have outlived every entry -- a condition: a gate that ended early proved nothing and fails the test.

    The gate goes up when the case makes its first entry call (its uploads and host references before that do not touch the
    default stream) and lasts three times the warm run's summed entry time plus the host time the warm run spent between its first
    entry's call and its last entry's return, at least 0.25 s and at most stream_gate.MAX_GATE_SECONDS.
    torch.cuda.synchronize() inside the existing helpers means "my work is done": for the length of the gated run it synchronises
    the current (side) stream, which is what the contract says is enough.
    engine.OnehotPlan is built once per design and shared by both runs: dlsa_onehot_plan_create / _destroy take no stream, upload
    with blocking copies and free device memory, which both wait for the default stream ("Streams").
    The Python drivers that fork (fit_linear_streaming, fit_linear_chunks) get their torch.cuda.Stream() from stream_gate too: a new
    stream may share its hardware queue with the default stream, and then waits behind the gate however right the code is.

test_late_inputs_*: the fork that fails to wait.  The test owns the device inputs: NaN (floating) or 0 (integer: codes and sort
orders, so that an early reader stays inside its arrays) until, on the side stream and behind a 0.3 s gate ON that stream, a copy_
brings the true values; the call follows at once.  Status and results equal the default-stream run bit for bit where the entry
is bit-reproducible and otherwise meet its existing bar.

test_detector_*: the detector on the test's own buffer (what side_stream() runs to qualify a stream)."""
import functools
import gc
import time

import numpy as np
import pytest

import guarded_workspace as gw
import stream_contract_cases as sc
import stream_gate as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_gpu_workspace_contract as wct        # noqa: E402  (the runners, bars and recorders of the workspace-contract test)
from test_gpu_workspace_contract import eng, orc, api        # noqa: E402,F401  (module-scoped fixtures)

MIN_GATE_SECONDS, LATE_GATE_SECONDS = 0.25, 0.3
CASES = {c.id: c for c in sc.SELECTED}
CASES.update({x.id: x for x in sc.EXTRA})
assert len(CASES) == len(sc.SELECTED) + len(sc.EXTRA)

dev, rel, same_bits = wct.dev, wct.rel, wct.same_bits


@pytest.fixture(scope="module")
def side():
    assert torch.cuda.is_available()
    print("stream contract: %d cases (%d of the workspace table's %d, %d extra)" % (len(CASES), len(sc.SELECTED), len(wct.CASES), len(sc.EXTRA)))
    sg.side_stream(1)                                           # (qualified now: no gate is up yet)
    return sg.side_stream()


# ---- the runners of the extra cases: the engine calls and the bar of the entry's existing test; what they return is compared ----
RUN = dict(wct.RUN)
SEED, ROW0 = 20260101, 12345678901


def runner(name):
    def deco(f):
        assert name not in RUN
        RUN[name] = f
        return f
    return deco


def _tdt(dtype):
    return torch.float64 if dtype == "f64" else torch.float32


@runner("synth")
def run_synth(c, n, p, dtype):
    X, y = c.eng.synth(SEED, ROW0, n, p, kind=c.eng.SYNTH_UNIFORM, dtype=_tdt(dtype))
    Xo, yo = c.orc.synth_logistic(SEED, ROW0, n, p, c.orc.SYNTH_UNIFORM)
    Xg = X.cpu().numpy()
    # tests/test_gpu_kernels.py: test_synth_rows_bit_identical_to_oracle (the fp32 rows are the same doubles, rounded once)
    assert Xg.dtype == (np.float64 if dtype == "f64" else np.float32) and np.array_equal(Xg, Xo.astype(Xg.dtype))
    assert np.mean(y.cpu().numpy() != yo) < 1e-3
    return X, y


@runner("synth_response")
def run_synth_response(c, n, p, dtype):
    X, _ = c.eng.synth(SEED, 100, n, p, kind=c.eng.SYNTH_UNIFORM, labels=False, dtype=_tdt(dtype))
    y = c.eng.synth_response(SEED, 100, X, sigma=0.5)
    Xo, yo = c.orc.synth_linear(SEED, 100, n, p, c.orc.SYNTH_UNIFORM, sigma=0.5)
    assert np.array_equal(X.cpu().numpy(), Xo.astype(np.float64 if dtype == "f64" else np.float32))
    assert rel(y.cpu().numpy(), yo) < (1e-12 if dtype == "f64" else 1e-6)          # tests/test_gpu_linear.py: test_synth_response_matches_oracle
    return X, y


@runner("synth_linear32")
def run_synth_linear32(c, n, p):
    X, y = c.eng.synth_linear32(424242, ROW0, n, p, sigma=0.7)
    Xo, yo = c.orc.synth_linear32(424242, ROW0, n, p, sigma=0.7)
    Xg = X.cpu().numpy()                                        # tests/test_gpu_linear.py: test_synth_linear32_matches_oracle_restatement
    assert Xg.shape == Xo.shape and np.max(np.abs(Xg - Xo)) < 3e-6
    yref = Xg.astype(np.float64) @ c.orc.true_beta(p) + (yo.astype(np.float64) - Xo.astype(np.float64) @ c.orc.true_beta(p))
    assert np.max(np.abs(y.cpu().numpy() - yref)) < 2e-5 * max(1.0, np.sqrt(p))
    return X, y


@runner("design")
def run_design(c, n, q, f, p):
    import test_gpu_design as td
    td.test_design_kernel_bit_exact(c.api, c.orc, n, q, f, p)


@functools.lru_cache(maxsize=None)
def _blocks(K, p):
    rng = np.random.default_rng(K * 100 + p)
    return rng.standard_normal((K, p)), rng.standard_normal((K, p)), rng.standard_normal((K, p, p))


def _sum_in_order(a, mask):
    s = np.zeros(a.shape[1:])
    for k in range(a.shape[0]):                                 # the kernel's fixed order: k = 0 .. K - 1, one fp64 add each
        if not mask[k]:
            s = s + a[k]
    return s.reshape(-1)


@runner("sum_blocks")
def run_sum_blocks(c, K, p):
    """the rank's message against the same sums taken in the kernel's order on the host: bit for bit, unmasked and with a mask
    (whose device copy is a stream-ordered allocation of the entry's own)"""
    coef, smc, sig = _blocks(K, p)
    out = []
    for mask in (None, [0, 1, 0, 0, 1, 0, 0][:K]):
        msg = c.eng.sum_blocks(dev(coef), dev(smc), dev(sig), mask=mask)
        m = mask or [0] * K
        want = np.concatenate([_sum_in_order(sig, m), _sum_in_order(smc, m), _sum_in_order(coef, m)])
        assert np.array_equal(msg.cpu().numpy().view(np.uint64), want.view(np.uint64))
        out.append(msg)
    return out


@runner("negbin_special")
def run_negbin_special(c):
    import test_gpu_negbin as tn
    tn.test_special_functions(c.eng)
    th, yy = np.meshgrid(np.logspace(-2, 6, 33), np.array([0.0, 1.0, 2.0, 10.0, 1e3, 1e6]), indexing="ij")
    return c.eng.negbin_special(dev(th.ravel()), dev(yy.ravel()))


@runner("sym_pinv_probe")
def run_sym_pinv_probe(c, kind, p):
    import pinv_reference as pv
    import test_gpu_pinv_solve as tp
    cs = pv.case(kind, p)
    theta, rank, eig, sweeps, V = tp.probe(c.eng, cs["S"], cs["v"])
    fr = pv.fractions(cs, eig, V, theta)                      # tests/test_gpu_pinv_solve.py: test_decomposition_and_solve
    assert rank == cs["rank"] and 0 < sweeps <= 40 and max(fr.values()) <= 1.0, (rank, sweeps, fr)
    return theta.tolist(), rank, eig.tolist(), sweeps, V.tolist()


def _blocks_of(mb):
    assert mb.status == [0] * len(mb.status), mb.status
    return mb.coef, mb.Sig_inv, mb.Sig_invMcoef, list(mb.loglik)


@runner("fit_linear_streaming")
def run_fit_linear_streaming(c, rows, p, chunks):
    """the generator's side stream (overlap: chunk i + 1 is generated while chunk i is consumed on the caller's stream)"""
    n = rows * chunks
    mb = c.api.fit_linear_streaming(n, p, partition_num=1, chunk_rows=rows, seed=SEED, kind="gaussian32", fit_intercept=True, overlap=True)
    out = c.api.dlsa_mapred(mb)
    truth = np.concatenate([[0.0], c.orc.true_beta(p)])
    assert float(np.max(np.abs(out["beta_byOLS"].to_numpy() - truth))) < 0.1         # tests/test_gpu_linear.py: the streaming tests
    return _blocks_of(mb)


@functools.lru_cache(maxsize=None)
def _host_chunks(rows, p, chunks):
    from oracle import dlsa_oracle as o
    n = rows * chunks
    X, y = o.synth_linear(SEED + 6, 0, n, p, o.SYNTH_UNIFORM)
    Xh, yh = X.astype(np.float32), y.astype(np.float32)
    A = np.hstack([np.ones((n, 1)), Xh.astype(np.float64)])
    pinned = [(torch.from_numpy(Xh[i * rows:(i + 1) * rows].copy()).pin_memory(), torch.from_numpy(yh[i * rows:(i + 1) * rows].copy()).pin_memory())
              for i in range(chunks)]
    return pinned, A.T @ A, A.T @ yh.astype(np.float64)


@runner("fit_linear_chunks")
def run_fit_linear_chunks(c, rows, p, chunks):
    """the copy stream (pinned host chunks: the copy of chunk i + 1 runs beside the kernels of chunk i)"""
    pinned, AtA, Aty = _host_chunks(rows, p, chunks)
    mb = c.api.fit_linear_chunks(((0, X, y) for X, y in pinned), p, partition_num=1, fit_intercept=True)
    assert mb.sample_size == rows * chunks
    assert rel(mb.Sig_inv[0].cpu().numpy(), AtA) < 2e-6 and rel(mb.Sig_invMcoef[0].cpu().numpy(), Aty) < 2e-5      # tests/test_gpu_linear.py
    return _blocks_of(mb)


for _x in sc.EXTRA:
    assert _x.family in RUN, _x.family


# ---- what the library saw, and when ------------------------------------------------------------------------------------------------
class StreamProxy:
    """Stands in front of libdlsa_hip.so: times every entry that takes a stream, notes the stream it was handed, and calls
    `before_first` ahead of the first of them and `after(name)` when each returns."""

    def __init__(self, lib, before_first=None, after=None):
        self._lib, self._before_first, self._after = lib, before_first, after
        self._names = set(sc.stream_entries())
        self.entries, self.streams, self.seconds, self.first_call, self.last_return = [], set(), 0.0, None, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._names:
            return fn

        def entry(*args):
            if self.first_call is None:
                if self._before_first is not None:
                    self._before_first()
                self.first_call = time.perf_counter()
            self.entries.append(name)
            self.streams.add(getattr(args[-1], "value", args[-1]) or 0)
            t0 = time.perf_counter()
            try:
                return fn(*args)
            finally:
                self.last_return = time.perf_counter()
                self.seconds += self.last_return - t0
                if self._after is not None:
                    self._after(name)
        return entry

    @property
    def between(self):
        """host time between the first entry's call and the last entry's return that was not spent inside an entry"""
        return 0.0 if self.first_call is None else max(0.0, self.last_return - self.first_call - self.seconds)


_PLANS = {}


def _shared_plans(mp):
    """engine.OnehotPlan, one per design for the whole module (kept alive: none is destroyed while a gate is up)"""
    from dlsa_amd import engine
    real = engine.OnehotPlan

    def plan(p, *arrays):
        key = (int(p),) + tuple(np.asarray(a, dtype=np.float64).tobytes() for a in arrays)
        if key not in _PLANS:
            _PLANS[key] = real(p, *arrays)
        return _PLANS[key]
    mp.setattr(engine, "OnehotPlan", plan)


def _run(case, ctx):
    """the case's engine calls and bar; what an extra case's runner returns is compared bit for bit as well"""
    return RUN[case.family](ctx, **case.params)


def _warm_run(case, ctx):
    from dlsa_amd import _lib, engine
    with pytest.MonkeyPatch.context() as mp:
        _shared_plans(mp)
        proxy = StreamProxy(_lib.load())
        mp.setattr(_lib, "load", lambda: proxy)
        seen = wct.record_results(mp, engine)
        out = _run(case, ctx)
        torch.cuda.synchronize()
    assert set(case.entries) <= set(proxy.entries), (case.entries, sorted(set(proxy.entries)))
    assert 0 in proxy.streams and (proxy.streams == {0} or _own_streams(case)), "the warm run is the default-stream run"
    return seen, out, proxy


def _own_streams(case):
    """the Python drivers that fork onto a side stream of their own: some of their entries are handed that stream by design"""
    return case.family.startswith("fit_linear")


def _gated_run(case, ctx, side, seconds):
    from dlsa_amd import _lib, engine, models
    real_sync = torch.cuda.synchronize
    state = {}
    forks = sg.SideStreamsTorch()

    def raise_gate():
        state["done"] = sg.gate(torch.cuda.default_stream(), seconds)

    def still_gated(name):
        if state["done"].query():
            state.setdefault("early", name)

    gc.collect()
    real_sync()
    try:
        with pytest.MonkeyPatch.context() as mp:
            _shared_plans(mp)
            g = gw.guarded(mp, fill=0x00)
            mp.setattr(engine, "torch", sg.PoisonTorch())
            mp.setattr(models, "torch", forks)
            mp.setattr(torch.cuda, "synchronize", lambda *a, **k: torch.cuda.current_stream().synchronize())
            proxy = StreamProxy(_lib.load(), before_first=raise_gate, after=still_gated)
            mp.setattr(_lib, "load", lambda: proxy)
            seen = wct.record_results(mp, engine)
            with torch.cuda.stream(side):
                out = _run(case, ctx)
                side.synchronize()
    finally:
        real_sync()
    g.check()
    assert "done" in state, "the case made no entry call"
    assert "early" not in state, ("gate too short: the %.2f s gate on the default stream had ended when %s returned -- the run proved nothing "
                                  "(or the entry waited for the default stream)" % (seconds, state["early"]))
    allowed = {side.cuda_stream} | {s.cuda_stream for s in forks.made}
    assert side.cuda_stream in proxy.streams <= allowed, "an entry was handed another stream than the current one: %s" % sorted(proxy.streams)
    assert bool(forks.made) == _own_streams(case)
    assert set(case.entries) <= set(proxy.entries), (case.entries, sorted(set(proxy.entries)))
    return seen, out, proxy


@pytest.mark.parametrize("cid", list(CASES))
def test_busy_default_stream(eng, orc, api, side, cid):
    case, ctx = CASES[cid], wct.Ctx(eng, orc, api)
    warm, warm_out, timing = _warm_run(case, ctx)
    seconds = min(sg.MAX_GATE_SECONDS, max(MIN_GATE_SECONDS, 3.0 * timing.seconds + timing.between))
    print("stream contract %s: warm run %d entry calls, %.4f s inside them, %.4f s between; gate %.2f s"
          % (cid, len(timing.entries), timing.seconds, timing.between, seconds))
    seen, out, proxy = _gated_run(case, ctx, side, seconds)
    print("stream contract %s: gate outlived the call (%d entry calls on the side stream, %.4f s inside them)" % (cid, len(proxy.entries), proxy.seconds))
    assert [n for n, _ in seen] == [n for n, _ in warm]
    if case.bits:
        for (name, a), (_, b) in zip(seen, warm):
            assert same_bits(a, b), "%s: the side-stream run behind a busy default stream differs from the default-stream run" % name
        assert same_bits(out, warm_out), "the side-stream run behind a busy default stream differs from the default-stream run"


# ---- late inputs behind a gate on the side stream -------------------------------------------------------------------------------------
def _late(side, arrays, call):
    """(default-stream result, late result): `arrays` {name: numpy array or device tensor} are the device inputs of call(**tensors).
    The late run's inputs hold NaN / 0 until a copy_ on the side stream, behind a gate on that stream, brings the true values."""
    from dlsa_amd import engine
    ready = {k: (v if torch.is_tensor(v) else dev(v)) for k, v in arrays.items()}
    ref = call(**ready)
    late = {k: (torch.full_like(t, float("nan")) if t.dtype.is_floating_point else torch.zeros_like(t)) for k, t in ready.items()}
    torch.cuda.synchronize()
    try:
        with pytest.MonkeyPatch.context() as mp, torch.cuda.stream(side):
            mp.setattr(engine, "torch", sg.PoisonTorch())
            done = sg.gate(side, LATE_GATE_SECONDS)
            for k, t in late.items():
                t.copy_(ready[k])
            assert not done.query(), "the gate on the side stream had ended before the call: the inputs were not late"
            out = call(**late)
            side.synchronize()
    finally:
        torch.cuda.synchronize()
    return ref, out


@pytest.mark.parametrize("n,p", [(8193, 50), (32771, 300), (65537, 500)])
def test_late_inputs_gram(eng, orc, side, n, p):
    """(32771 x 300 keeps pacing counts in the workspace; Gram sums are not bit-reproducible across runs: the existing bar)"""
    import test_gpu_kernels as tk
    buf, w = wct._gram_data(n, p, p)
    Ho = orc.gram(buf, w)
    _, H = _late(side, dict(X=buf, w=w), lambda X, w: eng.gram(X, w))
    H = H.cpu().numpy()
    print("late gram", (n, p), eng.gram_last_kernel()[0], rel(H, Ho))
    assert rel(H, Ho) < tk.TOL_KERNEL and np.array_equal(H, H.T)


def test_late_inputs_irls_pass(eng, orc, side):
    n, p = 8192, 50
    X, y = orc.synth_logistic(300 + p, 0, n, p, orc.SYNTH_GAUSSIAN)
    beta = orc.true_beta(p) * 0.8 + 0.05 * np.random.default_rng(p).standard_normal(p)
    ref, out = _late(side, dict(X=X, y=y, beta=beta), lambda X, y, beta: eng.irls_pass(X, y, beta, want_w=True))
    assert eng.gram_last_kernel()[0].startswith("irls_pass_narrow_kernel")
    wo, go, llo = orc.logit_pass(X, y, beta)
    assert rel(out[3].cpu().numpy(), wo) < 1e-12 and rel(out[0].cpu().numpy(), orc.gram(X, wo)) < 1e-12
    assert same_bits(out, ref)


def test_late_inputs_logit_pass(eng, orc, side):
    X, y, beta, X1 = wct._logit_data(4099, 121, False)
    _, (w, g, ll) = _late(side, dict(X=X, y=y, beta=beta), lambda X, y, beta: eng.logit_pass(X, y, beta))
    wo, go, llo = orc.logit_pass(X1, y, beta)                   # tests/test_gpu_kernels.py: test_logit_pass_matches_oracle
    assert rel(w.cpu().numpy(), wo) < 1e-12 and rel(g.cpu().numpy(), go) < 1e-11 and abs(ll.item() - llo) < 1e-12 * abs(llo)


# (driver 0 deals the partitions to S = min(chains, (K - 1) / 2) chains: K = 3 runs one chain on the caller's stream; K = 9 under
#  chains = 2 with the other two drivers switched off is the smallest table shape that forks onto a stream of the library's own)
@pytest.mark.parametrize("tag,K,rows,p,options,driver", [
    ("chains", 3, 70001, 40, dict(chains=2), 0),
    ("chains-forked", 9, 2000, 8, dict(chains=2, small=False, batched=False), 0),
    ("lock-step", 9, 2000, 64, dict(batched=True), 2),
    ("one-launch", 300, 200, 16, dict(small=True), 1)])
def test_late_inputs_irls_fit(eng, orc, side, tag, K, rows, p, options, driver):
    X, y = wct._irls_rows(K, rows, p)[:2]
    offs = [k * rows for k in range(K + 1)]
    paths = []

    def call(X, y):
        with eng.irls_options(**options):
            r = eng.irls_fit(X, y, offs)
        paths.append(eng.irls_last_fit_path())
        return r
    ref, out = _late(side, dict(X=X, y=y), call)
    assert paths == [driver, driver], paths
    wct._check_logistic("late irls_fit %s" % tag, out, wct._irls_blocks(K, rows, p, False, False), eng)
    assert same_bits(out, ref)


def test_late_inputs_onehot_irls_fit(eng, orc, side):
    n, q, nlevels = 30000, 4, (9, 5, 30)
    plan, X, y, dn, dc, dy = wct._onehot_logistic(n, q, nlevels)
    offs = [0, n // 4, n // 4, 5 * n // 8, n]
    ref, out = _late(side, dict(num=dn, codes=dc, y=dy), lambda num, codes, y: eng.onehot_irls_fit(plan, num, codes, y, offs))
    assert out["status"] == [0, 4, 0, 0], out["status"]
    blocks = wct._onehot_blocks(n, q, nlevels, tuple((offs[k], offs[k + 1], 1) for k in (0, 2, 3)))
    keep = {k: out[k][[0, 2, 3]] for k in ("coef", "Sig_inv", "Sig_invMcoef")}
    keep["status"] = [0, 0, 0]
    wct._check_logistic("late onehot_irls_fit", keep, blocks, eng, dense=False)
    assert same_bits(out, ref)


def test_late_inputs_cox_fit(eng, orc, side):
    import cox_strata_cases as cases
    n, p = 5003, 7
    X, t, ev, codes, offs, refs = wct._cox_fit_case(n, p, "efron", True)
    arrays = dict(X=X, t=t, ev=ev, order=cases.sort_order(t, codes, offs), strata=np.ascontiguousarray(codes))
    ref, out = _late(side, arrays, lambda X, t, ev, order, strata: eng.cox_fit(X, t, ev, order, offs, ties="efron", strata=strata))
    assert out["status"] == [0, 4, 0], out["status"]
    for k, (b, H, ll) in refs.items():                          # tests/test_gpu_cox_strata.py: test_fit_matches_reference
        assert max(rel(out["coef"][k].cpu().numpy(), b), rel(out["Sig_inv"][k].cpu().numpy(), H), abs(out["loglik"][k] - ll) / abs(ll)) <= 1e-10
    assert same_bits(out, ref)


def test_late_inputs_poisson_fit_ex(eng, orc, side):
    rows, K, p = 4001, 3, 130
    X, y, o, refs = wct._count_fit_case("poisson", rows, K, p, True, True)
    ref, out = _late(side, dict(X=X, y=y, o=o),
                     lambda X, y, o: eng.poisson_fit_ex(X, y, list(range(K)), [rows] * K, row_step=K, offset=o, fit_intercept=True))
    assert out["status"] == [0] * K, out["status"]
    for k, r in enumerate(refs):                                # tests/test_gpu_poisson.py: test_fit_matches_reference
        b, H, ll = r[:3]
        assert max(rel(out["coef"][k].cpu().numpy(), b), rel(out["Sig_inv"][k].cpu().numpy(), H), abs(out["loglik"][k] - ll) / abs(ll)) <= 1e-10
    assert same_bits(out, ref)


def test_late_inputs_multinomial_fit(eng, orc, side):
    n, p, C = 6001, 5, 3
    X, y, (b, S, ll, _) = wct._multinomial_fit_case(n, p, C, True)
    ref, out = _late(side, dict(X=X, y=y), lambda X, y: eng.multinomial_fit_ex(X, y, [0], [n], classes=C, fit_intercept=True))
    assert out["status"] == [0] and out["rc"] == 0              # tests/test_gpu_multinomial.py: test_fit_matches_reference
    assert max(rel(out["coef"][0].cpu().numpy(), b), rel(out["Sig_inv"][0].cpu().numpy(), S), abs(out["loglik"][0] - ll) / abs(ll)) <= 1e-10
    assert same_bits(out, ref)


@pytest.mark.parametrize("p", [257, 1030])
def test_late_inputs_lars_path(eng, orc, side, p):
    S, b, n, icpt, typ, ro = wct._lars_case(p)
    ref, out = _late(side, dict(S=S, b=b), lambda S, b: eng.lars_path(S, b, icpt, float(n), type=typ))
    assert out["beta"].shape == ro["beta"].shape
    errs = {k: rel(out[k].cpu().numpy(), ro[k]) for k in ("beta", "AIC", "BIC") + (("beta0",) if icpt else ())}
    assert all(v < 1e-7 for v in errs.values()), errs           # tests/test_gpu_kernels.py: the correlated wide problems
    if p == 1030:                                               # (the one LARS kernel the workspace table holds to its bits)
        assert same_bits(out, ref)


def test_late_inputs_wls_solve(eng, orc, side):
    """both routes, as tests/test_gpu_pinv_solve.py: test_routes_of_wls_solve"""
    import pinv_reference as pv
    import solve_reference as sr
    p = 260
    S, v = pv.route_case(p, "below")
    _, (theta, rank) = _late(side, dict(S=np.array(S), v=np.array(v)), lambda S, v: eng.wls_solve(S, v))
    assert rank == p and sr.forward_error(theta.cpu().numpy(), sr.solve(S, v)) <= sr.cap(p) * sr.cond2(S)
    cs = pv.case("ones", p)
    _, (theta, rank) = _late(side, dict(S=np.array(cs["S"]), v=np.array(cs["v"])), lambda S, v: eng.wls_solve(S, v))
    fr = wct._pinv_fractions(pv, cs, theta.cpu().numpy())
    assert rank == cs["rank"] == 1 and max(fr.values()) <= 1.0, fr


# ---- the detector tested on itself --------------------------------------------------------------------------------------------------
def test_detector_misses_nothing_and_invents_nothing(side):
    """With the default stream gated, a fill_(1) queued on the default stream is NOT seen by a clone() on the side stream (all
    zeros, the gate still pending), and the same fill queued on the side stream IS seen.  Races on the test's own buffer only."""
    unseen, seen = sg.runs_beside_the_default_stream(side, seconds=0.1)
    assert unseen, "a write queued behind the gate on the default stream was seen from the side stream, or the gate had ended"
    assert seen, "a write queued on the side stream was not seen there while the default stream was gated"


def test_detector_gate_is_a_bounded_sleep(side):
    """the gate returns at once, is pending, and ends by itself after about the time asked for"""
    rate = sg.cycles_per_second()
    assert rate > 1e6
    t0 = time.perf_counter()
    done = sg.gate(torch.cuda.default_stream(), 0.2)
    queued = time.perf_counter() - t0
    pending = not done.query()
    done.synchronize()
    took = time.perf_counter() - t0
    print("gate of 0.2 s: queued in %.4f s, took %.3f s" % (queued, took))
    assert pending and queued < 0.1 and 0.1 <= took <= 1.0, (pending, queued, took)
