"""GPU: the memory contract of the C ABI (include/dlsa_hip.h: the caller brings the scratch, sized by the matching
*_workspace_bytes() query and 256-byte aligned), entry by entry, at exactly the declared size.

Every other GPU test reaches the library through engine._workspace, which hands out at least 1 MiB from a grow-only cache: a
carve that runs past its query lands in slack, a region read before it is written holds what the previous call left, and the
logistic fits pick their driver from the bytes they happen to get.  Here every case of tests/workspace_contract_cases.py makes
its engine calls under tests/guarded_workspace.py -- a body of exactly the query, pre-filled with 0xFF, between two guards --
and must (1) return DLSA_OK, (2) leave the guards intact, (3) meet the bar the entry's existing test applies against its
existing reference (the helpers and bars are imported from those tests, not restated), and, where the existing test asserts
bit-reproducibility, (4) equal a run on a 0x00 body bit for bit.  The refusals: ws_bytes = query - 1 and a body pointer offset
by 8 both return DLSA_ERR_WORKSPACE, leave the outputs the wrapper allocated (pre-filled with a sentinel) and the guards alone.
Two kinds of entry accept less than the query by design and are refused where their own bound lies: the logistic fits (one
chain's slice: the query under chains = 1) and the dlsa_gram_*, dlsa_loglik*_f64 and dlsa_xtv_f32 entries (the need of the
kernel the shape dispatches, read from the error text of a 256-byte call and asserted to be at most the query).

The lock-step logistic driver (dlsa_irls_last_fit_path() == 2) takes its memory from the stream's pool, not from ws: where a
logistic-fit case prints path 2, the guard saw the argument check only.

test_padded_result_pitch: the pass entries that take ldh, called directly with ldh = pe + 3 into a sentinel-filled buffer."""
import contextlib
import ctypes
import functools
import inspect
import math
import re

import numpy as np
import pytest

import guarded_workspace as gw
from workspace_contract_cases import CASES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DLSA_ERR_WORKSPACE = 3
SENTINEL_F, SENTINEL_I = -7.0625, 77
BY_ID = {c.id: c for c in CASES}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available()
    from dlsa_amd import engine
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import dlsa_oracle
    return dlsa_oracle


@pytest.fixture(scope="module")
def api():
    import dlsa_amd
    return dlsa_amd


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- what the library saw -----------------------------------------------------------------------------------------------------
class LibProxy:
    """Stands in front of libdlsa_hip.so for the length of a test: records the queries and the entries that take a workspace and,
    for the refusals, changes the (ws, ws_bytes) pair on its way in -- "short": ws_bytes - 1; "offset": the pointer + 8."""

    def __init__(self, lib, mode=None, only=None, shim=None):
        self._lib, self._mode, self._only, self._shim = lib, mode, only, shim
        self.queries, self.entries, self.changed = [], [], 0

    def __getattr__(self, name):
        from dlsa_amd import _lib
        fn = getattr(self._lib, name)
        sig = _lib.SIGNATURES.get(name)
        if sig is None:
            return fn
        if name.endswith("_workspace_bytes"):
            def query(*args):
                self.queries.append(name)
                return fn(*args)
            return query
        if _lib.c_sz not in sig[1]:
            return fn
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
                elif self._mode == "need":
                    # these entries check the dispatched kernel's own need, which is at most the query: that need, read from the
                    # message of a 256-byte call (itself a refusal), and then one byte less than it
                    query, args[at] = args[at], 256
                    assert fn(*args) == DLSA_ERR_WORKSPACE
                    need = int(re.search(r"workspace (\d+) bytes needed", _lib.last_error()).group(1))
                    assert 256 < need <= query, (need, query)
                    self.need, args[at] = need, need - 1
                else:
                    args[at - 1] = ctypes.c_void_p(args[at - 1].value + 8)
                self.changed += 1
            try:
                return fn(*args)
            finally:
                if self._shim is not None:
                    self._shim.mark = len(self._shim.made)
        return entry


def _entry_wrappers(engine):
    """the engine's functions that bring a workspace"""
    return [n for n, f in vars(engine).items() if inspect.isfunction(f) and n != "_workspace" and "_workspace(" in inspect.getsource(f)]


def record_results(monkeypatch, engine):
    """every result an engine entry returns, in call order"""
    seen = []

    def wrap(name, f):
        @functools.wraps(f)
        def g(*a, **k):
            r = f(*a, **k)
            seen.append((name, r))
            return r
        return g
    for n in _entry_wrappers(engine):
        monkeypatch.setattr(engine, n, wrap(n, getattr(engine, n)))
    return seen


def same_bits(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and bool(torch.equal(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


class SentinelTorch:
    """engine.torch for a refused call: what the wrapper allocates for its outputs comes pre-filled with a sentinel and is kept"""

    def __init__(self):
        self.made, self.mark, self.target = [], 0, None

    def __getattr__(self, name):
        return getattr(torch, name)

    def _filled(self, t):
        if t.numel():
            t.fill_(SENTINEL_F if t.dtype.is_floating_point else SENTINEL_I)
        self.made.append(t)
        return t

    def empty(self, *a, **k):
        return self._filled(torch.empty(*a, **k))

    def zeros(self, *a, **k):
        return self._filled(torch.empty(*a, **k))

    def untouched(self):
        """the refused call's own outputs still hold the sentinel"""
        torch.cuda.synchronize()
        # (the solver probes' tests bring their own pre-filled outputs: nothing of the wrapper's to look at there)
        return all(bool((t == (SENTINEL_F if t.dtype.is_floating_point else SENTINEL_I)).all()) for t in self.target or () if t.numel())


class Ctx:
    def __init__(self, eng, orc, api):
        self.eng, self.orc, self.api = eng, orc, api


# ---- the runners: the engine calls of a family and the bar of its existing test ------------------------------------------------
RUN = {}


def runner(*names):
    def deco(f):
        for n in names:
            RUN[n] = f
        return f
    return deco


@functools.lru_cache(maxsize=4)
def _gram_data(n, p, ld, f32=False):
    rng = np.random.default_rng(n * 1000 + p)
    buf = rng.random((n, ld)) - 0.5            # asymmetric operands, as tests/test_gpu_kernels.py
    w = rng.random(n) * 0.25
    if f32:
        buf, w = buf.astype(np.float32), w.astype(np.float32)
    return buf, w


@runner("gram_f64")
def run_gram_f64(c, n, p, weighted, ld):
    import test_gpu_kernels as tk
    buf, w = _gram_data(n, p, ld)
    Xd = dev(buf)[:, :p]
    H = c.eng.gram(Xd, dev(w) if weighted else None).cpu().numpy()
    print("gram_f64", (n, p, ld), c.eng.gram_last_kernel()[0])
    Ho = c.orc.gram(buf[:, :p], w if weighted else None)
    assert rel(H, Ho) < tk.TOL_KERNEL, rel(H, Ho)
    assert np.array_equal(H, H.T)


@runner("gram_f32")
def run_gram_f32(c, n, p):
    buf, w = _gram_data(n, p, p, True)
    X64, w64 = buf.astype(np.float64), w.astype(np.float64)
    Ho = X64.T @ (w64[:, None] * X64)
    H = c.eng.gram(dev(buf), dev(w)).cpu().numpy()
    assert rel(H, Ho) < 2e-5 and np.array_equal(H, H.T)          # tests/test_gpu_kernels.py: test_gram_f32, test_gram_f32_wide_panels


@runner("gram_f32_acc64")
def run_gram_f32_acc64(c, n, p):
    buf, w = _gram_data(n, p, p, True)
    X = dev(buf)
    ref = X.double().T @ X.double()
    H = c.eng.gram_acc64(X)
    d = ref.diagonal().sqrt()
    assert H.dtype == torch.float64 and torch.equal(H, H.T)     # tests/test_gpu_linear.py: test_gram_f32_acc64_sums_fp32_passes_in_fp64
    assert float(((H - ref).abs() / (d[:, None] * d[None, :])).max()) < 2e-6


@runner("xtv")
def run_xtv(c, n, p, dtype):
    rng = np.random.default_rng(3 + n)
    X, v = rng.random((n, p)) - 0.5, rng.standard_normal(n)
    if dtype == "f32":
        X, v = X.astype(np.float32), v.astype(np.float32)
    g, vv = c.eng.xtv(dev(X), dev(v))
    X64, v64 = X.astype(np.float64), v.astype(np.float64)
    tol = 1e-12 if dtype == "f64" else 1e-6                     # tests/test_gpu_api.py: test_xtv, test_linear_model_fp32_rows
    assert rel(g.cpu().numpy(), X64.T @ v64) < tol
    assert abs(vv.item() - v64 @ v64) <= tol * (v64 @ v64)


@runner("xtv_stats")
def run_xtv_stats(c, n, p, dtype):
    import test_gpu_linear as tl
    tl.test_xtv_stats_matches_numpy_and_accumulates(c.eng, dtype, n, p)


@functools.lru_cache(maxsize=4)
def _logit_data(n, p, icpt):
    rng = np.random.default_rng(n + 7 * p)
    X = rng.random((n, p)) - 0.5
    pe = p + icpt
    beta = rng.standard_normal(pe) * (3.0 / np.sqrt(pe))
    y = (rng.random(n) < 0.5).astype(np.float64)
    X1 = np.column_stack([np.ones(n), X]) if icpt else X
    return X, y, beta, X1


@runner("logit_pass")
def run_logit_pass(c, n, p, icpt):
    X, y, beta, X1 = _logit_data(n, p, icpt)
    w, g, ll = c.eng.logit_pass(dev(X), dev(y), dev(beta), fit_intercept=icpt)
    wo, go, llo = c.orc.logit_pass(X1, y, beta)
    assert rel(w.cpu().numpy(), wo) < 1e-12                     # tests/test_gpu_kernels.py: test_logit_pass_matches_oracle
    assert rel(g.cpu().numpy(), go) < 1e-11
    assert abs(ll.item() - llo) < 1e-12 * abs(llo)


@runner("loglik")
def run_loglik(c, n, p, icpt, cols):
    X, y, _, X1 = _logit_data(n, p, icpt)
    par = np.random.default_rng(12 + p).standard_normal((p + icpt, cols)) * (2.0 / np.sqrt(p + icpt))
    out = c.eng.loglik(dev(X), dev(y), dev(par), fit_intercept=icpt).cpu().numpy()
    assert rel(out, c.orc.logistic_loglik(X1, y, par)) < 1e-12  # tests/test_gpu_api.py: test_loglik_single_pass_many_columns


@runner("irls_pass")
def run_irls_pass(c, n, p, fused):
    X, y = c.orc.synth_logistic(300 + p, 0, n, p, c.orc.SYNTH_GAUSSIAN)
    beta = c.orc.true_beta(p) * 0.8 + 0.05 * np.random.default_rng(p).standard_normal(p)
    wo, go, llo = c.orc.logit_pass(X, y, beta)
    Ho = c.orc.gram(X, wo)
    H, g, ll, w = c.eng.irls_pass(dev(X), dev(y), dev(beta), want_w=True)
    kernel = c.eng.gram_last_kernel()[0]
    print("irls_pass", (n, p), kernel)
    assert kernel.startswith("irls_pass_narrow_kernel") == fused, kernel
    assert torch.equal(H, H.T)                                  # tests/test_gpu_irls_pass.py: test_fused_pass_matches_oracle
    assert rel(w.cpu().numpy(), wo) < 1e-12
    assert rel(H.cpu().numpy(), Ho) < 1e-12
    assert np.max(np.abs(g.cpu().numpy() - go)) < 1e-12 * np.max(np.abs(X).sum(0))
    assert abs(float(ll) - llo) < 1e-12 * abs(llo)


@runner("newton_wide_pass")
def run_newton_wide_pass(c, n, p, icpt):
    import test_gpu_wide as tw
    tw.test_wide_pass_matches_oracle(c.eng, c.orc, p, n, icpt)


@runner("gram_icpt")
def run_gram_icpt(c, n, p):
    import test_gpu_nocopy as tn
    tn.test_implicit_intercept_passes_match_oracle_on_the_materialised_column(c.eng, c.orc, n, p)


# ---- the logistic fits ------------------------------------------------------------------------------------------------------
PATHS = {0: "chains", 1: "one-launch", 2: "lock step (pool memory: outside the guard)"}


@functools.lru_cache(maxsize=2)
def _irls_rows(K, rows, p):
    from oracle import dlsa_oracle as orc
    X, y = orc.synth_logistic(31 + p, 0, K * rows, p, orc.SYNTH_UNIFORM)
    return X, y, dev(X), dev(y)


@functools.lru_cache(maxsize=None)
def _irls_blocks(K, rows, p, icpt, strided):
    from oracle import dlsa_oracle as orc
    X, y = _irls_rows(K, rows, p)[:2]
    parts = [slice(k, K * rows, K) for k in range(K)] if strided else [slice(k * rows, (k + 1) * rows) for k in range(K)]
    return [orc.logistic_model_block(X[s], y[s], fit_intercept=icpt) for s in parts]


LAST = {}


def _check_logistic(tag, r, blocks, eng, dense=True):
    # (dlsa_irls_last_fit_path speaks of the dense fits; the structured ones always run the host-driven chains)
    path = LAST["path"] = eng.irls_last_fit_path() if dense else 0
    worst = {}
    assert r["status"] == [0] * len(blocks), r["status"]
    for k, (co, smo, so) in enumerate(blocks):                  # the parity bar of tests/test_gpu_chains.py and tests/test_gpu_wide.py
        for key, ref in (("coef", co), ("Sig_inv", so), ("Sig_invMcoef", smo)):
            worst[key] = max(worst.get(key, 0.0), rel(r[key][k].cpu().numpy(), ref))
    print("logistic fit %s: driver %d (%s) %s" % (tag, path, PATHS[path], " ".join("%s %.1e" % kv for kv in worst.items())))
    assert all(v < 1e-10 for v in worst.values()), worst


@runner("irls_fit")
def run_irls_fit(c, K, rows, p, options, tag=""):
    X, y, Xd, yd = _irls_rows(K, rows, p)
    offs = [k * rows for k in range(K + 1)]
    with c.eng.irls_options(**options) if options else contextlib.nullcontext():
        r = c.eng.irls_fit(Xd, yd, offs)
    _check_logistic("irls_fit K=%d x %d p=%d %s" % (K, rows, p, options), r, _irls_blocks(K, rows, p, False, False), c.eng)


@runner("irls_fit_ex")
def run_irls_fit_ex(c, K, rows, p, options, icpt, strided):
    X, y, Xd, yd = _irls_rows(K, rows, p)
    first = list(range(K)) if strided else [k * rows for k in range(K)]
    with c.eng.irls_options(**options) if options else contextlib.nullcontext():
        r = c.eng.irls_fit_ex(Xd, yd, first, [rows] * K, K if strided else 1, fit_intercept=icpt)
    _check_logistic("irls_fit_ex K=%d x %d p=%d icpt=%d step=%d %s" % (K, rows, p, icpt, K if strided else 1, options), r,
                    _irls_blocks(K, rows, p, icpt, strided), c.eng)


@functools.lru_cache(maxsize=2)
def _onehot_logistic(n, q, nlevels):
    import dlsa_amd
    from oracle import dlsa_oracle as orc
    import test_gpu_onehot as to
    rng = np.random.default_rng(11 + n)
    p, num, codes, desc, nl, level_col = to._random_design(rng, n, q, nlevels)
    plan = to._plan(dlsa_amd, p, desc, nl, level_col)
    X, _ = orc.design_matrix(num, codes, *desc)
    beta = rng.normal(size=p) * 0.3
    y = (rng.random(n) < 1 / (1 + np.exp(-X @ beta))).astype(np.float64)
    return plan, X, y, dev(num), dev(codes), dev(y)


@functools.lru_cache(maxsize=None)
def _onehot_blocks(n, q, nlevels, parts):
    from oracle import dlsa_oracle as orc
    _, X, y = _onehot_logistic(n, q, nlevels)[:3]
    return [orc.logistic_model_block(X[slice(*s)], y[slice(*s)]) for s in parts]


@runner("onehot_irls_fit")
def run_onehot_irls_fit(c, n, q, nlevels, options):
    plan, X, y, dn, dc, dy = _onehot_logistic(n, q, nlevels)
    offs = [0, n // 4, n // 4, 5 * n // 8, n]                   # one empty partition, as test_structured_fit_many_partitions_matches_dense
    with c.eng.irls_options(**options) if options else contextlib.nullcontext():
        r = c.eng.onehot_irls_fit(plan, dn, dc, dy, offs)
    assert r["status"] == [0, 4, 0, 0], r["status"]
    assert float(r["Sig_inv"][1].abs().max()) == 0.0 and float(r["coef"][1].abs().max()) == 0.0
    blocks = _onehot_blocks(n, q, nlevels, tuple((offs[k], offs[k + 1], 1) for k in (0, 2, 3)))
    keep = {k: r[k][[0, 2, 3]] for k in ("coef", "Sig_inv", "Sig_invMcoef")}
    keep["status"] = [0, 0, 0]
    _check_logistic("onehot_irls_fit n=%d %s" % (n, options), keep, blocks, c.eng, dense=False)


@runner("onehot_irls_fit_ex")
def run_onehot_irls_fit_ex(c, n, q, nlevels, K, options):
    plan, X, y, dn, dc, dy = _onehot_logistic(n, q, nlevels)
    with c.eng.irls_options(**options) if options else contextlib.nullcontext():
        r = c.eng.onehot_irls_fit_ex(plan, dn, dc, dy, list(range(K)), [len(range(k, n, K)) for k in range(K)], row_step=K)
    _check_logistic("onehot_irls_fit_ex n=%d K=%d %s" % (n, K, options), r,
                    _onehot_blocks(n, q, nlevels, tuple((k, n, K) for k in range(K))), c.eng, dense=False)


# ---- Cox ---------------------------------------------------------------------------------------------------------------------
def _cox_also(c, n, p, ties, strata):
    """include/dlsa_hip.h: the strata query of the unstratified model is the ties query, and for Breslow the oldest query"""
    from dlsa_amd import _lib
    lib, code = _lib.load(), c.eng.cox_ties(ties)
    if not strata:
        assert lib.dlsa_cox_strata_workspace_bytes(n, p, code, 0) == lib.dlsa_cox_ties_workspace_bytes(n, p, code) > 0
        if ties == "breslow":
            assert lib.dlsa_cox_ties_workspace_bytes(n, p, 0) == lib.dlsa_cox_workspace_bytes(n, p)


@runner("cox_pass")
def run_cox_pass(c, n, p, ties, strata):
    import cox_strata_cases as cases
    import test_gpu_cox_strata as ts
    _cox_also(c, n, p, ties, strata)
    X, t, ev, beta, codes = cases.pass_case(p, n, "random7")
    if strata:
        ts._check_pass(c.eng, X, t, ev, beta, codes, ties, form=ts.CUMSUM[ties])
    else:
        ts._check("%s pass" % ties, X, ts._pass(c.eng, X, t, ev, beta, None, ties), ts.CUMSUM[ties](X, t, ev, beta))


@functools.lru_cache(maxsize=None)
def _cox_fit_case(n, p, ties, strata):
    import cox_strata_cases as cases
    import cox_strata_reference as sr
    import test_gpu_cox_strata as ts
    X, t, ev, codes = cases.fit_case(p, n)
    offs = [0, n // 3, 2 * n // 3, n]
    ev = ev.copy()
    ev[offs[1]:offs[2]] = 0.0                                   # a partition without events: the zero block
    refs = {}
    for k in (0, 2):
        sl = slice(offs[k], offs[k + 1])
        if strata:
            refs[k] = sr.fit(X[sl], t[sl], ev[sl], codes[sl], form=ts.CUMSUM[ties])
        else:
            refs[k] = (ts.cr.fit if ties == "breslow" else ts.er.fit)(X[sl], t[sl], ev[sl], form=ts.CUMSUM[ties])
    return X, t, ev, codes if strata else None, offs, refs


@runner("cox_fit")
def run_cox_fit(c, n, p, ties, strata, K):
    import test_gpu_cox_strata as ts
    _cox_also(c, n // 3 + 1, p, ties, strata)
    X, t, ev, codes, offs, refs = _cox_fit_case(n, p, ties, strata)
    r = ts._fit(c.eng, X, t, ev, offs, codes, ties)
    assert r["status"] == [0, 4, 0], r["status"]
    assert not r["Sig_inv"][1].any() and not r["coef"][1].any() and not r["Sig_invMcoef"][1].any()
    for k, (b, H, ll) in refs.items():                          # the 1e-10 of tests/test_gpu_cox_strata.py: test_fit_matches_reference
        errs = (rel(r["coef"][k].cpu().numpy(), b), rel(r["Sig_inv"][k].cpu().numpy(), H), rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b),
                abs(r["loglik"][k] - ll) / abs(ll))
        print("cox fit %s strata=%s p=%d k=%d: coef %.1e Sig_inv %.1e Sig_invMcoef %.1e loglik %.1e" % ((ties, strata, p, k) + errs))
        assert max(errs) <= 1e-10, errs


# ---- the count families --------------------------------------------------------------------------------------------------------
NB_ALPHA, TW_POWER = 0.5, 1.5


def _count_data(fam, seed, n, p, icpt):
    if fam == "poisson":
        import test_gpu_poisson as tp
        return tp._data(seed, n, p, icpt, True)
    if fam == "negbin":
        import negbin_reference as nr
        return nr.data(seed, n, p, icpt, True, NB_ALPHA)
    if fam == "gamma":
        import test_gpu_gamma as tg
        return tg._data(seed, n, p, icpt, True)
    import tweedie_reference as tr
    return tr.data(seed, n, p, icpt, True, TW_POWER)


def _count_pass(fam):
    def run(c, n, p, icpt):
        X, y, o = _count_data(fam, 10 + p, n, p, icpt)
        if fam == "poisson":
            import test_gpu_poisson as tp
            tp._check_pass(c.eng, X, y, o, tp._away_from_optimum(p + icpt), icpt)
        elif fam == "negbin":
            import test_gpu_negbin as tn
            tn._check_pass(c.eng, X, y, o, tn._away_from_optimum(p + icpt), NB_ALPHA, icpt)
        elif fam == "gamma":
            import test_gpu_gamma as tg
            tg._check_pass(c.eng, X, y, o, tg._away_from_optimum(p + icpt), icpt, 0.37)
        else:
            import test_gpu_tweedie as tt
            import tweedie_reference as tr
            tt._check_pass(c.eng, X, y, o, tr.away_from_optimum(p + icpt), icpt, TW_POWER, 0.37)
    return run


@functools.lru_cache(maxsize=None)
def _count_fit_case(fam, rows, K, p, icpt, strided):
    n = rows * K
    X, y, o = _count_data(fam, 40 + p, n, p, icpt)
    parts = [slice(k, n, K) for k in range(K)] if strided else [slice(k * rows, (k + 1) * rows) for k in range(K)]
    refs = []
    for s in parts:
        if fam == "poisson":
            import poisson_reference as pr
            refs.append(pr.fit(X[s], y[s], o[s], icpt))
        elif fam == "negbin":
            import negbin_reference as nr
            refs.append(nr.fit(X[s], y[s], o[s], icpt))
        elif fam == "gamma":
            import gamma_reference as gr
            refs.append(gr.fit(X[s], y[s], o[s], icpt))
        else:
            import tweedie_reference as tr
            refs.append(tr.fit(X[s], y[s], TW_POWER, o[s], icpt))
    return X, y, o, refs


def _count_fit(fam):
    def run(c, rows, K, p, icpt, strided):
        X, y, o, refs = _count_fit_case(fam, rows, K, p, icpt, strided)
        first = list(range(K)) if strided else [k * rows for k in range(K)]
        kw = dict(power=TW_POWER) if fam == "tweedie" else {}
        r = getattr(c.eng, fam + "_fit_ex")(dev(X), dev(y), first, [rows] * K, row_step=K if strided else 1, offset=dev(o), fit_intercept=icpt, **kw)
        assert r["status"] == [0] * K, r["status"]
        worst = {}
        for k, ref in enumerate(refs):
            b, H, ll = ref[:3]
            errs = {"coef": rel(r["coef"][k].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][k].cpu().numpy(), H),
                    "Sig_invMcoef": rel(r["Sig_invMcoef"][k].cpu().numpy(), H @ b), "ll": abs(r["loglik"][k] - ll) / abs(ll)}
            if fam == "negbin":                                 # tests/test_gpu_negbin.py: test_fit_matches_reference
                a, info, pearson = ref[3:]
                assert a > 0 and r["alpha"][k] > 0
                assert abs(r["alpha"][k] - a) <= 1e-9 * a and abs(r["alpha_info"][k] - info) <= 1e-6 * info
                assert abs(r["pearson"][k] - pearson) <= 1e-9 * pearson
            elif fam in ("gamma", "tweedie"):                   # tests/test_gpu_gamma.py, tests/test_gpu_tweedie.py: test_fit_matches_reference
                phi, P, dv = ref[3:]
                errs.update({"phi": abs(r["dispersion"][k] - phi) / phi, "P": abs(r["pearson"][k] - P) / P, "Dev": abs(r["deviance"][k] - dv) / dv})
            worst = {key: max(v, worst.get(key, 0.0)) for key, v in errs.items()}
        print("%s fit %dx%d p=%d icpt=%d step=%d (%s evaluations): %s" % (fam, K, rows, p, icpt, K if strided else 1, r["n_iter"],
                                                                          " ".join("%s %.1e" % kv for kv in worst.items())))
        assert all(v <= 1e-10 for v in worst.values()), worst
    return run


for _fam in ("poisson", "negbin", "gamma", "tweedie"):
    RUN[_fam + "_pass"] = _count_pass(_fam)
    RUN[_fam + "_fit"] = _count_fit(_fam)


@runner("multinomial_pass")
def run_multinomial_pass(c, n, p, C, icpt):
    import multinomial_reference as mr
    import test_gpu_multinomial as tm
    X, y = mr.data(10 + p, n, p, C, icpt)
    tm._check_pass(c.eng, X, y, mr.away_from_optimum((C - 1) * (p + icpt)), C, icpt)


@functools.lru_cache(maxsize=None)
def _multinomial_fit_case(n, p, C, icpt):
    import multinomial_reference as mr
    X, y = mr.data(40 + p, n, p, C, icpt)
    return X, y, mr.fit(X, y, C, bool(icpt))


@runner("multinomial_fit")
def run_multinomial_fit(c, n, p, C, icpt):
    import test_gpu_multinomial as tm
    X, y, (b, S, ll, n_iter) = _multinomial_fit_case(n, p, C, icpt)
    r = tm._fit(c.eng, X, y, [0, n], C, icpt)
    assert r["status"] == [0] and r["rc"] == 0                  # tests/test_gpu_multinomial.py: test_fit_matches_reference
    errs = {"coef": rel(r["coef"][0].cpu().numpy(), b), "Sig_inv": rel(r["Sig_inv"][0].cpu().numpy(), S),
            "Sig_invMcoef": rel(r["Sig_invMcoef"][0].cpu().numpy(), S @ b), "ll": abs(r["loglik"][0] - ll) / abs(ll)}
    print("multinomial fit n=%d p=%d C=%d: %d evaluations (reference %d) %s" % (n, p, C, r["n_iter"][0], n_iter, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-10 for v in errs.values()), errs
    Sn = r["Sig_inv"][0].cpu().numpy()
    assert np.array_equal(Sn, Sn.T)


# ---- the structured one-hot families: the existing tests' own bodies, at their smallest shapes -----------------------------------
def _ordered(c, ordered):
    return c.eng.kernel_options(onehot_ordered=ordered)


@runner("onehot_logit_gram")
def run_onehot_logit_gram(c, n, q, nlevels, intercept, baseline, ordered):
    import test_gpu_onehot as to
    to._check_passes(c.api, c.orc, n, q, nlevels, intercept=intercept, baseline=baseline, ordered=ordered)


@runner("onehot_poisson_pass")
def run_onehot_poisson_pass(c, n, q, nlevels, intercept, baseline, ordered):
    import test_gpu_onehot_poisson as t
    with _ordered(c, ordered):
        t.test_pass_matches_reference(c.api, c.orc, n, q, nlevels, intercept, baseline, True)


@runner("onehot_negbin_pass")
def run_onehot_negbin_pass(c, n, q, nlevels, intercept, baseline, ordered):
    import test_gpu_onehot_negbin as t
    with _ordered(c, ordered):
        t.test_pass_matches_reference(c.api, c.orc, n, q, nlevels, intercept, baseline, True, 0.5)


@runner("onehot_gamma_pass")
def run_onehot_gamma_pass(c, n, q, nlevels, intercept, baseline, ordered):
    import test_gpu_onehot_gamma as t
    with _ordered(c, ordered):
        t.test_pass_matches_dense_and_reference(c.api, c.orc, n, q, nlevels, intercept, baseline, True, 0.37)


@runner("onehot_tweedie_pass")
def run_onehot_tweedie_pass(c, n, q, nlevels, intercept, baseline, ordered):
    import test_gpu_onehot_tweedie as t
    with _ordered(c, ordered):
        t.test_pass_matches_dense_and_reference(c.api, c.orc, n, q, nlevels, intercept, baseline, True, 1.2, 0.37)


@runner("onehot_multinomial_pass")
def run_onehot_multinomial_pass(c, n, q, nlevels, intercept, baseline, ordered):
    import test_gpu_onehot_multinomial as t
    with _ordered(c, ordered):
        t.test_pass_matches_reference(c.api, c.orc, n, q, nlevels, 3, (intercept, baseline))


@runner("onehot_poisson_fit")
def run_onehot_poisson_fit(c, ordered):
    import test_gpu_onehot_poisson as t
    with _ordered(c, ordered):
        t.test_fit_matches_reference(c.api, c.orc, 24_000, 2, (40, 5), 6, True, 24_002)


@runner("onehot_negbin_fit")
def run_onehot_negbin_fit(c, ordered):
    import test_gpu_onehot_negbin as t
    with _ordered(c, ordered):
        t.test_fit_matches_reference(c.api, c.orc, 0.2, True)


@runner("onehot_gamma_fit")
def run_onehot_gamma_fit(c, ordered):
    import test_gpu_onehot_gamma as t
    with _ordered(c, ordered):
        t.test_fit_matches_dense_and_reference(c.api, c.orc, 24_000, 2, (40, 5), 6, False, 24_002)


@runner("onehot_tweedie_fit")
def run_onehot_tweedie_fit(c, ordered):
    import test_gpu_onehot_tweedie as t
    with _ordered(c, ordered):
        t.test_fit_matches_dense_and_reference(c.api, c.orc, 24_000, 2, (40, 5), 6, False, 24_002, 1.3)


@runner("onehot_multinomial_fit")
def run_onehot_multinomial_fit(c, ordered):
    import test_gpu_onehot_multinomial as t
    with _ordered(c, ordered):
        t.test_fit_matches_reference(c.api, c.orc, 20_000, 1, (4, 3), 4, True, 7, 8)


# ---- the solvers ---------------------------------------------------------------------------------------------------------------
@runner("spd_solve")
def run_spd_solve(c, p):
    rng = np.random.default_rng(1 + p)                          # the systems and the bar of tests/test_gpu_kernels.py: test_spd_solve
    A = rng.standard_normal((p + 5, p))
    S = A.T @ A + 0.1 * np.eye(p)
    v = rng.standard_normal(p)
    th = c.eng.spd_solve(dev(S), dev(v)).cpu().numpy()
    assert rel(th, np.linalg.solve(S, v)) < 1e-9


def _pinv_fractions(pv, cs, theta, eig=None):
    """the measures and caps of tests/test_gpu_pinv_solve.py that need no eigenvectors, on a closed-form case"""
    p = cs["p"]
    fr = {"theta": pv.theta_error(theta, cs["theta"]) / (pv.C(p) * float(cs["lmax"] / cs["min_kept"]))}
    if eig is not None:
        fr["eig"] = pv.eigenvalue_error(eig, cs["lam"], cs["lmax"]) / pv.C(p)
    if cs["singular"]:
        fr["null"] = pv.null_component(cs["N"], theta) / pv.C(p)
    return fr


@runner("sym_pinv_solve")
def run_sym_pinv_solve(c, p):
    import pinv_reference as pv
    for kind in ("toeplitz", "ones"):                           # full rank, and rank 1
        cs = pv.case(kind, p)
        theta, rank, eig = c.eng.sym_pinv_solve(dev(np.array(cs["S"])), dev(np.array(cs["v"])))
        fr = _pinv_fractions(pv, cs, theta.cpu().numpy(), np.array(eig))
        print("sym_pinv_solve %s p=%d rank %d: %s" % (kind, p, rank, " ".join("%s=%.4f" % kv for kv in fr.items())))
        assert rank == cs["rank"] and max(fr.values()) <= 1.0, fr


@runner("wls_solve")
def run_wls_solve(c, p):
    """both routes, as tests/test_gpu_pinv_solve.py: test_routes_of_wls_solve -- the Cholesky route on a system 100 times inside
    lstsq's cut, the spectral route on the rank-1 matrix of ones"""
    import pinv_reference as pv
    import solve_reference as sr
    S, v = pv.route_case(p, "below")
    theta, rank = c.eng.wls_solve(dev(np.array(S)), dev(np.array(v)))
    assert rank == p and sr.forward_error(theta.cpu().numpy(), sr.solve(S, v)) <= sr.cap(p) * sr.cond2(S)
    cs = pv.case("ones", p)
    theta, rank = c.eng.wls_solve(dev(np.array(cs["S"])), dev(np.array(cs["v"])))
    fr = _pinv_fractions(pv, cs, theta.cpu().numpy())
    assert rank == cs["rank"] == 1 and max(fr.values()) <= 1.0, fr


@runner("newton_probe")
def run_newton_probe(c, route, p):
    import test_gpu_newton_solvers as ns
    ns_test = {"factor": ns.test_factor_route, "reuse": ns.test_factor_route, "inverse": ns.test_inverse_route, "sweep": ns.test_sweep_route}[route]
    ns_test(c.eng, p, 1e6)


@runner("newton_probe_batched")
def run_newton_probe_batched(c, p):
    import test_gpu_newton_solvers as ns
    ns.test_batched_sweep(c.eng, p)


@runner("newton_probe_batched1")
def run_newton_probe_batched1(c, p):
    """count = 1 on the batched route: the single-system sweep's bits"""
    import solve_reference as sr
    import test_gpu_newton_solvers as ns
    case = sr.case(p, 1e6)
    S, v = np.array(case["S"]), np.array(case["v"])
    lds = p + ns.PAD
    x = torch.full((p,), ns.SENTINEL, dtype=torch.float64, device="cuda")
    M = torch.full((p * p,), ns.SENTINEL, dtype=torch.float64, device="cuda")
    st = torch.full((3,), ns.SENTINEL, dtype=torch.float64, device="cuda")
    c.eng.newton_solve_probe("sweep_batched", dev(ns.pitched(S, lds)), dev(v), p, lds, count=1, x=x, M=M, stats=st,
                             active=torch.ones(1, dtype=torch.int32, device="cuda"))
    xs, Hs, sts = ns.run(c.eng, "sweep", S, v, lds=lds)
    assert np.array_equal(ns.bits(x.cpu().numpy()), ns.bits(xs)) and np.array_equal(ns.bits(M.cpu().numpy()), ns.bits(Hs.reshape(-1)))
    assert np.array_equal(ns.bits(st.cpu().numpy()), ns.bits(sts))
    assert sr.backward_error(S, xs, v) <= sr.cap(p)


# ---- LARS ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lars_case(p):
    from oracle import dlsa_oracle as orc
    import test_gpu_kernels as tk
    if p == 3:
        rng = np.random.default_rng(5)
        n = 2000
        X = np.column_stack([np.ones(n), rng.random((n, p - 1)) - 0.5])
        S, b, icpt, typ = X.T @ (rng.random(n)[:, None] * 0.25 * X), orc.true_beta(p) + 0.05 * rng.standard_normal(p), True, "lar"
    else:
        (S, b, n), icpt, typ = tk._correlated_lsa_problem(p, {120: 0.98, 257: 0.97, 1030: 0.9}[p], {120: 5, 257: 11, 1030: 3}[p]), p == 1030, "lasso"
    return S, b, n, icpt, typ, orc.lars_lsa(S, b, icpt, n, type=typ)


@runner("lars")
def run_lars(c, p, kopt):
    S, b, n, icpt, typ, ro = _lars_case(p)
    with c.eng.kernel_options(**kopt) if kopt else contextlib.nullcontext():
        r = c.eng.lars_path(dev(S), dev(b), icpt, float(n), type=typ)
    assert r["beta"].shape == ro["beta"].shape, (r["beta"].shape, ro["beta"].shape)
    errs = {k: rel(r[k].cpu().numpy(), ro[k]) for k in ("beta", "AIC", "BIC") + (("beta0",) if icpt else ())}
    print("lars p=%d %s: %s" % (p, kopt, " ".join("%s %.1e" % kv for kv in errs.items())))
    # tests/test_gpu_kernels.py: 1e-8 on the narrow problem (test_lars_intercept_matches_oracle), 1e-7 on the correlated wide ones
    assert all(v < (1e-8 if p == 3 else 1e-7) for v in errs.values()), errs


for _c in CASES:
    assert _c.family in RUN, _c.family


# ---- the tests -----------------------------------------------------------------------------------------------------------------
def _guarded_run(case, ctx, fill):
    from dlsa_amd import _lib, engine
    with pytest.MonkeyPatch.context() as mp:
        g = gw.guarded(mp, fill=fill)
        proxy = LibProxy(_lib.load())
        mp.setattr(_lib, "load", lambda: proxy)
        seen = record_results(mp, engine)
        RUN[case.family](ctx, **case.params)
        g.check()
    assert g.allocations, "the case made no call that brings a workspace"
    assert set(case.entries) <= set(proxy.entries), (case.entries, sorted(set(proxy.entries)))
    assert set(case.queries) <= set(proxy.queries), (case.queries, sorted(set(proxy.queries)))
    return seen, g


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_contract_at_the_declared_size(eng, orc, api, cid):
    """DLSA_OK, intact guards and the existing bar on a body of exactly the query filled with 0xFF; where the entry is
    bit-reproducible, the same bits on a body filled with 0x00"""
    case, ctx = BY_ID[cid], Ctx(eng, orc, api)
    seen, g = _guarded_run(case, ctx, gw.POISON)
    print("contract %s: %d workspaces, %s" % (cid, len(g.allocations), sorted(set(g.queries))[:4]))
    if case.refuse == "chains1":
        # the logistic fits pick their driver and their chain count from the shapes and the options, not from spare bytes: the same
        # driver, and the same bits, with sixteen times the query and 256 MiB on top (what the engine's grow-only cache may hold)
        from dlsa_amd import engine
        at_query = LAST.pop("path")
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(engine, "_workspace", lambda nbytes, device: torch.full((16 * int(nbytes) + (256 << 20),), 0xFF, dtype=torch.uint8, device=device))
            roomy = record_results(mp, engine)
            RUN[case.family](ctx, **case.params)
        print("contract %s: driver %d at the query, %d with room to spare" % (cid, at_query, LAST["path"]))
        assert LAST.pop("path") == at_query
        assert [n for n, _ in seen] == [n for n, _ in roomy] and all(same_bits(a, b) for (_, a), (_, b) in zip(seen, roomy))
    if case.bits:
        seen0, _ = _guarded_run(case, ctx, 0x00)
        assert [n for n, _ in seen] == [n for n, _ in seen0]
        for (name, a), (_, b) in zip(seen, seen0):
            assert same_bits(a, b), "%s: the result depends on what the workspace held before the call" % name


def _one_case_per_entry():
    """a refusal is decided before any work: one case (the table's first) for every entry the table names"""
    first = {}
    for c in CASES:
        for e in c.entries:
            first.setdefault(e, c.id)
    return [(cid, e) for e, cid in first.items()]


@pytest.mark.parametrize("mode", ["short", "offset"])
@pytest.mark.parametrize("cid,entry", _one_case_per_entry())
def test_refusals(eng, orc, api, cid, entry, mode):
    """ws_bytes = query - 1, and the body pointer offset by 8, at `entry` (the case's calls before it run as they are):
    DLSA_ERR_WORKSPACE, the outputs of that call and every guard untouched"""
    from dlsa_amd import _lib, engine
    case, ctx = BY_ID[cid], Ctx(eng, orc, api)
    with pytest.MonkeyPatch.context() as mp:
        g = gw.guarded(mp)
        shim = SentinelTorch()
        proxy = LibProxy(_lib.load(), "need" if (mode == "short" and case.refuse == "need") else mode, only=entry, shim=shim)
        mp.setattr(_lib, "load", lambda: proxy)
        mp.setattr(engine, "torch", shim)
        with engine.irls_options(chains=1) if case.refuse == "chains1" else contextlib.nullcontext():
            with pytest.raises(_lib.DlsaError) as e:
                RUN[case.family](ctx, **case.params)
        assert e.value.code == DLSA_ERR_WORKSPACE, str(e.value)
        assert proxy.changed == 1 and proxy.entries[-1] == entry
        assert shim.untouched(), "a refused call wrote into its outputs"
        g.check()


def test_the_guard_sees_a_device_write(eng):
    """the checker on device memory, as tests/test_guarded_workspace_cpu.py on the host: a kernel's store of one double just past
    the body (and one just before it) is reported with its side and offsets"""
    with pytest.MonkeyPatch.context() as mp:
        g = gw.guarded(mp)
        body = eng._workspace(4096, torch.device("cuda"))
        assert body.is_cuda and body.data_ptr() % 256 == 0 and bool((body == 0xFF).all())
        g.check()
        buf = g.allocations[0].buf
        buf[gw.GUARD_BYTES + 4096: gw.GUARD_BYTES + 4104].view(torch.float64).fill_(1.0)
        with pytest.raises(gw.GuardDamaged, match="back guard damaged, 8 bytes, first offset 0, last offset 7"):
            g.check()
        buf[gw.GUARD_BYTES + 4096: gw.GUARD_BYTES + 4104] = gw.GUARD_BYTE
        buf[gw.GUARD_BYTES - 8: gw.GUARD_BYTES].view(torch.float64).fill_(0.0)
        with pytest.raises(gw.GuardDamaged, match="front guard damaged, 8 bytes, first offset %d, last offset %d" % (gw.GUARD_BYTES - 8, gw.GUARD_BYTES - 1)):
            g.check()


# ---- ldh = pe + 3 ----------------------------------------------------------------------------------------------------------------
def _ws(lib_query, *a):
    n = lib_query(*a)
    assert n > 0
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")


def _pitched_pair(call, d):
    """call(H, ldh) fills a d x d result at pitch ldh: the packed run and the run at ldh = d + 3 into a sentinel-filled buffer"""
    from dlsa_amd import _lib
    tight = torch.full((d, d), SENTINEL_F, dtype=torch.float64, device="cuda")
    wide = torch.full((d, d + 3), SENTINEL_F, dtype=torch.float64, device="cuda")
    _lib.check(call(tight, d))
    _lib.check(call(wide, d + 3))
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :d], tight), "the block at ldh = pe + 3 differs from the packed one"
    assert bool((wide[:, d:] == SENTINEL_F).all()), "the pad columns were written"
    assert not bool((tight == SENTINEL_F).any())


PITCH = ["irls_pass-fused", "irls_pass-two-launch", "gram_icpt", "newton_wide_pass", "newton_wide_pass-icpt", "cox_pass-breslow", "cox_pass-efron-strata",
         "poisson", "negbin", "gamma", "tweedie", "multinomial-C3", "multinomial-C8-p40"]


@pytest.mark.parametrize("what", PITCH)
def test_padded_result_pitch(eng, orc, what):
    """The engine always passes ldh = pe.  One direct call per pass entry that takes ldh, with ldh = pe + 3: the pe x pe block
    equals the ldh = pe result bit for bit and the pad columns keep the sentinel (the multinomial sub-block writer and the
    mirror kernels are the ones that could get this wrong)."""
    from dlsa_amd import _lib
    from dlsa_amd.engine import _ptr, _stream
    lib = _lib.load()
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    if what.startswith("irls_pass"):
        n, p = (8192, 50) if what.endswith("fused") else (8191, 51)
        X, y = orc.synth_logistic(300 + p, 0, n, p, orc.SYNTH_GAUSSIAN)
        Xd, yd, bd = dev(X), dev(y), dev(orc.true_beta(p) * 0.8)
        ws, g, ll = _ws(lib.dlsa_irls_pass_workspace_bytes, n, p), f64(p), f64(1)
        _pitched_pair(lambda H, ldh: lib.dlsa_irls_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(bd), n, p, _ptr(H), ldh, _ptr(g), _ptr(ll), None,
                                                             _ptr(ws), ws.numel(), _stream()), p)
    elif what == "gram_icpt":
        n, p = 5001, 120
        X, _ = orc.synth_logistic(41 + p, 0, n, p, orc.SYNTH_GAUSSIAN)
        Xd, wd = dev(X), dev(np.random.default_rng(p).random(n) * 0.25)
        ws = _ws(lib.dlsa_gram_icpt_workspace_bytes, n, p)
        _pitched_pair(lambda H, ldh: lib.dlsa_gram_icpt_f64(_ptr(Xd), p, _ptr(wd), n, p, _ptr(H), ldh, _ptr(ws), ws.numel(), _stream()), p + 1)
    elif what.startswith("newton_wide_pass"):
        n, p, icpt = 32785, 121, int(what.endswith("icpt"))
        X, y = orc.synth_logistic(700 + p, 0, n, p, orc.SYNTH_GAUSSIAN)
        Xd, yd, bd = dev(X), dev(y), dev(np.concatenate([[0.25] * icpt, orc.true_beta(p) * 0.7]))
        ws, g, ll = _ws(lib.dlsa_newton_wide_workspace_bytes, n, p, icpt), f64(p + icpt), f64(1)
        _pitched_pair(lambda H, ldh: lib.dlsa_newton_wide_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(bd), n, p, icpt, None, _ptr(g), _ptr(ll),
                                                                    _ptr(H), ldh, _ptr(ws), ws.numel(), _stream()), p + icpt)
    elif what.startswith("cox_pass"):
        import cox_strata_cases as cases
        n, p = 5003, 7
        strata = what.endswith("strata")
        code = 1 if "efron" in what else 0
        X, t, ev, beta, codes = cases.pass_case(p, n, "random7")
        Xd, td, ed, bd = dev(X), dev(t), dev(ev), dev(beta)
        od = dev(cases.sort_order(t, codes if strata else None))
        sd = dev(codes.astype(np.int32)) if strata else None
        ws, g, ll = _ws(lib.dlsa_cox_strata_workspace_bytes, n, p, code, int(strata)), f64(p), f64(1)
        _pitched_pair(lambda H, ldh: lib.dlsa_cox_pass_strata_f64(_ptr(Xd), p, _ptr(td), _ptr(ed), _ptr(sd), _ptr(od), n, p, code, _ptr(bd),
                                                                   _ptr(H), ldh, _ptr(g), _ptr(ll), None, _ptr(ws), ws.numel(), _stream()), p)
    elif what.startswith("multinomial"):
        import multinomial_reference as mr
        n, p, C = (6001, 5, 3) if what.endswith("C3") else (6001, 40, 8)
        X, y = mr.data(10 + p, n, p, C, True)
        d = (C - 1) * (p + 1)
        Xd, yd, td = dev(X), dev(y), dev(mr.away_from_optimum(d))
        ws, g, ll = _ws(lib.dlsa_multinomial_workspace_bytes, n, p, 1, C, 1), f64(d), f64(1)
        _pitched_pair(lambda H, ldh: lib.dlsa_multinomial_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(td), C, n, p, 1, _ptr(H), ldh, _ptr(g), _ptr(ll),
                                                                    None, 0, _ptr(ws), ws.numel(), _stream()), d)
    else:
        n, p, icpt = 4001, 130, 1
        X, y, o = _count_data(what, 10 + p, n, p, True)
        Xd, yd, od = dev(X), dev(y), dev(o)
        bd = dev(np.linspace(-0.8, 0.6, p + 1) / math.sqrt((p + 1) / 10))
        ws, g, ll = _ws(getattr(lib, "dlsa_%s_workspace_bytes" % what), n, p, icpt, 1), f64(p + 1), f64(1)
        tail = (_ptr(ws), ws.numel(), _stream())
        call = {
            "poisson": lambda H, ldh: lib.dlsa_poisson_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(od), _ptr(bd), n, p, icpt, _ptr(H), ldh, _ptr(g), _ptr(ll),
                                                                None, *tail),
            "negbin": lambda H, ldh: lib.dlsa_negbin_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(od), _ptr(bd), NB_ALPHA, n, p, icpt, _ptr(H), ldh, _ptr(g),
                                                              _ptr(ll), None, None, None, *tail),
            "gamma": lambda H, ldh: lib.dlsa_gamma_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(od), _ptr(bd), 0.37, n, p, icpt, _ptr(H), ldh, _ptr(g),
                                                            _ptr(ll), None, None, *tail),
            "tweedie": lambda H, ldh: lib.dlsa_tweedie_pass_f64(_ptr(Xd), p, _ptr(yd), _ptr(od), _ptr(bd), TW_POWER, 0.37, n, p, icpt, _ptr(H), ldh,
                                                                _ptr(g), _ptr(ll), None, None, *tail),
        }[what]
        _pitched_pair(call, p + 1)
