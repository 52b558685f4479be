"""GPU: the LARS / lasso path at the widths lars_c.hip serves (449 <= m = p - intercept <= 2044) and just beyond (lars.hip), held
against an oracle-free certificate of the path (tests/lars_certificate.py: equicorrelation, step support, breakpoints, lasso signs,
monotone C, the final point, RSS / dof / AIC / BIC / beta0) on every case, and against the oracle's restatement of lsa.py:90-212
wherever it finishes in seconds (m <= 1100) and once at m = 2044.

The oracle runs in worker processes (numpy only, no GPU) started when the module's first test asks for one, so that its minutes
overlap the GPU runs and the certificates.  Every GPU run reads the grid-abort count (dlsa_lars_grid_barrier_timeout(0.0)) before
and after: a path that came from the silent rerun on lars.hip's single workgroup did not test lars_c.hip."""
import concurrent.futures
import multiprocessing
import os
import time

import numpy as np
import pytest

import lars_certificate as lc
from lars_problems import oracle_path, problem

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WIDTHS = [449, 450, 463, 464, 465, 511, 512, 513, 767, 1020, 1021, 1023, 1024, 1025, 1536, 2043, 2044]
COMBOS = [("lar", 0.5), ("lasso", 0.97), ("lasso", 0.5), ("lar", 0.97)]
ORACLE_MAX_M = 1100
# every width with and without the intercept (p = m + intercept), lar / lasso at rho 0.5 / 0.97 in turn; the oracle once at m = 2044
WIDE = []
for _i, (_m, _icpt) in enumerate((m, icpt) for m in WIDTHS for icpt in (False, True)):
    _typ, _rho = ("lasso", 0.97) if (_m, _icpt) == (2044, False) else COMBOS[_i % 4]
    WIDE.append((_m, _icpt, _typ, _rho, _m <= ORACLE_MAX_M or (_m, _icpt) == (2044, False)))
WIDE.append((2045, False, "lasso", 0.97, False))              # lars.hip's grid kernel

# degenerate inputs at m ~ 500 .. 1400 (kind, p, intercept, type); 'rankdef' (n = p / 2 rows) up to max_steps = n / 2, also against the oracle
DEGENERATE = [("zerocol", 517, False, "lasso"), ("zerocol", 1101, True, "lar"), ("ties", 640, False, "lar"), ("ties", 1280, False, "lasso"),
              ("tinyb", 703, True, "lasso"), ("tinyb", 1399, False, "lar"), ("pairs", 560, False, "lasso"), ("pairs", 1203, True, "lar"),
              ("rankdef", 480, False, "lasso"), ("rankdef", 530, True, "lar")]

# seeds moved on where the first one gives a lasso path at rho 0.97 without a drop (checked on the oracle's paths)
SEED_SHIFT = {(463, True): 1, (2044, True): 1}
REPORT = {}


def _spec_wide(m, icpt, rho):
    return ("corr", m + int(icpt), rho, 5000 + m + 7 * int(icpt) + SEED_SHIFT.get((m, icpt), 0))


def _spec_deg(kind, p):
    return (kind, p, 0.0, 6000 + p)


def _oracle_jobs():
    jobs = [(_spec_wide(m, icpt, rho), icpt, typ, None) for m, icpt, typ, rho, orc in WIDE if orc]
    jobs += [(_spec_deg(k, p), icpt, typ, p // 4) for k, p, icpt, typ in DEGENERATE if k == "rankdef"]
    return sorted(jobs, key=lambda j: -j[0][1])                 # the widest first: they bound the wall time


@pytest.fixture(scope="module")
def oracle():
    """job -> future of the oracle's path.  The workers are spawned (never forked from a process that holds the GPU), with one BLAS
    thread each: the oracle's steps are small mat-vecs and copies, and six workers with a full thread pool each only contend."""
    ctx = multiprocessing.get_context("spawn")
    jobs = _oracle_jobs()
    threads = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")
    saved = {k: os.environ.get(k) for k in threads}
    os.environ.update({k: "1" for k in threads})           # read by the workers as they start (all of them start on the submits)
    try:
        ex = concurrent.futures.ProcessPoolExecutor(max_workers=min(6, len(jobs)), mp_context=ctx)
        futs = {j: ex.submit(oracle_path, j) for j in jobs}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield lambda job: futs[job].result(timeout=900)
    finally:
        ex.shutdown(wait=True, cancel_futures=True)


@pytest.fixture(scope="module")
def eng():
    from dlsa_amd import engine
    assert torch.cuda.is_available()
    return engine


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    lines = ["lars wide: %.0f s" % (time.time() - t0)]
    for key in sorted(REPORT):
        lines.append("  %-22s certificate %.1e  oracle %s" % (key, REPORT[key][0], "%.1e" % REPORT[key][1] if REPORT[key][1] is not None else "-"))
    print("\n".join(lines))


def rel_inf(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _width_class(m):
    return "m 449..512" if m <= 512 else "m 513..1024" if m <= 1024 else "m 1025..2044" if m <= 2044 else "m 2045 (lars.hip)"


def _note(cls, cert, orc=None):
    c, o = REPORT.get(cls, (0.0, None))
    REPORT[cls] = (max(c, cert), o if orc is None else max(o or 0.0, orc))


def _run(eng, S, b, icpt, n, typ, max_steps=None, **opts):
    """the device path; fails when a grid barrier gave up and lars.hip's single workgroup produced it"""
    from dlsa_amd import _lib
    lib = _lib.load()
    before = lib.dlsa_lars_grid_barrier_timeout(0.0)
    with eng.kernel_options(**opts) if opts else eng.kernel_options():
        r = eng.lars_path(torch.from_numpy(S).cuda(), torch.from_numpy(b).cuda(), icpt, float(n), type=typ, max_steps=max_steps)
    out = {k: r[k].cpu().numpy() for k in ("beta", "beta0", "AIC", "BIC")}
    assert lib.dlsa_lars_grid_barrier_timeout(0.0) == before, "a grid launch aborted: the path came from the single-workgroup rerun"
    return out


def _against_oracle(r, ro, icpt):
    assert r["beta"].shape == ro["beta"].shape, (r["beta"].shape, ro["beta"].shape)
    e = max(rel_inf(r[k], ro[k]) for k in ("beta", "AIC", "BIC") + (("beta0",) if icpt else ()))
    assert e < 1e-7, e
    return e


@pytest.mark.parametrize("m,icpt,typ,rho,with_oracle", WIDE)
def test_wide_path_is_certified(eng, oracle, m, icpt, typ, rho, with_oracle):
    spec = _spec_wide(m, icpt, rho)
    S, b, n = problem(spec)
    r = _run(eng, S, b, icpt, n, typ)
    if typ == "lasso" and rho > 0.9:
        assert r["beta"].shape[0] > m + 1                       # the path has drops
    res = lc.certify(S, b, icpt, n, typ, r)
    e = _against_oracle(r, oracle((spec, icpt, typ, None)), icpt) if with_oracle else None
    _note(_width_class(m), max(res.values()), e)


@pytest.mark.parametrize("m,icpt", [(700, False), (1101, True), (2044, True)])
def test_any_workgroup_count_walks_the_certified_path(eng, m, icpt):
    """lars_wgs decides which 16-column blocks a workgroup owns (NBW = blocks per workgroup; 2, 3, 5 and 17 workgroups put the
    emits of the new Q / RT rows on several waves) and how many row groups sum them -- never the path.  Against the default count:
    the same step count and the path to 1e-8 (the sums differ only in their order; the bound of the count test in test_gpu_kernels.py)."""
    S, b, n = problem(_spec_wide(m, icpt, 0.97))
    r0 = _run(eng, S, b, icpt, n, "lasso")
    worst = 0.0
    for wgs in (2, 3, 5, 17, 33, 64):
        r = _run(eng, S, b, icpt, n, "lasso", lars_wgs=wgs)
        assert r["beta"].shape == r0["beta"].shape, wgs
        e = max(rel_inf(r[k], r0[k]) for k in ("beta", "AIC", "BIC") + (("beta0",) if icpt else ()))
        assert e < 1e-8, (wgs, e)
        worst = max(worst, e)
        _note("workgroup counts", max(lc.certify(S, b, icpt, n, "lasso", r).values()))
    print("m = %d: workgroup counts 2 .. 64 against the default, worst %.1e" % (m, worst))


@pytest.mark.parametrize("kind,p,icpt,typ", DEGENERATE)
def test_degenerate_inputs(eng, oracle, kind, p, icpt, typ):
    spec = _spec_deg(kind, p)
    S, b, n = problem(spec)
    ms = p // 4 if kind == "rankdef" else None                 # (n = p / 2 rows: the active set stays below the rank)
    r = _run(eng, S, b, icpt, n, typ, max_steps=ms)
    res = lc.certify(S, b, icpt, n, typ, r, max_steps=ms)
    e = _against_oracle(r, oracle((spec, icpt, typ, ms)), icpt) if kind == "rankdef" else None
    _note("degenerate " + kind, max(res.values()), e)


@pytest.mark.parametrize("m,icpt,typ", [(1101, True, "lasso"), (2044, False, "lar")])
def test_max_steps_gives_the_prefix_of_the_full_path(eng, m, icpt, typ):
    S, b, n = problem(_spec_wide(m, icpt, 0.97))
    full = _run(eng, S, b, icpt, n, typ)
    K = full["beta"].shape[0] // 3
    cut = _run(eng, S, b, icpt, n, typ, max_steps=K)
    assert cut["beta"].shape[0] == K + 1
    for k in ("beta", "beta0", "AIC", "BIC"):
        assert np.array_equal(cut[k], full[k][: K + 1]), k
    lc.certify(S, b, icpt, n, typ, cut, max_steps=K)
