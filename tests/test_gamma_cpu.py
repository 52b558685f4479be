"""CPU checks of the Gamma map step: the numpy reference checks itself (finite differences, the intercept-only fit, the dispersion),
combine_gamma_dispersion on hand-made blocks, the header against _lib.SIGNATURES for the six new symbols, what the engine and the
models hand to the C ABI (a recording fake library, as test_engine_marshal_cpu.py), and the Python-side refusals."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import gamma_reference as gr
import test_engine_marshal_cpu as tm
from conftest import ROOT
from dlsa_amd import _lib, engine, models
from test_engine_marshal_cpu import fake  # noqa: F401  (the recording fake library, a fixture)

SYMBOLS = ["dlsa_gamma_workspace_bytes", "dlsa_gamma_pass_f64", "dlsa_gamma_fit_f64", "dlsa_onehot_gamma_workspace_bytes",
           "dlsa_onehot_gamma_pass_f64", "dlsa_onehot_gamma_fit_f64"]


def _data(seed, n, p, intercept=True, offset=True, shape=2.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    beta = np.linspace(-0.6, 0.6, p)
    o = np.log(rng.uniform(0.5, 2.0, n)) if offset else None
    mu = np.exp(X @ beta + (0.3 if intercept else 0.0) + (0.0 if o is None else o))
    return X, rng.gamma(shape, mu / shape), o


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("dispersion", [1.0, 0.37])
def test_reference_finite_differences(intercept, offset, dispersion):
    X, y, o = _data(1, 200, 4, intercept, offset)
    pe = 4 + intercept
    b = np.linspace(-0.3, 0.4, pe)
    ll, g, H, r, P, dev = gr.terms(X, y, b, o, intercept, dispersion)
    assert np.allclose(r, y / np.exp(gr.design(X, intercept) @ b + (0 if o is None else o)))
    assert P == pytest.approx(((r - 1) ** 2).sum()) and dev == pytest.approx(2 * (r - 1 - np.log(r)).sum()) and dev > 0
    h = 1e-6
    for j in range(pe):
        e = np.zeros(pe); e[j] = h
        lp, gp = gr.terms(X, y, b + e, o, intercept, dispersion)[:2]
        lm, gm = gr.terms(X, y, b - e, o, intercept, dispersion)[:2]
        assert abs((lp - lm) / (2 * h) - g[j]) <= 1e-6 * max(1.0, abs(g[j]))
        assert np.max(np.abs((gp - gm) / (2 * h) + H[:, j])) <= 1e-6 * max(1.0, np.max(np.abs(H)))


def test_reference_loglik_is_the_gamma_density():
    """the full log-likelihood against the density written out: shape nu, scale mu / nu"""
    X, y, o = _data(2, 50, 3)
    b = np.array([0.2, -0.1, 0.3, 0.05])
    phi = 0.37
    nu = 1 / phi
    mu = np.exp(gr.design(X, True) @ b + o)
    dens = sum((nu - 1) * math.log(v) - v * nu / m - nu * math.log(m / nu) - math.lgamma(nu) for v, m in zip(y, mu))
    assert gr.terms(X, y, b, o, True, phi)[0] == pytest.approx(dens, rel=1e-12)


@pytest.mark.parametrize("offset", [False, True])
def test_intercept_only_fit_is_the_log_mean(offset):
    X, y, o = _data(3, 500, 2, True, offset)
    Z = np.zeros((500, 0))
    b = gr.fit(Z, y, o, True)[0]
    want = np.log(np.mean(y * np.exp(-(0.0 if o is None else o))))
    assert b.shape == (1,) and abs(b[0] - want) <= 1e-14 * max(1.0, abs(want))
    assert gr.start(X, y, o, True)[0] == want and not gr.start(X, y, o, True)[1:].any()


def test_reference_fit_score_vanishes_and_the_dispersion_scales_the_block():
    X, y, o = _data(4, 2000, 6)
    b, S, ll, phi, P, dev = gr.fit(X, y, o, True)
    l1, g, H, _, P1, d1 = gr.terms(X, y, b, o, True)
    assert np.max(np.abs(g)) <= 1e-10 * len(y)
    assert phi == P / (2000 - 7) and P == P1 and dev == d1 and 0.4 < phi < 0.6            # shape 2: phi = 0.5
    assert np.allclose(S, H / phi, rtol=1e-15) and np.all(np.linalg.eigvalsh(S) > 0)
    assert ll == gr.terms(X, y, b, o, True, phi)[0]
    b2, S2, ll2, phi2 = gr.fit(X, y, o, True, dispersion=0.25)[:4]
    assert np.array_equal(b, b2) and phi2 == 0.25 and np.allclose(S2, H / 0.25, rtol=1e-15)


# ---- combine_gamma_dispersion ------------------------------------------------------------------------------------------------
def _mb(status, pearson, df):
    K = len(status)
    z = torch.zeros((K, 2), dtype=torch.float64)
    return models.MappedBlocks(z, z, torch.zeros((K, 2, 2), dtype=torch.float64), ["a", "b"], status=status,
                               extra={"dispersion": [0.0] * K, "pearson": pearson, "deviance": [0.0] * K, "df": df})


def test_combine_gamma_dispersion():
    assert models.combine_gamma_dispersion(_mb([0, 0, 0], [10.0, 30.0, 20.0], [40, 60, 100])) == 60.0 / 200
    # only the partitions with status OK and degrees of freedom count
    assert models.combine_gamma_dispersion(_mb([0, 1, 4, 0, 2], [10.0, 1e9, 0.0, 20.0, 1e9], [40, 60, -2, 80, 7])) == 30.0 / 120
    assert models.combine_gamma_dispersion(_mb([0, 0], [5.0, 3.0], [0, 10])) == 0.3
    assert math.isnan(models.combine_gamma_dispersion(_mb([1, 4], [1.0, 0.0], [10, -3])))
    assert math.isnan(models.combine_gamma_dispersion(_mb([0], [1.0], [0])))


# ---- header <-> SIGNATURES -------------------------------------------------------------------------------------------------
def _ctype(decl):
    decl = decl.strip()
    name = decl.split()[-1].lstrip("*")
    kind = decl[: decl.rfind(name)].strip()
    if kind.endswith("*"):
        if name.endswith("_host"):
            return {"const int64_t*": ctypes.POINTER(_lib.c_i64), "int*": ctypes.POINTER(_lib.c_int),
                    "double*": ctypes.POINTER(_lib.c_dbl)}[kind]
        return _lib.c_vp
    return {"int64_t": _lib.c_i64, "int": _lib.c_int, "double": _lib.c_dbl, "size_t": _lib.c_sz}[kind]


@pytest.mark.parametrize("name", SYMBOLS)
def test_header_declaration_matches_the_binding(name):
    hdr = open(os.path.join(ROOT, "include", "dlsa_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "%s is not declared" % name
    res, args = _lib.SIGNATURES[name]
    assert res is {"size_t": _lib.c_sz, "int": _lib.c_int}[m.group(1)]
    assert [_ctype(a) for a in m.group(2).split(",")] == args
    # the siblings: the Gamma entries are the Poisson ones plus the dispersion arguments
    if name.endswith("workspace_bytes"):
        assert _lib.SIGNATURES[name.replace("gamma", "poisson")] == (res, args)
    elif name.endswith("fit_f64"):
        pois = _lib.SIGNATURES[name.replace("gamma", "poisson")][1]
        assert len(args) == len(pois) + 4 and args.count(_lib.c_dbl) == pois.count(_lib.c_dbl) + 1


# ---- what the wrappers hand to the C ABI --------------------------------------------------------------------------------------
DISP3 = [tm.host(tm.CD, "dispersion"), tm.host(tm.CD, "pearson"), tm.host(tm.CD, "deviance")]


def _check_gamma_result(r, pe, nrows):
    keys = ["coef", "Sig_invMcoef", "Sig_inv", "n_iter", "status", "loglik", "dispersion", "pearson", "deviance"]
    assert list(r) == keys + ["rc", "df"]
    for key, shape in (("coef", (tm.K, pe)), ("Sig_invMcoef", (tm.K, pe)), ("Sig_inv", (tm.K, pe, pe))):
        assert tuple(r[key].shape) == shape and r[key].dtype == torch.float64 and r[key].is_contiguous(), key
    assert all(type(v) is float for k in keys[5:] for v in r[k])
    assert r["df"] == [m - pe for m in nrows] and all(type(v) is int for v in r["df"])


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("dispersion", [None, 0.75])
def test_gamma_fit_ex(fake, step, icpt, with_offset, dispersion):  # noqa: F811
    X, y, offset = tm.rows()
    offset = offset if with_offset else None
    first, nrows = tm.PARTS[step]
    r = engine.gamma_fit_ex(X, y, first, nrows, row_step=step, offset=offset, fit_intercept=icpt, dispersion=dispersion, tol=1e-9, max_iter=17)
    _check_gamma_result(r, tm.P + int(icpt), nrows)
    tm.check_call(fake, "dlsa_gamma_fit_f64",
                  [tm.ptr(X), tm.val(4), tm.ptr(y), tm.ptr(offset), tm.arr(tm.I64, first), tm.arr(tm.I64, nrows), tm.val(step), tm.val(tm.K),
                   tm.val(tm.P), tm.val(int(icpt)), tm.val(0.0 if dispersion is None else dispersion), tm.val(1e-9), tm.val(17)]
                  + tm.OUT3 + tm.HOST3 + DISP3 + tm.TAIL, r)
    assert fake.ws_calls == [("dlsa_gamma_workspace_bytes", (4, tm.P, int(icpt), step))]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("dispersion", [None, 0.75])
def test_onehot_gamma_fit_ex(fake, step, with_offset, dispersion):  # noqa: F811
    plan, num, codes = tm.raw()
    _, y, offset = tm.rows()
    offset = offset if with_offset else None
    first, nrows = tm.PARTS[step]
    r = engine.onehot_gamma_fit_ex(plan, num, codes, y, first, nrows, row_step=step, offset=offset, dispersion=dispersion, tol=1e-9, max_iter=17)
    _check_gamma_result(r, tm.PLAN_P, nrows)
    tm.check_call(fake, "dlsa_onehot_gamma_fit_f64",
                  tm.raw_spec(num, codes) + [tm.ptr(y), tm.ptr(offset), tm.arr(tm.I64, first), tm.arr(tm.I64, nrows), tm.val(step), tm.val(tm.K),
                                             tm.val(0.0 if dispersion is None else dispersion), tm.val(1e-9), tm.val(17)]
                  + tm.OUT3 + tm.HOST3 + DISP3 + tm.TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_gamma_workspace_bytes" and fake.ws_calls[0][1][1:] == (4, step)


def _check_pass(res, pe, want_H, want_w, want_stats):
    assert isinstance(res, tuple) and len(res) == 5
    for t, shape, want in zip(res, [(pe, pe), (pe,), (1,), (tm.N,), (2,)], [want_H, True, True, want_w, want_stats]):
        if not want:
            assert t is None
        else:
            assert tuple(t.shape) == shape and t.dtype == torch.float64 and t.is_contiguous()
    return dict(zip(["H", "g", "ll", "w", "st"], res))


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w,want_stats", [(True, False, False), (False, True, False), (False, False, True)])
def test_gamma_pass(fake, icpt, with_offset, want_H, want_w, want_stats):  # noqa: F811
    X, y, offset = tm.rows()
    offset = offset if with_offset else None
    pe = tm.P + int(icpt)
    beta = torch.zeros(pe, dtype=torch.float64)
    res = engine.gamma_pass(X, y, beta, 0.75, offset=offset, fit_intercept=icpt, want_H=want_H, want_w=want_w, want_stats=want_stats)
    r = _check_pass(res, pe, want_H, want_w, want_stats)
    tm.check_call(fake, "dlsa_gamma_pass_f64",
                  [tm.ptr(X), tm.val(4), tm.ptr(y), tm.ptr(offset), tm.ptr(beta), tm.val(0.75), tm.val(tm.N), tm.val(tm.P), tm.val(int(icpt)),
                   tm.out("H"), tm.val(pe), tm.out("g"), tm.out("ll"), tm.out("w"), tm.out("st")] + tm.TAIL, r)
    assert fake.ws_calls == [("dlsa_gamma_workspace_bytes", (tm.N, tm.P, int(icpt), 1))]


@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w,want_stats", [(True, False, False), (False, True, False), (False, False, True)])
def test_onehot_gamma_pass(fake, with_offset, want_H, want_w, want_stats):  # noqa: F811
    plan, num, codes = tm.raw()
    _, y, offset = tm.rows()
    offset = offset if with_offset else None
    beta = torch.zeros(tm.PLAN_P, dtype=torch.float64)
    res = engine.onehot_gamma_pass(plan, num, codes, y, beta, 0.75, offset=offset, want_H=want_H, want_w=want_w, want_stats=want_stats)
    r = _check_pass(res, tm.PLAN_P, want_H, want_w, want_stats)
    tm.check_call(fake, "dlsa_onehot_gamma_pass_f64",
                  tm.raw_spec(num, codes) + [tm.ptr(y), tm.ptr(offset), tm.ptr(beta), tm.val(0.75), tm.val(tm.N), tm.out("H"), tm.val(tm.PLAN_P),
                                             tm.out("g"), tm.out("ll"), tm.out("w"), tm.out("st")] + tm.TAIL, r)


def test_pass_defaults_are_unit_dispersion_and_no_stats(fake):  # noqa: F811
    X, y, _ = tm.rows()
    H, g, ll, w, st = engine.gamma_pass(X, y, torch.zeros(tm.P, dtype=torch.float64))
    assert H is not None and w is None and st is None and fake.calls[0][1][5] == 1.0


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it is on the GPU: lets the models' own checks pass in front of the fake library"""
    is_cuda = property(lambda self: True)


def _on_device(t):
    return None if t is None else torch.Tensor._make_subclass(_OnDevice, t)


@pytest.mark.parametrize("dispersion", [None, 0.75])
@pytest.mark.parametrize("with_exposure", [False, True])
def test_fit_gamma_partitions_marshals(fake, dispersion, with_exposure):  # noqa: F811
    X, y, _ = tm.rows()
    X, y = _on_device(X), _on_device(y + 0.5)               # (rows() draws counts 0 .. 2: made positive)
    e = torch.linspace(0.5, 2.0, tm.N, dtype=torch.float64) if with_exposure else None
    mb = models.fit_gamma_partitions(X, y, partition_num=2, fit_intercept=True, exposure=e, dispersion=dispersion, tol=1e-9, max_iter=17)
    name, a = fake.calls[0]
    first, nrows = tm.PARTS[2]
    assert name == "dlsa_gamma_fit_f64" and len(fake.calls) == 1 and len(a) == len(_lib.SIGNATURES[name][1])
    assert tm.addr(a[0]) == X.data_ptr() and a[1] == 4 and tm.addr(a[2]) == y.data_ptr()
    if with_exposure:                                        # the offset the kernel reads is a tensor of its own: log(exposure)
        assert tm.addr(a[3]) not in (0, e.data_ptr())
    else:
        assert tm.addr(a[3]) == 0
    assert list(a[4]) == first and list(a[5]) == nrows and a[6:13] == (2, 2, tm.P, 1, 0.0 if dispersion is None else dispersion, 1e-9, 17)
    assert mb.names == ["intercept", "x0", "x1", "x2"] and mb.sample_size == tm.N
    assert list(mb.extra) == ["dispersion", "pearson", "deviance", "df"] and mb.extra["df"] == [m - 4 for m in nrows]
    # every host list came from its own output array (the fake writes 100 * position + k)
    for key, pos in (("dispersion", 19), ("pearson", 20), ("deviance", 21)):
        assert mb.extra[key] == [100.0 * pos, 100.0 * pos + 1]
    assert mb.loglik == [1800.0, 1801.0] and mb.status == [1700, 1701]


@pytest.mark.parametrize("structured", [True, False])
def test_fit_gamma_design_marshals(fake, structured):  # noqa: F811
    plan, num, codes = tm.raw()
    _, y, offset = tm.rows()
    y = _on_device(y + 0.5)
    Xbuilt = torch.rand((tm.N, tm.PLAN_P), dtype=torch.float64)
    spec = types.SimpleNamespace(onehot_plan=lambda: plan, names=["c%d" % i for i in range(tm.PLAN_P)], build=lambda n, c: (Xbuilt, None))
    mb = models.fit_gamma_design(num, codes, y, spec, part_offsets=tm.OFFS, offset=offset, dispersion=0.75, structured=structured, tol=1e-9,
                                 max_iter=17)
    name, a = fake.calls[0]
    first, nrows = tm.PARTS[1]
    if structured:
        assert name == "dlsa_onehot_gamma_fit_f64"
        assert tm.addr(a[0]) == tm.PLAN_H and tm.addr(a[1]) == num.data_ptr() and tm.addr(a[3]) == codes.data_ptr()
        assert tm.addr(a[5]) == y.data_ptr() and tm.addr(a[6]) == offset.data_ptr()
        assert list(a[7]) == first and list(a[8]) == nrows and a[9:14] == (1, 2, 0.75, 1e-9, 17)
    else:                                                     # the dense fit on the built matrix, no implicit intercept
        assert name == "dlsa_gamma_fit_f64"
        assert tm.addr(a[0]) == Xbuilt.data_ptr() and tm.addr(a[2]) == y.data_ptr() and tm.addr(a[3]) == offset.data_ptr()
        assert list(a[4]) == first and list(a[5]) == nrows and a[6:13] == (1, 2, tm.PLAN_P, 0, 0.75, 1e-9, 17)
    assert mb.names == spec.names and mb.extra["df"] == [m - tm.PLAN_P for m in nrows]


# ---- the Python-side refusals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_a_response_that_is_not_positive_is_refused(fake, bad):  # noqa: F811
    X, y, _ = tm.rows()
    y = y + 0.5
    y[3] = bad
    with pytest.raises(ValueError, match="fit_gamma_partitions: the response must be positive"):
        models.fit_gamma_partitions(_on_device(X), _on_device(y), fit_intercept=True)
    plan, num, codes = tm.raw()
    spec = types.SimpleNamespace(onehot_plan=lambda: plan, names=[])
    with pytest.raises(ValueError, match="fit_gamma_design: the response must be positive"):
        models.fit_gamma_design(num, codes, _on_device(y), spec)
    assert fake.calls == []


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan"), float("inf")])
def test_a_dispersion_that_is_not_positive_is_refused(fake, bad):  # noqa: F811
    X, y, _ = tm.rows()
    X, y = _on_device(X), _on_device(y + 0.5)
    plan, num, codes = tm.raw()
    beta = torch.zeros(tm.P, dtype=torch.float64)
    with pytest.raises(ValueError, match="dispersion must be positive"):
        models.fit_gamma_partitions(X, y, dispersion=bad)
    with pytest.raises(ValueError, match="dispersion must be positive"):
        models.fit_gamma_design(num, codes, y, types.SimpleNamespace(onehot_plan=lambda: plan, names=[]), dispersion=bad)
    with pytest.raises(ValueError, match="^gamma_fit_ex: dispersion must be positive"):
        engine.gamma_fit_ex(X, y, *tm.PARTS[1], dispersion=bad)
    with pytest.raises(ValueError, match="^onehot_gamma_fit_ex: dispersion must be positive"):
        engine.onehot_gamma_fit_ex(plan, num, codes, y, *tm.PARTS[1], dispersion=bad)
    with pytest.raises(ValueError, match="^gamma_pass: dispersion must be positive"):
        engine.gamma_pass(X, y, beta, bad)
    with pytest.raises(ValueError, match="^onehot_gamma_pass: dispersion must be positive"):
        engine.onehot_gamma_pass(plan, num, codes, y, torch.zeros(tm.PLAN_P, dtype=torch.float64), bad)
    assert fake.calls == []


def test_offset_and_exposure_together_are_refused(fake):  # noqa: F811
    X, y, offset = tm.rows()
    with pytest.raises(ValueError, match="an offset or an exposure, not both"):
        models.fit_gamma_partitions(_on_device(X), _on_device(y + 0.5), offset=offset, exposure=torch.exp(offset))
    with pytest.raises(ValueError, match="exposure must be positive"):
        models.fit_gamma_partitions(_on_device(X), _on_device(y + 0.5), exposure=offset - 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        models.fit_gamma_partitions(X, y + 0.5)
    assert fake.calls == []


def test_the_c_abi_refuses_before_any_hip_call():
    """argument validation of the new entries happens before any HIP call, so it runs without a GPU"""
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    i64 = ctypes.c_int64
    assert lib.dlsa_gamma_workspace_bytes(1000, 0, 0, 1) == 0 and lib.dlsa_gamma_workspace_bytes(1000, 5, 1, 0) == 0
    assert lib.dlsa_gamma_workspace_bytes(1000, 2048, 1, 1) == 0
    assert lib.dlsa_gamma_workspace_bytes(1000, 5, 1, 2) > lib.dlsa_gamma_workspace_bytes(1000, 5, 1, 1) > 0
    assert lib.dlsa_onehot_gamma_workspace_bytes(None, 10, 1) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dlsa_gamma_pass_f64(one, 4, one, None, one, bad, 10, 4, 1, None, 0, None, None, None, None, one, 1 << 30, None) == 1
        assert "dispersion" in _lib.last_error()
    assert lib.dlsa_gamma_pass_f64(None, 4, one, None, one, 1.0, 10, 4, 1, None, 0, None, None, None, None, one, 1 << 30, None) == 1
    assert "null" in _lib.last_error()
    assert lib.dlsa_gamma_pass_f64(one, 4, one, None, one, 1.0, 10, 4, 1, None, 0, None, None, None, None, one, 16, None) == 3
    first, rows = (i64 * 2)(0, 5), (i64 * 2)(5, 5)
    fit = lambda disp, ws_bytes=16: lib.dlsa_gamma_fit_f64(one, 4, one, None, first, rows, 1, 2, 4, 1, disp, 1e-13, 100, one, one, one,  # noqa: E731
                                                          None, None, None, None, None, None, one, ws_bytes, None)
    assert fit(float("inf")) == 1 and "finite" in _lib.last_error()
    assert fit(0.0) == 3 and fit(0.5) == 3                   # a valid call stops at the workspace check
    assert lib.dlsa_onehot_gamma_fit_f64(None, None, 0, None, 0, one, None, first, rows, 1, 2, 0.0, 1e-13, 100, one, one, one, None, None,
                                         None, None, None, None, one, 16, None) == 1
