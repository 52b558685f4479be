"""CPU checks of the Tweedie map step: the numpy reference checks itself (finite differences, the dispersion sums row by row with
rows at y = 0, the intercept-only fit, a longdouble run of itself on the GPU tests' inputs, the calibration band of
test_block_is_calibrated), combine_tweedie_dispersion on hand-made blocks, the header against _lib.SIGNATURES for the six new
symbols, what the engine and the models hand to the C ABI (a recording fake library, as test_engine_marshal_cpu.py), the
Python-side refusals and simulate_tweedie's draws."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import test_engine_marshal_cpu as tm
import tweedie_reference as tr
from conftest import ROOT
from dlsa_amd import _lib, engine, models
from test_engine_marshal_cpu import fake  # noqa: F401  (the recording fake library, a fixture)

SYMBOLS = ["dlsa_tweedie_workspace_bytes", "dlsa_tweedie_pass_f64", "dlsa_tweedie_fit_f64", "dlsa_onehot_tweedie_workspace_bytes",
           "dlsa_onehot_tweedie_pass_f64", "dlsa_onehot_tweedie_fit_f64"]
L = np.longdouble


def lrel(a, b):
    a, b = np.asarray(a, L), np.asarray(b, L)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("intercept,offset", [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("power,dispersion", [(1.5, 1.0), (1.2, 0.37), (1.8, 2.5)])
def test_reference_finite_differences(intercept, offset, power, dispersion):
    X, y, o = tr.data(1, 200, 4, intercept, offset, power)
    assert (y == 0).any()
    pe = 4 + intercept
    b = np.linspace(-0.3, 0.4, pe)
    ll, g, H, w, P, dev = tr.terms(X, y, b, power, o, intercept, dispersion)
    assert np.all(w > 0)                                      # the observed weight: the negative quasi-log-likelihood is convex
    h = 1e-6
    for j in range(pe):
        e = np.zeros(pe); e[j] = h
        lp, gp = tr.terms(X, y, b + e, power, o, intercept, dispersion)[:2]
        lm, gm = tr.terms(X, y, b - e, power, o, intercept, dispersion)[:2]
        assert abs((lp - lm) / (2 * h) - g[j]) <= 1e-6 * max(1.0, abs(g[j]))
        assert np.max(np.abs((gp - gm) / (2 * h) + H[:, j])) <= 1e-6 * max(1.0, np.max(np.abs(H)))


@pytest.mark.parametrize("power", [1.2, 1.5, 1.8])
def test_dispersion_sums_row_by_row(power):
    """P and Dev written out with math.pow per row; a row at y = 0 contributes mu^(2 - xi) to P and 2 mu^(2 - xi) / (2 - xi) to Dev.
    The unit deviance is the one of the textbooks: 2 (y (y^(1 - xi) - mu^(1 - xi)) / (1 - xi) - (y^(2 - xi) - mu^(2 - xi)) / (2 - xi))."""
    X, y, o = tr.data(5, 60, 3, True, True, power)
    y[:3] = 0.0
    b = np.array([0.2, -0.1, 0.3, 0.05])
    mu = np.exp(tr.design(X, True) @ b + o)
    P = dev = 0.0
    for v, m in zip(y, mu):
        P += (v - m) ** 2 / math.pow(m, power)
        if v == 0.0:
            dev += 2.0 * math.pow(m, 2 - power) / (2 - power)
        else:
            dev += 2.0 * (v * (math.pow(v, 1 - power) - math.pow(m, 1 - power)) / (1 - power)
                          - (math.pow(v, 2 - power) - math.pow(m, 2 - power)) / (2 - power))
    got = tr.terms(X, y, b, power, o, True, 0.7)
    assert got[4] == pytest.approx(P, rel=1e-13) and got[5] == pytest.approx(dev, rel=1e-12) and dev > 0
    # all-zero responses: P = sum mu^(2 - xi), Dev = 2 sum mu^(2 - xi) / (2 - xi), nothing else
    z = tr.terms(X, np.zeros(60), b, power, o, True)
    s = float((mu ** (2 - power)).sum())
    assert np.isfinite(z[5]) and z[4] == pytest.approx(s, rel=1e-13) and z[5] == pytest.approx(2 * s / (2 - power), rel=1e-13)
    # the quasi-log-likelihood and the deviance differ by a term free of beta: Dev + 2 sum q = 2 sum y^(2 - xi) / ((1 - xi)(2 - xi))
    c = 2.0 * float((y[y > 0] ** (2 - power)).sum()) / ((1 - power) * (2 - power))
    one = tr.terms(X, y, b, power, o, True)
    assert one[5] + 2 * one[0] == pytest.approx(c, rel=1e-12)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("power", [1.2, 1.5, 1.8])
def test_intercept_only_fit_reproduces_the_start(offset, power):
    X, y, o = tr.data(3, 500, 2, True, offset, power)
    Z = np.zeros((500, 0))
    b = tr.fit(Z, y, power, o, True)[0]
    oo = np.zeros(500) if o is None else o
    want = np.log((y * np.exp((1 - power) * oo)).sum() / np.exp((2 - power) * oo).sum())
    assert b.shape == (1,) and abs(b[0] - want) <= 1e-14 * max(1.0, abs(want))
    assert tr.start(X, y, power, o, True)[0] == pytest.approx(want, rel=1e-15) and not tr.start(X, y, power, o, True)[1:].any()
    if not offset:
        assert want == pytest.approx(math.log(y.mean()), rel=1e-14)
    assert abs(tr.terms(Z, y, b, power, o, True)[1][0]) <= 1e-10 * len(y)        # the score vanishes there


def test_reference_fit_score_vanishes_and_the_dispersion_scales_the_block():
    power = 1.5
    X, y, o = tr.data(4, 2000, 6, True, True, power)
    b, S, ll, phi, P, dev = tr.fit(X, y, power, o, True)
    l1, g, H, _, P1, d1 = tr.terms(X, y, b, power, o, True)
    assert np.max(np.abs(g)) <= 1e-10 * len(y)
    assert phi == P / (2000 - 7) and P == P1 and dev == d1 and 0.65 < phi < 0.95           # drawn at 0.8
    assert np.allclose(S, H / phi, rtol=1e-15) and np.all(np.linalg.eigvalsh(S) > 0)
    assert ll == tr.terms(X, y, b, power, o, True, phi)[0] and ll == pytest.approx(l1 / phi, rel=1e-15)
    b2, S2, ll2, phi2 = tr.fit(X, y, power, o, True, dispersion=0.25)[:4]
    assert np.array_equal(b, b2) and phi2 == 0.25 and np.allclose(S2, H / 0.25, rtol=1e-15)
    # beta depends on the power
    assert np.max(np.abs(tr.fit(X, y, 1.2, o, True)[0] - b)) > 1e-4


WIDE = 8      # columns of H compared at widths where a longdouble H takes seconds


@pytest.mark.parametrize("p", [1, 7, 50, 100, 130, 260, 500, 600])
@pytest.mark.parametrize("power", [1.1, 1.5, 1.9])
def test_reference_against_its_longdouble_run(p, power):
    """the inputs of test_gpu_tweedie.test_pass_matches_reference: the headroom under its 1e-12 (measured: <= 2e-15)"""
    n = 3 * p + 37
    X, y, o = tr.data(10 + p, n, p, True, True, power)
    b = tr.away_from_optimum(p + 1)
    cols = None if p <= 130 else WIDE
    got = tr.terms(X, y, b, power, o, True, 0.37, h_cols=cols)
    want = tr.terms(X, y, b, power, o, True, 0.37, L, h_cols=cols)
    errs = [lrel(u, v) for u, v in zip(got, want)]
    print("p=%d power=%g: ll %.1e g %.1e H %.1e w %.1e P %.1e Dev %.1e" % (p, power, *errs))
    assert max(errs) <= 1e-13


@pytest.mark.parametrize("power", [1.5, 1.2])
def test_reference_against_its_longdouble_run_eta_span(power):
    """the inputs of test_pass_eta_spanning_600 (measured: <= 8e-15 at 1.5, <= 2.7e-14 at 1.2: the rounding of (1 - xi) eta at |eta| =
    300); every quantity stays finite"""
    X, y, o, b = tr.eta_span_case(power)
    got = tr.terms(X, y, b, power, o, True)
    want = tr.terms(X, y, b, power, o, True, 1.0, L)
    assert all(np.isfinite(np.asarray(v, float)).all() for v in got)
    errs = [lrel(u, v) for u, v in zip(got, want)]
    print("eta span, power=%g: ll %.1e g %.1e H %.1e w %.1e P %.1e Dev %.1e" % (power, *errs))
    assert max(errs) <= 1e-13


@pytest.mark.parametrize("p", [1, 7, 50])
def test_reference_fit_against_its_longdouble_run(p):
    """the inputs of test_fit_matches_reference, first partition: the headroom under its 1e-10"""
    n = max(2000, 10 * p)
    X, y, o = tr.data(40 + p, n, p, True, True)
    sl = slice(0, int(0.30 * n))
    got = tr.fit(X[sl], y[sl], 1.5, o[sl], True)
    want = tr.fit(X[sl], y[sl], 1.5, o[sl], True, dtype=L)
    errs = [lrel(u, v) for u, v in zip(got, want)]
    print("fit p=%d: coef %.1e Sig_inv %.1e ll %.1e phi %.1e P %.1e Dev %.1e" % (p, *errs))
    assert max(errs) <= 1e-12


@pytest.mark.parametrize("power,dispersion", tr.CALIBRATION)
def test_calibration_band_separates_the_scaling_mistakes(power, dispersion):
    """the design and seed of test_gpu_tweedie.test_block_is_calibrated on the reference alone: Q lies inside 240 +- 3 sqrt(480), the
    unscaled blocks' Q outside (measured: 229.5 / 69.0 at (1.8, 0.3), 249.2 / 491.8 at (1.2, 2.0))"""
    K, m = 40, 1500
    X, y, o = tr.calibration_case(power, dispersion, K, m)
    fits = [tr.fit(X[k * m:(k + 1) * m], y[k * m:(k + 1) * m], power, o[k * m:(k + 1) * m], True) for k in range(K)]
    coef, S, phi = np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), np.array([f[3] for f in fits])
    q, q_unscaled = tr.calibration_q(coef, S), tr.calibration_q(coef, S * phi[:, None, None])
    pooled = sum(f[4] for f in fits) / (K * (m - 6))
    print("(%g, %g): Q %.1f, unscaled %.1f, pooled dispersion %.4f" % (power, dispersion, q, q_unscaled, pooled))
    assert 174.0 <= q <= 306.0 and not 174.0 <= q_unscaled <= 306.0
    assert abs(pooled - dispersion) <= 0.04 * dispersion


# ---- combine_tweedie_dispersion ----------------------------------------------------------------------------------------------
def _mb(status, pearson, df):
    K = len(status)
    z = torch.zeros((K, 2), dtype=torch.float64)
    return models.MappedBlocks(z, z, torch.zeros((K, 2, 2), dtype=torch.float64), ["a", "b"], status=status,
                               extra={"dispersion": [0.0] * K, "pearson": pearson, "deviance": [0.0] * K, "df": df})


def test_combine_tweedie_dispersion():
    cases = [([0, 0, 0], [10.0, 30.0, 20.0], [40, 60, 100]), ([0, 1, 4, 0, 2], [10.0, 1e9, 0.0, 20.0, 1e9], [40, 60, -2, 80, 7]),
             ([0, 0], [5.0, 3.0], [0, 10])]
    for want, case in zip([60.0 / 200, 30.0 / 120, 0.3], cases):
        assert models.combine_tweedie_dispersion(_mb(*case)) == want
        assert models.combine_gamma_dispersion(_mb(*case)) == want          # one implementation, the Gamma one's behaviour
    assert math.isnan(models.combine_tweedie_dispersion(_mb([1, 4], [1.0, 0.0], [10, -3])))
    assert math.isnan(models.combine_tweedie_dispersion(_mb([0], [1.0], [0])))


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
    names = [a.split()[-1].lstrip("*") for a in m.group(2).split(",")]
    # the siblings: the Tweedie entries are the Gamma ones with `power` in front of the dispersion
    gamma = _lib.SIGNATURES[name.replace("tweedie", "gamma")]
    if name.endswith("workspace_bytes"):
        assert gamma == (res, args)
    else:
        at = names.index("power")
        assert names[at + 1] in ("dispersion", "dispersion_fixed") and args[at] is _lib.c_dbl
        assert gamma == (res, args[:at] + args[at + 1:])


# ---- what the wrappers hand to the C ABI --------------------------------------------------------------------------------------
DISP3 = [tm.host(tm.CD, "dispersion"), tm.host(tm.CD, "pearson"), tm.host(tm.CD, "deviance")]


def _check_result(r, pe, nrows):
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
def test_tweedie_fit_ex(fake, step, icpt, with_offset, dispersion):  # noqa: F811
    X, y, offset = tm.rows()
    offset = offset if with_offset else None
    first, nrows = tm.PARTS[step]
    r = engine.tweedie_fit_ex(X, y, first, nrows, row_step=step, offset=offset, fit_intercept=icpt, power=1.3, dispersion=dispersion,
                              tol=1e-9, max_iter=17)
    _check_result(r, tm.P + int(icpt), nrows)
    tm.check_call(fake, "dlsa_tweedie_fit_f64",
                  [tm.ptr(X), tm.val(4), tm.ptr(y), tm.ptr(offset), tm.arr(tm.I64, first), tm.arr(tm.I64, nrows), tm.val(step), tm.val(tm.K),
                   tm.val(tm.P), tm.val(int(icpt)), tm.val(1.3), tm.val(0.0 if dispersion is None else dispersion), tm.val(1e-9), tm.val(17)]
                  + tm.OUT3 + tm.HOST3 + DISP3 + tm.TAIL, r)
    assert fake.ws_calls == [("dlsa_tweedie_workspace_bytes", (4, tm.P, int(icpt), step))]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("dispersion", [None, 0.75])
def test_onehot_tweedie_fit_ex(fake, step, with_offset, dispersion):  # noqa: F811
    plan, num, codes = tm.raw()
    _, y, offset = tm.rows()
    offset = offset if with_offset else None
    first, nrows = tm.PARTS[step]
    r = engine.onehot_tweedie_fit_ex(plan, num, codes, y, first, nrows, row_step=step, offset=offset, power=1.3, dispersion=dispersion,
                                     tol=1e-9, max_iter=17)
    _check_result(r, tm.PLAN_P, nrows)
    tm.check_call(fake, "dlsa_onehot_tweedie_fit_f64",
                  tm.raw_spec(num, codes) + [tm.ptr(y), tm.ptr(offset), tm.arr(tm.I64, first), tm.arr(tm.I64, nrows), tm.val(step), tm.val(tm.K),
                                             tm.val(1.3), tm.val(0.0 if dispersion is None else dispersion), tm.val(1e-9), tm.val(17)]
                  + tm.OUT3 + tm.HOST3 + DISP3 + tm.TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_tweedie_workspace_bytes" and fake.ws_calls[0][1][1:] == (4, step)


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
def test_tweedie_pass(fake, icpt, with_offset, want_H, want_w, want_stats):  # noqa: F811
    X, y, offset = tm.rows()
    offset = offset if with_offset else None
    pe = tm.P + int(icpt)
    beta = torch.zeros(pe, dtype=torch.float64)
    res = engine.tweedie_pass(X, y, beta, 1.3, 0.75, offset=offset, fit_intercept=icpt, want_H=want_H, want_w=want_w, want_stats=want_stats)
    r = _check_pass(res, pe, want_H, want_w, want_stats)
    tm.check_call(fake, "dlsa_tweedie_pass_f64",
                  [tm.ptr(X), tm.val(4), tm.ptr(y), tm.ptr(offset), tm.ptr(beta), tm.val(1.3), tm.val(0.75), tm.val(tm.N), tm.val(tm.P),
                   tm.val(int(icpt)), tm.out("H"), tm.val(pe), tm.out("g"), tm.out("ll"), tm.out("w"), tm.out("st")] + tm.TAIL, r)
    assert fake.ws_calls == [("dlsa_tweedie_workspace_bytes", (tm.N, tm.P, int(icpt), 1))]


@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w,want_stats", [(True, False, False), (False, True, False), (False, False, True)])
def test_onehot_tweedie_pass(fake, with_offset, want_H, want_w, want_stats):  # noqa: F811
    plan, num, codes = tm.raw()
    _, y, offset = tm.rows()
    offset = offset if with_offset else None
    beta = torch.zeros(tm.PLAN_P, dtype=torch.float64)
    res = engine.onehot_tweedie_pass(plan, num, codes, y, beta, 1.3, 0.75, offset=offset, want_H=want_H, want_w=want_w, want_stats=want_stats)
    r = _check_pass(res, tm.PLAN_P, want_H, want_w, want_stats)
    tm.check_call(fake, "dlsa_onehot_tweedie_pass_f64",
                  tm.raw_spec(num, codes) + [tm.ptr(y), tm.ptr(offset), tm.ptr(beta), tm.val(1.3), tm.val(0.75), tm.val(tm.N), tm.out("H"),
                                             tm.val(tm.PLAN_P), tm.out("g"), tm.out("ll"), tm.out("w"), tm.out("st")] + tm.TAIL, r)


def test_pass_defaults_and_the_required_power(fake):  # noqa: F811
    X, y, _ = tm.rows()
    beta = torch.zeros(tm.P, dtype=torch.float64)
    H, g, ll, w, st = engine.tweedie_pass(X, y, beta, 1.7)
    assert H is not None and w is None and st is None and fake.calls[0][1][5:7] == (1.7, 1.0)
    with pytest.raises(TypeError):
        engine.tweedie_pass(X, y, beta)                       # power is a required positional argument
    plan, num, codes = tm.raw()
    with pytest.raises(TypeError):
        engine.onehot_tweedie_pass(plan, num, codes, y, torch.zeros(tm.PLAN_P, dtype=torch.float64))
    engine.tweedie_fit_ex(X, y, *tm.PARTS[1])                  # the fits' default power is 1.5
    assert fake.calls[1][0] == "dlsa_tweedie_fit_f64" and fake.calls[1][1][10:12] == (1.5, 0.0)


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it is on the GPU: lets the models' own checks pass in front of the fake library"""
    is_cuda = property(lambda self: True)


def _on_device(t):
    return None if t is None else torch.Tensor._make_subclass(_OnDevice, t)


@pytest.mark.parametrize("dispersion", [None, 0.75])
@pytest.mark.parametrize("with_exposure", [False, True])
def test_fit_tweedie_partitions_marshals(fake, dispersion, with_exposure):  # noqa: F811
    X, y, _ = tm.rows()
    assert bool((y == 0).any()) and bool((y > 0).any())      # (rows() draws counts 0 .. 2: zeros are data here)
    X, y = _on_device(X), _on_device(y)
    e = torch.linspace(0.5, 2.0, tm.N, dtype=torch.float64) if with_exposure else None
    mb = models.fit_tweedie_partitions(X, y, partition_num=2, fit_intercept=True, exposure=e, power=1.3, dispersion=dispersion, tol=1e-9,
                                       max_iter=17)
    name, a = fake.calls[0]
    first, nrows = tm.PARTS[2]
    assert name == "dlsa_tweedie_fit_f64" and len(fake.calls) == 1 and len(a) == len(_lib.SIGNATURES[name][1])
    assert tm.addr(a[0]) == X.data_ptr() and a[1] == 4 and tm.addr(a[2]) == y.data_ptr()
    if with_exposure:                                        # the offset the kernel reads is a tensor of its own: log(exposure)
        assert tm.addr(a[3]) not in (0, e.data_ptr())
    else:
        assert tm.addr(a[3]) == 0
    assert list(a[4]) == first and list(a[5]) == nrows and a[6:14] == (2, 2, tm.P, 1, 1.3, 0.0 if dispersion is None else dispersion, 1e-9, 17)
    assert mb.names == ["intercept", "x0", "x1", "x2"] and mb.sample_size == tm.N
    assert list(mb.extra) == ["dispersion", "pearson", "deviance", "df"] and mb.extra["df"] == [m - 4 for m in nrows]
    # every host list came from its own output array (the fake writes 100 * position + k)
    for key, pos in (("dispersion", 20), ("pearson", 21), ("deviance", 22)):
        assert mb.extra[key] == [100.0 * pos, 100.0 * pos + 1]
    assert mb.loglik == [1900.0, 1901.0] and mb.status == [1800, 1801]


@pytest.mark.parametrize("structured", [True, False])
def test_fit_tweedie_design_marshals(fake, structured):  # noqa: F811
    plan, num, codes = tm.raw()
    _, y, offset = tm.rows()
    y = _on_device(y)
    Xbuilt = torch.rand((tm.N, tm.PLAN_P), dtype=torch.float64)
    spec = types.SimpleNamespace(onehot_plan=lambda: plan, names=["c%d" % i for i in range(tm.PLAN_P)], build=lambda n, c: (Xbuilt, None))
    mb = models.fit_tweedie_design(num, codes, y, spec, part_offsets=tm.OFFS, offset=offset, power=1.3, dispersion=0.75, structured=structured,
                                   tol=1e-9, max_iter=17)
    name, a = fake.calls[0]
    first, nrows = tm.PARTS[1]
    if structured:
        assert name == "dlsa_onehot_tweedie_fit_f64"
        assert tm.addr(a[0]) == tm.PLAN_H and tm.addr(a[1]) == num.data_ptr() and tm.addr(a[3]) == codes.data_ptr()
        assert tm.addr(a[5]) == y.data_ptr() and tm.addr(a[6]) == offset.data_ptr()
        assert list(a[7]) == first and list(a[8]) == nrows and a[9:15] == (1, 2, 1.3, 0.75, 1e-9, 17)
    else:                                                     # the dense fit on the built matrix, no implicit intercept
        assert name == "dlsa_tweedie_fit_f64"
        assert tm.addr(a[0]) == Xbuilt.data_ptr() and tm.addr(a[2]) == y.data_ptr() and tm.addr(a[3]) == offset.data_ptr()
        assert list(a[4]) == first and list(a[5]) == nrows and a[6:14] == (1, 2, tm.PLAN_P, 0, 1.3, 0.75, 1e-9, 17)
    assert mb.names == spec.names and mb.extra["df"] == [m - tm.PLAN_P for m in nrows]


# ---- the Python-side refusals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [1.0, 2.0, 0.5, 2.5, float("nan"), float("inf")])
def test_a_power_outside_the_family_is_refused(fake, power):  # noqa: F811
    X, y, _ = tm.rows()
    X, y = _on_device(X), _on_device(y)
    plan, num, codes = tm.raw()
    spec = types.SimpleNamespace(onehot_plan=lambda: plan, names=[])
    beta = torch.zeros(tm.P, dtype=torch.float64)
    msg = "power must lie strictly between 1 and 2"
    with pytest.raises(ValueError, match="^fit_tweedie_partitions: " + msg):
        models.fit_tweedie_partitions(X, y, power=power)
    with pytest.raises(ValueError, match="^fit_tweedie_design: " + msg):
        models.fit_tweedie_design(num, codes, y, spec, power=power)
    with pytest.raises(ValueError, match="^tweedie_fit_ex: " + msg):
        engine.tweedie_fit_ex(X, y, *tm.PARTS[1], power=power)
    with pytest.raises(ValueError, match="^onehot_tweedie_fit_ex: " + msg):
        engine.onehot_tweedie_fit_ex(plan, num, codes, y, *tm.PARTS[1], power=power)
    with pytest.raises(ValueError, match="^tweedie_pass: " + msg):
        engine.tweedie_pass(X, y, beta, power)
    with pytest.raises(ValueError, match="^onehot_tweedie_pass: " + msg):
        engine.onehot_tweedie_pass(plan, num, codes, y, torch.zeros(tm.PLAN_P, dtype=torch.float64), power)
    with pytest.raises(ValueError, match="^simulate_tweedie: " + msg):
        models.simulate_tweedie(10, 2, 1, power, 1.0)
    assert fake.calls == []


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_a_negative_or_non_finite_response_is_refused(fake, bad):  # noqa: F811
    X, y, _ = tm.rows()
    y = y.clone()
    y[3] = bad
    with pytest.raises(ValueError, match="fit_tweedie_partitions: the response must be non-negative and finite"):
        models.fit_tweedie_partitions(_on_device(X), _on_device(y), fit_intercept=True)
    plan, num, codes = tm.raw()
    spec = types.SimpleNamespace(onehot_plan=lambda: plan, names=[])
    with pytest.raises(ValueError, match="fit_tweedie_design: the response must be non-negative and finite"):
        models.fit_tweedie_design(num, codes, _on_device(y), spec)
    assert fake.calls == []


def test_all_zero_responses_are_refused_and_zeros_are_not(fake):  # noqa: F811
    X, y, _ = tm.rows()
    plan, num, codes = tm.raw()
    spec = types.SimpleNamespace(onehot_plan=lambda: plan, names=[])
    with pytest.raises(ValueError, match="fit_tweedie_partitions: no response is positive"):
        models.fit_tweedie_partitions(_on_device(X), _on_device(torch.zeros_like(y)), fit_intercept=True)
    with pytest.raises(ValueError, match="fit_tweedie_design: no response is positive"):
        models.fit_tweedie_design(num, codes, _on_device(torch.zeros_like(y)), spec)
    assert fake.calls == []
    one = torch.zeros_like(y)
    one[2] = 0.5
    models.fit_tweedie_partitions(_on_device(X), _on_device(one), fit_intercept=True)
    assert [c[0] for c in fake.calls] == ["dlsa_tweedie_fit_f64"]


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan"), float("inf")])
def test_a_dispersion_that_is_not_positive_is_refused(fake, bad):  # noqa: F811
    X, y, _ = tm.rows()
    X, y = _on_device(X), _on_device(y)
    plan, num, codes = tm.raw()
    beta = torch.zeros(tm.P, dtype=torch.float64)
    with pytest.raises(ValueError, match="dispersion must be positive"):
        models.fit_tweedie_partitions(X, y, dispersion=bad)
    with pytest.raises(ValueError, match="dispersion must be positive"):
        models.fit_tweedie_design(num, codes, y, types.SimpleNamespace(onehot_plan=lambda: plan, names=[]), dispersion=bad)
    with pytest.raises(ValueError, match="^tweedie_fit_ex: dispersion must be positive"):
        engine.tweedie_fit_ex(X, y, *tm.PARTS[1], dispersion=bad)
    with pytest.raises(ValueError, match="^onehot_tweedie_fit_ex: dispersion must be positive"):
        engine.onehot_tweedie_fit_ex(plan, num, codes, y, *tm.PARTS[1], dispersion=bad)
    with pytest.raises(ValueError, match="^tweedie_pass: dispersion must be positive"):
        engine.tweedie_pass(X, y, beta, 1.5, bad)
    with pytest.raises(ValueError, match="^onehot_tweedie_pass: dispersion must be positive"):
        engine.onehot_tweedie_pass(plan, num, codes, y, torch.zeros(tm.PLAN_P, dtype=torch.float64), 1.5, bad)
    assert fake.calls == []


def test_offset_and_exposure_together_are_refused(fake):  # noqa: F811
    X, y, offset = tm.rows()
    with pytest.raises(ValueError, match="an offset or an exposure, not both"):
        models.fit_tweedie_partitions(_on_device(X), _on_device(y), offset=offset, exposure=torch.exp(offset))
    with pytest.raises(ValueError, match="exposure must be positive"):
        models.fit_tweedie_partitions(_on_device(X), _on_device(y), exposure=offset - 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        models.fit_tweedie_partitions(X, y)
    assert fake.calls == []


def test_the_c_abi_refuses_before_any_hip_call():
    """argument validation of the new entries happens before any HIP call, so it runs without a GPU"""
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    i64 = ctypes.c_int64
    assert lib.dlsa_tweedie_workspace_bytes(1000, 0, 0, 1) == 0 and lib.dlsa_tweedie_workspace_bytes(1000, 5, 1, 0) == 0
    assert lib.dlsa_tweedie_workspace_bytes(1000, 2048, 1, 1) == 0
    assert lib.dlsa_tweedie_workspace_bytes(1000, 5, 1, 2) > lib.dlsa_tweedie_workspace_bytes(1000, 5, 1, 1) > 0
    assert lib.dlsa_onehot_tweedie_workspace_bytes(None, 10, 1) == 0

    def run(power, disp, ws_bytes=1 << 30, X=one):
        return lib.dlsa_tweedie_pass_f64(X, 4, one, None, one, power, disp, 10, 4, 1, None, 0, None, None, None, None, one, ws_bytes, None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert run(1.5, bad) == 1 and "dispersion" in _lib.last_error()
    for bad in (1.0, 2.0, 0.5, 2.5, float("nan"), float("inf")):
        assert run(bad, 1.0) == 1 and "power" in _lib.last_error()
    assert run(1.5, 1.0, X=None) == 1 and "null" in _lib.last_error()
    assert run(1.5, 1.0, ws_bytes=16) == 3
    first, rows = (i64 * 2)(0, 5), (i64 * 2)(5, 5)
    fit = lambda power, disp, ws_bytes=16: lib.dlsa_tweedie_fit_f64(one, 4, one, None, first, rows, 1, 2, 4, 1, power, disp, 1e-13, 100, one,  # noqa: E731
                                                                    one, one, None, None, None, None, None, None, one, ws_bytes, None)
    assert fit(1.5, float("inf")) == 1 and "finite" in _lib.last_error()
    for bad in (1.0, 2.0, float("nan")):
        assert fit(bad, 0.0) == 1 and "power" in _lib.last_error()
    assert fit(1.5, 0.0) == 3 and fit(1.01, 0.5) == 3 and fit(1.99, 0.5) == 3      # a valid call stops at the workspace check
    assert lib.dlsa_onehot_tweedie_fit_f64(None, None, 0, None, 0, one, None, first, rows, 1, 2, 1.5, 0.0, 1e-13, 100, one, one, one, None,
                                           None, None, None, None, None, one, 16, None) == 1


# ---- simulate_tweedie ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power,dispersion", [(1.2, 2.0), (1.5, 0.8), (1.8, 0.3)])
def test_compound_draws_zero_share_and_mean(power, dispersion):
    """models._tweedie_draw (what simulate_tweedie draws with) at a constant mu: the share of zeros is e^-lambda with lambda =
    mu^(2 - xi) / (phi (2 - xi)), the mean mu, the variance phi mu^xi; 200000 draws, bounds at five standard errors"""
    n, mu = 200_000, 1.7
    y = models._tweedie_draw(np.random.default_rng(11), np.full(n, mu), power, dispersion)
    lam = mu ** (2 - power) / (dispersion * (2 - power))
    p0 = math.exp(-lam)
    var = dispersion * mu ** power
    assert np.all(y >= 0) and abs((y == 0).mean() - p0) <= 5 * math.sqrt(p0 * (1 - p0) / n) + 1e-12
    assert abs(y.mean() - mu) <= 5 * math.sqrt(var / n)
    # Var(s^2) = (kappa_4 + 2 var^2) / n with kappa_4 = xi (2 xi - 1) phi^3 mu^(3 xi - 2)
    k4 = power * (2 * power - 1) * dispersion ** 3 * mu ** (3 * power - 2)
    assert abs(y.var() - var) <= 5 * math.sqrt((k4 + 2 * var * var) / n)
    # the reference's own draws are the same construction
    assert np.array_equal(y, tr.draw(np.random.default_rng(11), np.full(n, mu), power, dispersion))


def test_simulate_tweedie_frame(monkeypatch):
    """simulate_tweedie's frame, with the seeded rows of engine.synth replaced by numpy ones (no GPU here)"""
    def synth(seed, first, n, p, labels=False):
        return torch.from_numpy(np.random.default_rng(seed).uniform(-0.5, 0.5, (n, p))), None
    monkeypatch.setattr(engine, "synth", synth)
    df = models.simulate_tweedie(20_000, 5, 4, 1.5, 0.8, seed=3, exposure=True)
    assert list(df.columns) == ["partition_id", "y", "exposure"] + ["x%d" % i for i in range(5)] and len(df) == 20_000
    assert sorted(df["partition_id"].unique()) == [0.0, 1.0, 2.0, 3.0]
    X, e, y = df[["x%d" % i for i in range(5)]].to_numpy(), df["exposure"].to_numpy(), df["y"].to_numpy()
    mu = e * np.exp(X @ np.array([0.5, 0.5, 0.0, 0.0, 0.0]))
    lam = np.sqrt(mu) / (0.8 * 0.5)
    p0 = np.exp(-lam)
    assert np.all(y >= 0)
    assert abs((y == 0).mean() - p0.mean()) <= 5 * math.sqrt((p0 * (1 - p0)).sum()) / len(y)
    assert abs((y - mu).mean()) <= 5 * math.sqrt((0.8 * mu ** 1.5).sum()) / len(y)
    with pytest.raises(ValueError, match="dispersion must be positive"):
        models.simulate_tweedie(10, 2, 1, 1.5, 0.0)
