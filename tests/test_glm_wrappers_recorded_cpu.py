"""CPU: the sixteen log-link engine wrappers ({,onehot_}{poisson,negbin,gamma,tweedie}_{pass,fit_ex}) and the fit_*_partitions /
fit_*_design entries of models.py, recorded call by call in front of the recording fake library of test_engine_marshal_cpu.py and
compared with tests/golden/glm_wrapper_calls.json.  records() walks a fixed grid of good calls -- the symbol, the workspace query,
every scalar, the role of the tensor behind every pointer, the partition arrays, the result -- and a fixed list of bad calls -- the
exception's type and text, pairs of wrong arguments included -- and notes the signatures of the public functions.

The golden file is the output of this file's records() on the commit BEFORE the wrappers became one body per job (run there with
DLSA_GLM_RECORD=<path to write>): the wrappers of this tree must hand the C ABI, return and refuse exactly what those did."""
import ctypes
import inspect
import json
import os
import types

import numpy as np
import torch

import test_engine_marshal_cpu as tm
from dlsa_amd import engine, models
from test_engine_marshal_cpu import fake  # noqa: F401  (the recording fake library, a fixture)
from test_tweedie_cpu import _on_device

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glm_wrapper_calls.json")
FAMILIES = ("poisson", "negbin", "gamma", "tweedie")
PASS_SCALARS = {"poisson": (), "negbin": (0.75,), "gamma": (0.6,), "tweedie": (1.3, 0.6)}           # positional, after beta
FIT_SCALARS = {"poisson": {}, "negbin": {"alpha": 0.75}, "gamma": {"dispersion": 0.6}, "tweedie": {"power": 1.3, "dispersion": 0.6}}
WANT_EXTRA = {"poisson": None, "negbin": "want_theta", "gamma": "want_stats", "tweedie": "want_stats"}
PASS_OUT = {"poisson": ["H", "g", "ll", "w"], "negbin": ["H", "g", "ll", "w", "mu", "theta_terms"],
            "gamma": ["H", "g", "ll", "w", "stats"], "tweedie": ["H", "g", "ll", "w", "stats"]}
WANTS = [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]          # want_H, want_w, the family's own


def _plain(v):
    """a result as JSON: tensors as "<dtype>[shape]", dicts as [key, value] pairs in their order, MappedBlocks by their fields"""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if torch.is_tensor(v):
        return "%s%s" % (v.dtype, list(v.shape))
    if isinstance(v, dict):
        return {"dict": [[k, _plain(x)] for k, x in v.items()]}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, models.MappedBlocks):
        return {"blocks": [[k, _plain(getattr(v, k))] for k in ("coef", "Sig_invMcoef", "Sig_inv", "names", "status", "n_iter", "loglik",
                                                                  "num_partitions", "sample_size", "extra")]}
    raise TypeError(type(v))


def _roles_of(res, names):
    """data_ptr -> "out:<name>" of the tensors of a result (a pass's tuple, a fit's dict, a MappedBlocks)"""
    if isinstance(res, tuple):
        items = zip(names, res)
    elif isinstance(res, dict):
        items = res.items()
    else:
        items = ((k, getattr(res, k)) for k in ("coef", "Sig_invMcoef", "Sig_inv"))
    return {t.data_ptr(): "out:" + k for k, t in items if torch.is_tensor(t)}


def _arg(a, roles):
    """one argument of a C call: a pointer as "@<the role of the tensor it addresses>" ("@own": a tensor the wrapper made itself; None:
    null), a partition array by its values, a host output array as "<ctype>*<length>", a scalar as it is (1 and 1.0 differ)"""
    if isinstance(a, ctypes.c_void_p):
        return None if not a.value else "@" + roles.get(a.value, "own")
    if isinstance(a, ctypes.Array):
        return {"i64": list(a)} if a._type_ is ctypes.c_int64 else "%s*%d" % (a._type_.__name__, len(a))
    assert type(a) in (int, float), type(a)
    return a


def record(lib, label, call, tensors, out_names=()):
    """one good call: every C call and workspace query it made, and what it returned"""
    lib.calls.clear(); lib.ws_calls.clear(); lib.ws.clear()
    res = call()
    roles = {t.data_ptr(): k for k, t in tensors.items() if t is not None}
    roles.update(_roles_of(res, out_names))
    roles.update({w.data_ptr(): "ws" for w in lib.ws})
    roles.update({tm.PLAN_H: "plan", tm.STREAM: "stream"})
    return {"call": label, "c": [[name, [_arg(a, roles) for a in args]] for name, args in lib.calls],
            "ws": [[name, [_arg(a, roles) for a in args]] for name, args in lib.ws_calls], "result": _plain(res)}


def refusal(lib, label, call):
    """one bad call: the exception's type and text (None where the family takes the call), and how many C calls were made"""
    lib.calls.clear(); lib.ws_calls.clear(); lib.ws.clear()
    raised = text = None
    try:
        call()
    except Exception as e:      # noqa: BLE001  (whatever it raises is what is recorded)
        raised, text = type(e).__name__, str(e)
    return {"call": label, "raises": raised, "text": text, "c_calls": len(lib.calls)}


def _spec(plan, Xbuilt):
    return types.SimpleNamespace(onehot_plan=lambda: plan, names=["c%d" % i for i in range(tm.PLAN_P)], build=lambda n, c: (Xbuilt, None))


def good_calls(lib):
    out = []
    X, y, offset = tm.rows()
    plan, num, codes = tm.raw()
    dense = {"X": X, "y": y, "offset": offset}
    rawt = {"num": num, "codes": codes, "y": y, "offset": offset}
    for fam in FAMILIES:
        sc, kw, extra = PASS_SCALARS[fam], FIT_SCALARS[fam], WANT_EXTRA[fam]
        f_pass, f_fit = getattr(engine, fam + "_pass"), getattr(engine, fam + "_fit_ex")
        o_pass, o_fit = getattr(engine, "onehot_%s_pass" % fam), getattr(engine, "onehot_%s_fit_ex" % fam)
        for want_H, want_w, want_x in WANTS:
            if extra is None and want_x and not (want_H and want_w):
                continue
            want = {"want_H": want_H, "want_w": want_w, **({extra: want_x} if extra else {})}
            first_wants = (want_H, want_w, want_x) == WANTS[0]          # offset x intercept crossed once, the flags one by one
            for with_offset in (False, True) if first_wants else (True,):
                o = offset if with_offset else None
                for icpt in (False, True) if first_wants else (True,):
                    beta = torch.zeros(tm.P + int(icpt), dtype=torch.float64)
                    out.append(record(lib, "%s_pass icpt=%d offset=%d %s" % (fam, icpt, with_offset, sorted(want.items())),
                                      lambda: f_pass(X, y, beta, *sc, offset=o, fit_intercept=icpt, **want), {**dense, "beta": beta},
                                      PASS_OUT[fam]))
                beta = torch.zeros(tm.PLAN_P, dtype=torch.float64)
                out.append(record(lib, "onehot_%s_pass offset=%d %s" % (fam, with_offset, sorted(want.items())),
                                  lambda: o_pass(plan, num, codes, y, beta, *sc, offset=o, **want), {**rawt, "beta": beta}, PASS_OUT[fam]))
        # the defaults: everything optional left out (NB2's alpha and Tweedie's power are required in a pass)
        required = {"poisson": (), "negbin": (0.75,), "gamma": (), "tweedie": (1.3,)}[fam]
        beta, betap = torch.zeros(tm.P, dtype=torch.float64), torch.zeros(tm.PLAN_P, dtype=torch.float64)
        out.append(record(lib, fam + "_pass defaults", lambda: f_pass(X, y, beta, *required), {**dense, "beta": beta}, PASS_OUT[fam]))
        out.append(record(lib, "onehot_%s_pass defaults" % fam, lambda: o_pass(plan, None, codes, y, betap, *required),
                          {**rawt, "beta": betap}, PASS_OUT[fam]))
        out.append(record(lib, fam + "_fit_ex defaults", lambda: f_fit(X, y, *tm.PARTS[1]), dense))
        out.append(record(lib, "onehot_%s_fit_ex defaults" % fam, lambda: o_fit(plan, None, codes, y, *tm.PARTS[1]), rawt))
        for step in (1, 2):
            first, nrows = tm.PARTS[step]
            for with_offset in (False, True):
                o = offset if with_offset else None
                for icpt in (False, True):
                    out.append(record(lib, "%s_fit_ex step=%d icpt=%d offset=%d" % (fam, step, icpt, with_offset),
                                      lambda: f_fit(X, y, first, nrows, row_step=step, offset=o, fit_intercept=icpt, tol=1e-9, max_iter=17, **kw),
                                      dense))
                out.append(record(lib, "onehot_%s_fit_ex step=%d offset=%d" % (fam, step, with_offset),
                                  lambda: o_fit(plan, num, codes, y, first, nrows, row_step=step, offset=o, tol=1e-9, max_iter=17, **kw), rawt))
        # a soft failure code comes back in the dict, `rc` and `df` where they were
        lib.rc = 5
        out.append(record(lib, fam + "_fit_ex rc=5", lambda: f_fit(X, y, *tm.PARTS[1], **kw), dense))
        out.append(record(lib, "onehot_%s_fit_ex rc=5" % fam, lambda: o_fit(plan, num, codes, y, *tm.PARTS[1], **kw), rawt))
        lib.rc = 0
        # models.py, in front of the same library
        Xd, yd = _on_device(X), _on_device(y)
        Xbuilt = torch.rand((tm.N, tm.PLAN_P), dtype=torch.float64)
        spec = _spec(plan, Xbuilt)
        fp, fd = getattr(models, "fit_%s_partitions" % fam), getattr(models, "fit_%s_design" % fam)
        e = torch.linspace(0.5, 2.0, tm.N, dtype=torch.float64)
        y1 = y.clone()
        y1[y1 == 0] = 0.5 if fam in ("gamma",) else 0.0              # (the Gamma family refuses a zero response)
        y1d = _on_device(y1)
        mt = {"X": X, "y": y1, "offset": offset, "exposure": e, "num": num, "codes": codes, "Xbuilt": Xbuilt}
        out.append(record(lib, "fit_%s_partitions defaults" % fam, lambda: fp(Xd, y1d), mt))
        out.append(record(lib, "fit_%s_partitions i%%2 icpt exposure" % fam,
                          lambda: fp(Xd, y1d, partition_num=2, fit_intercept=True, exposure=e, names=["a", "b", "c"], tol=1e-9, max_iter=17, **kw),
                          mt))
        out.append(record(lib, "fit_%s_partitions offsets offset" % fam, lambda: fp(Xd, y1d, part_offsets=tm.OFFS, offset=offset, **kw), mt))
        for structured in (True, False):
            out.append(record(lib, "fit_%s_design structured=%d defaults" % (fam, structured),
                              lambda: fd(num, codes, y1d, spec, structured=structured), mt))
            out.append(record(lib, "fit_%s_design structured=%d offsets offset" % (fam, structured),
                              lambda: fd(num, codes, y1d, spec, part_offsets=tm.OFFS, offset=offset, structured=structured, tol=1e-9,
                                         max_iter=17, **kw), mt))
            out.append(record(lib, "fit_%s_design structured=%d i%%2 exposure" % (fam, structured),
                              lambda: fd(num, codes, y1d, spec, partition_num=2, exposure=e, structured=structured, **kw), mt))
        assert Xd.data_ptr() == X.data_ptr() and yd.data_ptr() == y.data_ptr()
    return out


BAD = (0.0, -0.5, float("inf"), float("nan"))


def bad_calls(lib):
    out = []
    X, y, offset = tm.rows()
    plan, num, codes = tm.raw()
    f32 = torch.float32
    b, bp = torch.zeros(tm.P, dtype=torch.float64), torch.zeros(tm.PLAN_P, dtype=torch.float64)
    wide = torch.zeros(tm.PLAN_P + 1, dtype=torch.float64)
    first, nrows = tm.PARTS[1]
    Xd, yd = _on_device(X), _on_device(y)
    spec = _spec(plan, None)
    for fam in FAMILIES:
        sc, kw = PASS_SCALARS[fam], FIT_SCALARS[fam]
        f_pass, f_fit = getattr(engine, fam + "_pass"), getattr(engine, fam + "_fit_ex")
        o_pass, o_fit = getattr(engine, "onehot_%s_pass" % fam), getattr(engine, "onehot_%s_fit_ex" % fam)
        fp, fd = getattr(models, "fit_%s_partitions" % fam), getattr(models, "fit_%s_design" % fam)

        def add(label, call):
            out.append(refusal(lib, "%s: %s" % (fam, label), call))
        # ---- each validator's refusals, at every entry that has the scalar
        for i, name in enumerate(kw):
            for bad in BAD + ((1.0, 2.0) if name == "power" else ()):
                swapped = tuple(bad if j == i else v for j, v in enumerate(sc))
                kws = {**kw, name: bad}
                add("pass %s=%r" % (name, bad), lambda: f_pass(X, y, b, *swapped))
                add("onehot pass %s=%r" % (name, bad), lambda: o_pass(plan, num, codes, y, bp, *swapped))
                add("fit %s=%r" % (name, bad), lambda: f_fit(X, y, first, nrows, **kws))
                add("onehot fit %s=%r" % (name, bad), lambda: o_fit(plan, num, codes, y, first, nrows, **kws))
                add("partitions %s=%r" % (name, bad), lambda: fp(Xd, yd, **kws))
                add("design %s=%r" % (name, bad), lambda: fd(num, codes, yd, spec, **kws))
        # ---- device, dtype and row counts
        add("pass X fp32", lambda: f_pass(X.to(f32), y, b, *sc))
        add("pass y fp32", lambda: f_pass(X, y.to(f32), b, *sc))
        add("pass beta fp32", lambda: f_pass(X, y, b.to(f32), *sc))
        add("pass offset fp32", lambda: f_pass(X, y, b, *sc, offset=offset.to(f32)))
        add("pass y short", lambda: f_pass(X, y[:5], b, *sc))
        add("pass offset short", lambda: f_pass(X, y, b, *sc, offset=offset[:5]))
        add("pass beta wide", lambda: f_pass(X, y, wide, *sc))
        add("pass no rows", lambda: f_pass(X[:0], y[:0], b, *sc))
        add("pass X column-major", lambda: f_pass(X.t().contiguous().t(), y, b, *sc))
        add("fit X fp32", lambda: f_fit(X.to(f32), y, first, nrows, **kw))
        add("fit y short", lambda: f_fit(X, y[:5], first, nrows, **kw))
        add("fit offset short", lambda: f_fit(X, y, first, nrows, offset=offset[:5], **kw))
        add("fit offset fp32", lambda: f_fit(X, y, first, nrows, offset=offset.to(f32), **kw))
        add("onehot pass beta fp32", lambda: o_pass(plan, num, codes, y, bp.to(f32), *sc))
        add("onehot pass y fp32", lambda: o_pass(plan, num, codes, y.to(f32), bp, *sc))
        add("onehot pass offset short", lambda: o_pass(plan, num, codes, y, bp, *sc, offset=offset[:5]))
        add("onehot pass num short", lambda: o_pass(plan, num[:5], codes, y, bp, *sc))
        add("onehot pass codes short", lambda: o_pass(plan, num, codes[:5], y, bp, *sc))
        add("onehot pass beta wide", lambda: o_pass(plan, num, codes, y, wide, *sc))
        add("onehot pass no rows", lambda: o_pass(plan, num[:0], codes[:0], y[:0], bp, *sc))
        add("onehot pass num fp32", lambda: o_pass(plan, num.to(f32), codes, y, bp, *sc))
        add("onehot pass codes int64", lambda: o_pass(plan, num, codes.to(torch.int64), y, bp, *sc))
        add("onehot fit offset short", lambda: o_fit(plan, num, codes, y, first, nrows, offset=offset[:5], **kw))
        add("onehot fit num short", lambda: o_fit(plan, num[:5], codes, y, first, nrows, **kw))
        add("onehot fit codes short", lambda: o_fit(plan, num, codes[:5], y, first, nrows, **kw))
        add("onehot fit num fp32", lambda: o_fit(plan, num.to(f32), codes, y, first, nrows, **kw))
        # ---- the partitions
        for case in ("K = 0", "unequal lengths", "step 0", "past n", "past n, strided"):
            pf, pr, st = tm.BAD_PARTS[case]
            add("fit partitions %s" % case, lambda: f_fit(X, y, pf, pr, row_step=st, **kw))
            add("onehot fit partitions %s" % case, lambda: o_fit(plan, num, codes, y, pf, pr, row_step=st, **kw))
        # ---- a hard failure of the library
        lib.rc = 1
        add("pass rc=1", lambda: f_pass(X, y, b, *sc))
        add("onehot pass rc=1", lambda: o_pass(plan, num, codes, y, bp, *sc))
        add("fit rc=1", lambda: f_fit(X, y, first, nrows, **kw))
        add("onehot fit rc=1", lambda: o_fit(plan, num, codes, y, first, nrows, **kw))
        lib.rc = 0
        # ---- two wrong arguments at once: which error wins
        badsc = tuple(BAD[1] for _ in sc)
        badkw = {k: BAD[1] for k in kw}
        add("pass: X fp32 + y short", lambda: f_pass(X.to(f32), y[:5], b, *sc))
        add("pass: offset fp32 + beta wide", lambda: f_pass(X, y, wide, *sc, offset=offset.to(f32)))
        add("pass: beta wide + scalars", lambda: f_pass(X, y, wide, *badsc))
        add("pass: y short + scalars", lambda: f_pass(X, y[:5], b, *badsc))
        add("pass: all scalars", lambda: f_pass(X, y, b, *badsc))
        add("onehot pass: beta fp32 + offset short", lambda: o_pass(plan, num, codes, y, bp.to(f32), *sc, offset=offset[:5]))
        add("onehot pass: y fp32 + num short", lambda: o_pass(plan, num[:5], codes, y.to(f32), bp, *sc))
        add("onehot pass: offset short + beta wide", lambda: o_pass(plan, num, codes, y, wide, *sc, offset=offset[:5]))
        add("onehot pass: beta wide + scalars", lambda: o_pass(plan, num, codes, y, wide, *badsc))
        add("onehot pass: scalars + num fp32", lambda: o_pass(plan, num.to(f32), codes, y, bp, *badsc))
        add("onehot pass: all scalars", lambda: o_pass(plan, num, codes, y, bp, *badsc))
        add("fit: y fp32 + y short", lambda: f_fit(X, y[:5].to(f32), first, nrows, **kw))
        add("fit: y short + scalars", lambda: f_fit(X, y[:5], first, nrows, **badkw))
        add("fit: y short + partitions", lambda: f_fit(X, y[:5], [], [], 0, **kw))
        add("fit: scalars + partitions", lambda: f_fit(X, y, [], [], 0, **badkw))
        add("onehot fit: num short + scalars", lambda: o_fit(plan, num[:5], codes, y, first, nrows, **badkw))
        add("onehot fit: offset short + partitions", lambda: o_fit(plan, num, codes, y, [], [], 0, offset=offset[:5], **kw))
        add("onehot fit: scalars + partitions", lambda: o_fit(plan, num, codes, y, [], [], 0, **badkw))
        add("onehot fit: partitions + num fp32", lambda: o_fit(plan, num.to(f32), codes, y, [], [], 0, **kw))
        # ---- models.py
        neg = y.clone()
        neg[3] = -1.0
        zero = torch.zeros_like(y)
        add("partitions on the CPU", lambda: fp(X, y, **kw))
        add("partitions on the CPU + scalars", lambda: fp(X, y, **badkw))
        add("partitions X fp32", lambda: fp(_on_device(X.to(f32)), yd, **kw))
        add("partitions X fp32 + scalars", lambda: fp(_on_device(X.to(f32)), yd, **badkw))
        add("design on the CPU", lambda: fd(num, codes, y, spec, **kw))
        add("design y no tensor", lambda: fd(num, codes, [0.0] * tm.N, spec, **kw))
        add("design num fp32", lambda: fd(num.to(f32), codes, yd, spec, **kw))
        add("design num fp32 + scalars", lambda: fd(num.to(f32), codes, yd, spec, **badkw))
        add("partitions y short", lambda: fp(Xd, _on_device(y[:5]), **kw))
        add("partitions scalars + y short", lambda: fp(Xd, _on_device(y[:5]), **badkw))
        add("partitions first scalar zero + y short", lambda: fp(Xd, _on_device(y[:5]), **{**kw, **{k: 0.0 for k in list(kw)[:1]}}))
        add("partitions all scalars", lambda: fp(Xd, yd, **badkw))
        add("design all scalars", lambda: fd(num, codes, yd, spec, **badkw))
        add("partitions negative response", lambda: fp(Xd, _on_device(neg), **kw))
        add("design negative response", lambda: fd(num, codes, _on_device(neg), spec, **kw))
        add("partitions zero response", lambda: fp(Xd, _on_device(zero), **kw))
        add("design zero response", lambda: fd(num, codes, _on_device(zero), spec, **kw))
        add("partitions nan response", lambda: fp(Xd, _on_device(torch.full_like(y, float("nan"))), **kw))
        add("partitions scalars + negative response", lambda: fp(Xd, _on_device(neg), **badkw))
        add("partitions y short + negative response", lambda: fp(Xd, _on_device(neg[:5]), **kw))
        add("partitions negative response + offset and exposure", lambda: fp(Xd, _on_device(neg), offset=offset, exposure=torch.exp(offset), **kw))
        pos = _on_device(y + 1.0)
        add("partitions offset and exposure", lambda: fp(Xd, pos, offset=offset, exposure=torch.exp(offset), **kw))
        add("design offset and exposure", lambda: fd(num, codes, pos, spec, offset=offset, exposure=torch.exp(offset), **kw))
        add("partitions exposure not positive", lambda: fp(Xd, pos, exposure=offset - 0.5, **kw))
        add("partitions offset short", lambda: fp(Xd, pos, offset=offset[:5], **kw))
        add("design exposure short", lambda: fd(num, codes, pos, spec, exposure=torch.exp(offset[:5]), **kw))
        add("partitions offset and exposure + offset short", lambda: fp(Xd, pos, offset=offset[:5], exposure=torch.exp(offset), **kw))
    return out


def signatures():
    names = ["%s%s_%s" % (pre, fam, job) for fam in FAMILIES for pre in ("", "onehot_") for job in ("pass", "fit_ex")]
    out = {"engine." + n: str(inspect.signature(getattr(engine, n))) for n in names}
    for fam in FAMILIES:
        for n in ("simulate_" + fam, "fit_%s_partitions" % fam, "fit_%s_design" % fam, fam + "_model", fam + "_model_eval"):
            out["models." + n] = str(inspect.signature(getattr(models, n)))
    out.update({"docstrings": sorted(k for k in out if not (getattr(engine if k.startswith("engine.") else models, k.split(".")[1]).__doc__ or "").strip())})
    return out


def simulated(monkeypatch):
    """the four simulators' frames with engine.synth's seeded rows replaced by numpy ones: the columns and the exact sums"""
    def synth(seed, first, n, p, labels=False):
        return torch.from_numpy(np.random.default_rng(seed).uniform(-0.5, 0.5, (n, p))), None
    monkeypatch.setattr(engine, "synth", synth)
    out = []
    for label, call in (("poisson", lambda e: models.simulate_poisson(500, 5, 4, seed=3, base_rate=1.5, exposure=e)),
                        ("negbin", lambda e: models.simulate_negbin(500, 5, 4, 0.7, seed=3, coef_value=0.3, exposure=e)),
                        ("gamma", lambda e: models.simulate_gamma(500, 5, 4, 2.5, seed=3, base_mean=1.5, exposure=e)),
                        ("tweedie", lambda e: models.simulate_tweedie(500, 5, 4, 1.5, 0.8, seed=3, exposure=e))):
        for e in (False, True):
            df = call(e)
            out.append({"call": "simulate_%s exposure=%d" % (label, e), "columns": list(df.columns), "rows": len(df),
                        "sums": [float(df[c].sum()) for c in df.columns]})
    for label, call in (("negbin alpha=0", lambda: models.simulate_negbin(10, 2, 1, 0.0)), ("gamma shape=0", lambda: models.simulate_gamma(10, 2, 1, 0.0)),
                        ("tweedie power=2", lambda: models.simulate_tweedie(10, 2, 1, 2.0, 1.0)),
                        ("tweedie dispersion=0", lambda: models.simulate_tweedie(10, 2, 1, 1.5, 0.0)),
                        ("tweedie power=2 dispersion=0", lambda: models.simulate_tweedie(10, 2, 1, 2.0, 0.0))):
        try:
            call()
            out.append({"call": "simulate " + label, "raises": None})
        except Exception as e:      # noqa: BLE001
            out.append({"call": "simulate " + label, "raises": type(e).__name__, "text": str(e)})
    return out


def records(lib, monkeypatch):
    torch.manual_seed(0)
    return {"signatures": signatures(), "calls": good_calls(lib), "refusals": bad_calls(lib), "simulated": simulated(monkeypatch)}


def _lines(rec):
    """the file's form: one record per line, so that a difference reads as a line"""
    parts = ['"signatures": ' + json.dumps(rec["signatures"], indent=1)]
    parts += ['"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in rec[k])) for k in ("calls", "refusals", "simulated")]
    return "{\n" + ",\n".join(parts) + "\n}\n"


def test_wrappers_hand_over_what_the_recorded_ones_did(fake, monkeypatch):  # noqa: F811
    rec = records(fake, monkeypatch)
    # a refusal comes before any C call (the library's own failure codes apart)
    assert all(r["c_calls"] == (1 if " rc=" in r["call"] else 0) for r in rec["refusals"] if r["raises"] is not None)
    assert rec["signatures"]["docstrings"] == []
    target = os.environ.get("DLSA_GLM_RECORD")
    if target:                                  # (the recording run, on the commit the golden file describes)
        with open(target, "w") as f:
            f.write(_lines(rec))
        return
    rec = json.loads(_lines(rec))               # (NaN and tuples as the file holds them)
    golden = json.load(open(GOLDEN))
    assert rec["signatures"] == golden["signatures"]
    for key in ("calls", "refusals", "simulated"):
        assert [r["call"] for r in rec[key]] == [r["call"] for r in golden[key]], key
        for got, want in zip(rec[key], golden[key]):
            assert repr(got) == repr(want), got["call"]
