"""CPU: the probit / cloglog extension without a GPU -- the extension header include/dlsa_hip_binary.h against _lib.BINARY_SIGNATURES
and the built library (names, return and argument types, the signatures equal to the Poisson ones), the main table untouched, what the
entries refuse before any HIP call, the marshalling of the four engine wrappers and of the model functions against a recording fake
library (tests/test_engine_marshal_cpu.py), the Python-level refusals, and the generator of the kernels' coefficient tables."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

import test_engine_marshal_cpu as tm                        # noqa: E402
from test_engine_marshal_cpu import fake                    # noqa: E402,F401  (the recording library)
from test_gamma_cpu import _on_device                       # noqa: E402
from dlsa_amd import _lib, engine, models                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dlsa_hip_binary.h")
LINKS = ("probit", "cloglog")
ENTRIES = ["dlsa_%s_%s" % (link, e) for link in LINKS for e in ("workspace_bytes", "pass_f64", "fit_f64")]


@pytest.fixture(autouse=True)
def _signatures(monkeypatch):
    """check_call looks the argument count up in _lib.SIGNATURES: for this file that table also holds the extension's entries"""
    monkeypatch.setattr(_lib, "SIGNATURES", {**_lib.SIGNATURES, **_lib.BINARY_SIGNATURES})


# ---- header <-> BINARY_SIGNATURES <-> the library ------------------------------------------------------------------------------------
def _declarations():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"^\s*(size_t|int)\s+(dlsa_\w+)\s*\(([^;]*)\)\s*;", text, re.M)}


def _main_declaration(name):
    with open(os.path.join(ROOT, "include", "dlsa_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"^\s*(size_t|int)\s+%s\s*\(([^;]*)\)\s*;" % name, text, re.M)
    return m.group(1), m.group(2)


def test_header_declares_exactly_the_bound_table():
    decl = _declarations()
    assert sorted(decl) == sorted(_lib.BINARY_SIGNATURES) == sorted(ENTRIES)
    for name, (res, args) in decl.items():
        bound_res, bound_args = _lib.BINARY_SIGNATURES[name]
        assert len(args.split(",")) == len(bound_args), name
        assert bound_res is (_lib.c_sz if res == "size_t" else _lib.c_int), name
        for text, ctype in zip(args.split(","), bound_args):
            text = " ".join(text.split())
            if "_host" in text:
                want = ctypes.POINTER({"int64_t": _lib.c_i64, "int": _lib.c_int, "double": _lib.c_dbl}[text.replace("const ", "").split("*")[0].strip()])
            elif "*" in text:
                want = _lib.c_vp
            else:
                want = {"int64_t": _lib.c_i64, "int": _lib.c_int, "double": _lib.c_dbl, "size_t": _lib.c_sz}[text.split()[0]]
            assert ctype is want or ctype == want, (name, text)
    with open(HEADER) as f:
        assert '#include "dlsa_hip.h"' in f.read()


@pytest.mark.parametrize("name", ENTRIES)
def test_signatures_are_the_poisson_ones_argument_for_argument(name):
    pois = re.sub(r"dlsa_(probit|cloglog)_", "dlsa_poisson_", name)
    assert _lib.BINARY_SIGNATURES[name] == _lib.SIGNATURES[pois]
    res, args = _declarations()[name]
    pres, pargs = _main_declaration(pois)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]       # noqa: E731
    assert res == pres and norm(args) == norm(pargs)                   # the same types AND the same parameter names


def test_the_main_table_is_as_it_was_and_the_tables_are_disjoint(monkeypatch):
    monkeypatch.undo()                                                  # (the autouse merge of this file)
    assert len(_lib.SIGNATURES) == 111
    tables = [_lib.SIGNATURES, _lib.ORDINAL_SIGNATURES, _lib.ONEHOT_ORDINAL_SIGNATURES, _lib.BINARY_SIGNATURES]
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not set(a) & set(b)
    with open(os.path.join(ROOT, "include", "dlsa_hip.h")) as f:
        text = f.read()
    assert "probit" not in text and "cloglog" not in text


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_library_exports_and_binds_the_entries(lib):
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.BINARY_SIGNATURES[name][1] and fn.restype is _lib.BINARY_SIGNATURES[name][0]


# ---- refusals without a GPU: every argument is judged before any HIP call --------------------------------------------------------------
def _pass(lib, link, X=1 << 20, p=5, n=10, ldx=None, icpt=0):
    return getattr(lib, "dlsa_%s_pass_f64" % link)(X, p if ldx is None else ldx, 1 << 20, None, 1 << 20, n, p, icpt, None, 0, None, None, None,
                                                   None, 0, None)


def _fit(lib, link, X=1 << 20, p=5, icpt=0, K=1, tol=1e-13, rows=10):
    first, nrows = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(rows)
    return getattr(lib, "dlsa_%s_fit_f64" % link)(X, p, 1 << 20, None, first, nrows, 1, K, p, icpt, tol, 100, 1 << 20, 1 << 20, 1 << 20, None,
                                                  None, None, None, 0, None)


@pytest.mark.parametrize("link", LINKS)
def test_refusals_come_before_any_hip_call(lib, link):
    """the pointers are never followed: a refusal comes on a machine without a GPU"""
    assert _pass(lib, link, X=None) == 1 and "%s_pass: null" % link in _lib.last_error()
    assert _fit(lib, link, X=None) == 1 and "%s_fit: null" % link in _lib.last_error()
    for kw in (dict(p=0), dict(p=2048, icpt=1), dict(n=0), dict(ldx=4)):
        assert _pass(lib, link, **kw) == 1 and "%s_pass: bad shape" % link in _lib.last_error(), kw
    for kw in (dict(p=0), dict(p=2048, icpt=1), dict(K=0)):
        assert _fit(lib, link, **kw) == 1 and "%s_fit: bad shape" % link in _lib.last_error(), kw
    assert _fit(lib, link, tol=0.0) == 1 and "tol" in _lib.last_error()
    assert _fit(lib, link, rows=-1) == 1 and "partition 0" in _lib.last_error()
    assert _pass(lib, link) == 3 and "%s_pass: workspace" % link in _lib.last_error()        # DLSA_ERR_WORKSPACE: a null workspace
    assert _fit(lib, link) == 3 and "%s_fit: workspace" % link in _lib.last_error()


@pytest.mark.parametrize("link", LINKS)
def test_query_is_zero_for_refused_shapes_and_is_the_poisson_query_in_shape(lib, link):
    q = getattr(lib, "dlsa_%s_workspace_bytes" % link)
    for args in [(100, 0, 0, 1), (100, 2048, 1, 1), (100, 2049, 0, 1), (-1, 5, 0, 1), (100, 5, 0, 0)]:
        assert q(*args) == 0, args
    assert q(100, 2048, 0, 1) > 0 and q(100, 2047, 1, 1) > 0                                  # pe = 2048 is the last accepted
    for p in (5, 130, 600):
        sizes = [q(n, p, 1, 1) for n in (0, 1, 1000, 1001, 50_000, 1_000_000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], (p, sizes)
        assert q(1000, p, 1, 4) >= q(1000, p, 1, 1) + 2 * 8 * 1000                            # room for the gathered responses and offsets


# ---- what the wrappers hand to the C ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
def test_fit_ex(fake, link, step, icpt, with_offset):  # noqa: F811
    X, y, offset = tm.rows()
    offset = offset if with_offset else None
    first, nrows = tm.PARTS[step]
    r = getattr(engine, link + "_fit_ex")(X, y, first, nrows, row_step=step, offset=offset, fit_intercept=icpt, tol=1e-9, max_iter=17)
    tm.check_fit_result(r, tm.P + int(icpt))
    tm.check_call(fake, "dlsa_%s_fit_f64" % link,
                  [tm.ptr(X), tm.val(4), tm.ptr(y), tm.ptr(offset), tm.arr(tm.I64, first), tm.arr(tm.I64, nrows), tm.val(step), tm.val(tm.K),
                   tm.val(tm.P), tm.val(int(icpt)), tm.val(1e-9), tm.val(17)] + tm.OUT3 + tm.HOST3 + tm.TAIL, r)
    assert fake.ws_calls == [("dlsa_%s_workspace_bytes" % link, (4, tm.P, int(icpt), step))]


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w", [(True, False), (False, True)])
def test_pass(fake, link, icpt, with_offset, want_H, want_w):  # noqa: F811
    X, y, offset = tm.rows()
    offset = offset if with_offset else None
    pe = tm.P + int(icpt)
    beta = torch.zeros(pe, dtype=torch.float64)
    res = getattr(engine, link + "_pass")(X, y, beta, offset=offset, fit_intercept=icpt, want_H=want_H, want_w=want_w)
    assert isinstance(res, tuple) and len(res) == 4
    for t, shape, want in zip(res, [(pe, pe), (pe,), (1,), (tm.N,)], [want_H, True, True, want_w]):
        assert (t is None) if not want else (tuple(t.shape) == shape and t.dtype == torch.float64)
    r = dict(zip(["H", "g", "ll", "w"], res))
    tm.check_call(fake, "dlsa_%s_pass_f64" % link,
                  [tm.ptr(X), tm.val(4), tm.ptr(y), tm.ptr(offset), tm.ptr(beta), tm.val(tm.N), tm.val(tm.P), tm.val(int(icpt)),
                   tm.out("H"), tm.val(pe), tm.out("g"), tm.out("ll"), tm.out("w")] + tm.TAIL, r)
    assert fake.ws_calls == [("dlsa_%s_workspace_bytes" % link, (tm.N, tm.P, int(icpt), 1))]


@pytest.mark.parametrize("link", LINKS)
def test_wrappers_check_lengths(fake, link):  # noqa: F811
    X, y, offset = tm.rows()
    with pytest.raises(ValueError):
        getattr(engine, link + "_fit_ex")(X, y[:-1], *tm.PARTS[1])
    with pytest.raises(ValueError):
        getattr(engine, link + "_fit_ex")(X, y, *tm.PARTS[1], offset=offset[:-1])
    with pytest.raises(ValueError):
        getattr(engine, link + "_pass")(X, y, torch.zeros(tm.P + 1, dtype=torch.float64))
    assert not fake.calls


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("with_exposure", [False, True])
def test_fit_partitions_marshals(fake, link, with_exposure):  # noqa: F811
    X, y, _ = tm.rows()
    X, y = _on_device(X), _on_device((y > 0).to(torch.float64))
    e = torch.linspace(0.5, 2.0, tm.N, dtype=torch.float64) if with_exposure else None
    mb = getattr(models, "fit_%s_partitions" % link)(X, y, partition_num=2, fit_intercept=True, exposure=e, tol=1e-9, max_iter=17)
    name, a = fake.calls[0]
    first, nrows = tm.PARTS[2]
    assert name == "dlsa_%s_fit_f64" % link and len(fake.calls) == 1 and len(a) == len(_lib.BINARY_SIGNATURES[name][1])
    assert tm.addr(a[0]) == X.data_ptr() and a[1] == 4 and tm.addr(a[2]) == y.data_ptr()
    if with_exposure:                                        # the offset the kernel reads is a tensor of its own: log(exposure)
        assert tm.addr(a[3]) not in (0, e.data_ptr())
    else:
        assert tm.addr(a[3]) == 0
    assert list(a[4]) == first and list(a[5]) == nrows and a[6:12] == (2, 2, tm.P, 1, 1e-9, 17)
    assert mb.names == ["intercept", "x0", "x1", "x2"] and mb.coef.shape == (2, 4) and mb.sample_size == tm.N and mb.extra == {}


# ---- the Python-level refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
def test_python_refusals(fake, link):  # noqa: F811
    X, y, offset = tm.rows()
    X, good = _on_device(X), (y > 0).to(torch.float64)
    fit = getattr(models, "fit_%s_partitions" % link)
    for bad in (2.0, 0.5, float("nan")):
        yb = good.clone(); yb[3] = bad
        with pytest.raises(ValueError, match="fit_%s_partitions: the response must be 0 or 1" % link):
            fit(X, _on_device(yb))
    with pytest.raises(ValueError, match="not both"):
        fit(X, _on_device(good), offset=offset, exposure=torch.ones(tm.N, dtype=torch.float64))
    with pytest.raises(ValueError, match="exposure must be positive"):
        fit(X, _on_device(good), exposure=torch.zeros(tm.N, dtype=torch.float64))
    with pytest.raises(ValueError, match="y must have n = 7"):
        fit(X, _on_device(good[:-1]))
    with pytest.raises(ValueError, match="n = 7 elements"):
        fit(X, _on_device(good), offset=offset[:-1])
    with pytest.raises(RuntimeError, match="GPU only"):
        fit(tm.rows()[0], good)
    assert not fake.calls


def test_the_public_names():
    import dlsa_amd
    for name in ("fit_probit_partitions", "fit_cloglog_partitions", "probit_model", "cloglog_model", "probit_model_eval", "cloglog_model_eval",
                 "simulate_binary"):
        assert callable(getattr(dlsa_amd, name)), name
    assert set(LINKS) <= set(engine.GLM_FAMILIES) and engine.GLM_FAMILIES["probit"] == engine.GLM_FAMILIES["poisson"]._replace(name="probit")
    import inspect
    for link in LINKS:                                       # dense rows only so far: no `structured` keyword
        for fn in ("%s_model", "%s_model_eval", "fit_%s_partitions"):
            assert "structured" not in inspect.signature(getattr(dlsa_amd, fn % link)).parameters
        assert not hasattr(dlsa_amd, "fit_%s_design" % link)


def test_probit_start_value_is_the_normal_quantile(tmp_path):
    """dlsa_amd/csrc/binary_start.h (the intercept's start value of the probit fit) compiled into a small program: the quantile of
    ones / rows against scipy's ndtri for shares from 1e-6 to 1 - 1e-6 and beyond, rare shares included -- a Newton iteration from
    the logit's scaling leaves the root for shares outside 0.005 .. 0.995"""
    special = pytest.importorskip("scipy.special")
    src = tmp_path / "quantile.c"
    src.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "binary_start.h"\n'
                   'int main(int argc, char** argv) {\n'
                   '    for (int i = 1; i + 1 < argc; i += 2) printf("%.17g\\n", dlsa_probit_quantile(atof(argv[i]), atof(argv[i + 1])));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "quantile"
    subprocess.run(["gcc", "-O1", "-std=c99", "-I", os.path.join(ROOT, "dlsa_amd", "csrc"), str(src), "-o", str(exe), "-lm"], check=True)
    cases = [(1.0, 1e9), (1.0, 1e6), (7.0, 4000.0), (1.0, 1000.0), (2.0, 1000.0), (3.0, 1000.0), (5.0, 1000.0), (1.0, 100.0), (3.0, 10.0),
             (1.0, 2.0), (1999.0, 4000.0), (2001.0, 4000.0), (7.0, 10.0), (995.0, 1000.0), (997.0, 1000.0), (999.0, 1000.0), (3993.0, 4000.0),
             (999999.0, 1e6), (1e9 - 1.0, 1e9)]
    args = [repr(v) for c in cases for v in c]
    got = [float(v) for v in subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.split()]
    assert len(got) == len(cases)
    for (ones, rows), x in zip(cases, got):
        # the upper tail by the mirror image, as the function takes it: 1 - ones / rows has lost its digits next to 1
        want = special.ndtri(ones / rows) if ones <= rows - ones else -special.ndtri((rows - ones) / rows)
        assert abs(x - want) <= 1e-13 * max(1.0, abs(want)), (ones, rows, x, want)
    assert got[cases.index((1.0, 2.0))] == 0.0


def test_coefficient_tables_are_what_the_generator_writes():
    """dlsa_amd/csrc/binary_terms.h holds, between its marker lines, exactly what tools/gen_binary_terms_coef.py writes"""
    pytest.importorskip("mpmath")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_binary_terms_coef.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
