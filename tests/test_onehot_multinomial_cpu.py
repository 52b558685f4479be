"""CPU checks of the structured one-hot multinomial map step (csrc/onehot_multinomial.hip): the three C-ABI entries are exported,
bound and declared, refuse null arguments before any HIP call, the workspace query is 0 for bad arguments, the Python layers carry
the new functions and keywords, multinomial_classes refuses J p > 2048 without a GPU, and the softmax of a row is typed once, in
csrc/multinomial_internal.h, for the dense and the structured kernel alike.  A dlsa_onehot_plan cannot be created without a device,
so the checks that need a plan run in tests/test_gpu_onehot_multinomial.py."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "dlsa_amd", "csrc")
ENTRIES = ("dlsa_onehot_multinomial_workspace_bytes", "dlsa_onehot_multinomial_pass_f64", "dlsa_onehot_multinomial_fit_f64")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def test_entries_are_exported_bound_and_declared(lib):
    from dlsa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dlsa_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, hdr)
    # the bound argument counts are the declared ones
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "onehot_multinomial.hip" in open(os.path.join(ROOT, "Makefile")).read()


def test_python_layers_carry_the_functions_and_keywords():
    import dlsa_amd
    from dlsa_amd import engine, models
    assert callable(dlsa_amd.fit_multinomial_design) and dlsa_amd.fit_multinomial_design is models.fit_multinomial_design
    sig = inspect.signature(models.fit_multinomial_design)
    assert list(sig.parameters) == ["num", "codes", "y", "spec", "classes", "partition_num", "part_offsets", "structured", "tol", "max_iter"]
    assert sig.parameters["structured"].default is True
    assert list(inspect.signature(engine.onehot_multinomial_pass).parameters) == ["plan", "num", "codes", "y", "theta", "classes", "want_H",
                                                                                  "want_prob"]
    assert list(inspect.signature(engine.onehot_multinomial_fit_ex).parameters) == ["plan", "num", "codes", "y", "part_first", "part_rows",
                                                                                    "row_step", "classes", "tol", "max_iter"]
    for f in (models.multinomial_model, models.multinomial_model_eval):
        assert inspect.signature(f).parameters["structured"].default is False, f.__name__
    # the other families' design fits still get spec.names: _fit_design's names keyword defaults to None
    assert inspect.signature(models._fit_design).parameters["names"].default is None


def test_multinomial_classes_refuses_too_many_coefficients_without_a_gpu():
    from dlsa_amd import engine
    assert engine.multinomial_classes("x", 8, 292) == 8           # 7 * 292 = 2044
    with pytest.raises(ValueError, match="exceed the solver's 2048"):
        engine.multinomial_classes("x", 8, 293)
    with pytest.raises(ValueError, match="exceed the solver's 2048"):
        engine.multinomial_classes("x", 3, 1025)
    for bad in (1, 9):
        with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
            engine.multinomial_classes("x", bad, 5)


def test_null_plan_and_null_pointers_are_refused_before_any_hip_call(lib):
    from dlsa_amd import _lib
    fake = ctypes.c_void_p(256)
    # pass(plan, num, ldn, codes, ldc, y, theta, classes, n, H, ldh, g, loglik, prob_out, ldprob, ws, ws_bytes, stream)
    args = [None, fake, 4, fake, 2, fake, fake, 3, 10, fake, 10, None, None, None, 0, fake, 1 << 30, None]
    assert lib.dlsa_onehot_multinomial_pass_f64(*args) == 1
    assert "null plan" in _lib.last_error()
    # fit(plan, num, ldn, codes, ldc, y, first, rows, step, K, classes, tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter, status,
    #     loglik, ws, ws_bytes, stream)
    first, rows = (ctypes.c_int64 * 2)(0, 5), (ctypes.c_int64 * 2)(5, 5)
    fargs = [None, fake, 4, fake, 2, fake, first, rows, 1, 2, 3, 1e-13, 100, fake, fake, fake, None, None, None, fake, 1 << 30, None]
    assert lib.dlsa_onehot_multinomial_fit_f64(*fargs) == 1
    assert "null argument" in _lib.last_error()
    # the null checks come first: a non-null plan is never dereferenced when another required pointer is null
    for i in (5, 6):
        a = list(args); a[0] = fake; a[i] = None
        assert lib.dlsa_onehot_multinomial_pass_f64(*a) == 1, i
    for i in (5, 6, 7, 13, 14, 15):
        a = list(fargs); a[0] = fake; a[i] = None
        assert lib.dlsa_onehot_multinomial_fit_f64(*a) == 1, i


def test_workspace_query_is_zero_for_bad_arguments(lib):
    # (a bad class count, J p > 2048, max_rows < 0 and row_step < 1 on a real plan: tests/test_gpu_onehot_multinomial.py)
    for a in ((None, 1000, 3, 1), (None, -1, 3, 1), (None, 1000, 3, 0), (None, 1000, 1, 1), (None, 1000, 9, 1)):
        assert lib.dlsa_onehot_multinomial_workspace_bytes(*a) == 0, a


# ---- the softmax of a row is typed once ---------------------------------------------------------------------------------------
def _strip(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _sources():
    return {f: _strip(open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".inc"))}


def test_the_softmax_of_a_row_is_typed_once():
    src = _sources()
    defs = [f for f, t in src.items() if re.search(r"double\s+mn_softmax_row\s*\(", t)]
    assert defs == ["multinomial_internal.h"]
    # both row kernels call it, and neither carries the log1p of the row's term itself
    for f in ("multinomial.hip", "onehot_multinomial.hip"):
        assert len(re.findall(r"\bmn_softmax_row\s*<\s*J\s*>\s*\(", src[f])) == 1, f
        assert "log1p" not in src[f] and '#include "multinomial_internal.h"' in open(os.path.join(CSRC, f)).read(), f
    assert len(re.findall(r"\blog1p\s*\(", src["multinomial_internal.h"])) == 1
    # what the sibling shares lives in the header; the kernels stay in the unit that launches them
    hdr = src["multinomial_internal.h"]
    for name in ("MN_MAX_CLASSES", "MN_NQ", "MN_BAD", "MN_CHECK_BLOCKS", "MnStart", "MnFitBufs", "mn_ldprob", "mn_fit_core", "mn_check",
                 "mn_weight", "mn_mirror", "mn_start", "mn_ll_fix", "mn_coef_ok"):
        assert re.search(r"\b%s\b" % name, hdr), name
    assert "__global__" not in hdr
    for kernel in ("mn_weight_kernel", "mn_mirror_kernel", "mn_start_kernel", "mn_ll_fix_kernel", "mn_check_kernel"):
        assert [f for f, t in src.items() if re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, t)] == ["multinomial.hip"], kernel
    assert [f for f, t in src.items() if re.search(r"__global__[^;{]*\boh_mn_row_kernel\s*\(", t)] == ["onehot_multinomial.hip"]
