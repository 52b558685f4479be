"""CPU checks of the structured one-hot NB2 map step (csrc/onehot_negbin.hip): the three C-ABI entries are exported, bound and
declared, refuse null / bad arguments before any HIP call, the workspace query is 0 for bad arguments -- and the new unit is a
third row model of the one row pass (csrc/onehot_pass.h) that takes its arithmetic from where the dense NB2 pass has it.  A
dlsa_onehot_plan cannot be created without a device, so the argument checks that need a plan run in
tests/test_gpu_onehot_negbin.py."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "dlsa_amd", "csrc")
ENTRIES = ("dlsa_onehot_negbin_workspace_bytes", "dlsa_onehot_negbin_pass_f64", "dlsa_onehot_negbin_fit_f64")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def _strip(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_entries_are_exported_bound_and_declared(lib):
    from dlsa_amd import _lib
    hdr = _strip(open(os.path.join(ROOT, "include", "dlsa_hip.h")).read())
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name + " is not declared in include/dlsa_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the arguments of the two entries each combines, in their order: the structured Poisson entry's with the dense NB2 entry's extras
    sig = _lib.SIGNATURES
    assert len(sig["dlsa_onehot_negbin_pass_f64"][1]) == len(sig["dlsa_onehot_poisson_pass_f64"][1]) + 3 == 20
    assert len(sig["dlsa_onehot_negbin_fit_f64"][1]) == len(sig["dlsa_onehot_poisson_fit_f64"][1]) + 4 == 26


def test_python_interface_exists():
    import dlsa_amd
    from dlsa_amd import engine
    assert callable(dlsa_amd.fit_negbin_design)
    assert callable(engine.onehot_negbin_pass) and callable(engine.onehot_negbin_fit_ex)
    par = inspect.signature(dlsa_amd.fit_negbin_design).parameters
    assert par["structured"].default is True and par["alpha"].default is None
    for f in (dlsa_amd.negbin_model, dlsa_amd.negbin_model_eval):
        assert inspect.signature(f).parameters["structured"].default is False


def test_null_plan_and_null_pointers_are_refused_before_any_hip_call(lib):
    from dlsa_amd import _lib
    fake = ctypes.c_void_p(256)
    # pass(plan, num, ldn, codes, ldc, y, offset, beta, alpha, n, H, ldh, g, loglik, w_out, mu_out, theta_terms, ws, ws_bytes, stream)
    args = [None, fake, 4, fake, 2, fake, None, fake, 0.5, 10, fake, 5, None, None, None, None, None, fake, 1 << 30, None]
    assert lib.dlsa_onehot_negbin_pass_f64(*args) == 1
    assert "null plan" in _lib.last_error()
    # fit(plan, num, ldn, codes, ldc, y, offset, first, rows, step, K, alpha_fixed, tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter,
    #     status, loglik, alpha, alpha_info, pearson, ws, ws_bytes, stream)
    first, rows = (ctypes.c_int64 * 2)(0, 5), (ctypes.c_int64 * 2)(5, 5)
    fargs = [None, fake, 4, fake, 2, fake, None, first, rows, 1, 2, 0.0, 1e-13, 100, fake, fake, fake, None, None, None, None, None, None,
             fake, 1 << 30, None]
    assert lib.dlsa_onehot_negbin_fit_f64(*fargs) == 1
    assert "null argument" in _lib.last_error()
    # the null checks come first: a non-null plan (a fake one here) is never dereferenced when another required pointer is null
    for i in (5, 7):
        a = list(args); a[0] = fake; a[i] = None
        assert lib.dlsa_onehot_negbin_pass_f64(*a) == 1, i
    for i in (5, 7, 8, 14, 15, 16):
        a = list(fargs); a[0] = fake; a[i] = None
        assert lib.dlsa_onehot_negbin_fit_f64(*a) == 1, i


def test_workspace_query_is_zero_for_bad_arguments(lib):
    # (monotonicity in max_rows needs a plan, hence a device: tests/test_gpu_onehot_negbin.py)
    assert lib.dlsa_onehot_negbin_workspace_bytes(None, 1000, 1) == 0
    assert lib.dlsa_onehot_negbin_workspace_bytes(None, -1, 1) == 0
    assert lib.dlsa_onehot_negbin_workspace_bytes(None, 1000, 0) == 0


def test_the_unit_is_a_row_model_of_the_one_row_pass():
    text = open(os.path.join(CSRC, "onehot_negbin.hip")).read()
    assert '#include "onehot_plan.h"' in text and '#include "onehot_pass.h"' in text
    code = _strip(text)
    assert "oh_row_pass(" in code and "__global__" not in code          # no kernel of its own: it instantiates oh_row_kernel
    assert re.search(r"struct\s+OhNbRow\b", code) and "STORES_MU" in code
    assert "onehot_negbin.hip" in open(os.path.join(ROOT, "Makefile")).read()
    # the Gram runs in the ordered floating-point mode
    assert re.search(r"onehot_gram_impl\([^;]*,\s*false\s*\)\s*;", code)


def test_the_nb_arithmetic_is_typed_once():
    src = {f: _strip(open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".inc"))}
    # NbRow (w = mu q, r = (y - mu) q, the log1p / overflow rules) has one definition, shared by both units through negbin_internal.h
    assert [f for f, t in src.items() if re.search(r"struct\s+NbRow\s*\{", t)] == ["negbin_internal.h"]
    for f in ("negbin.hip", "onehot_negbin.hip"):
        assert '#include "negbin_internal.h"' in open(os.path.join(CSRC, f)).read(), f
    assert "nb.terms(" in src["onehot_negbin.hip"] and "log1p" not in src["onehot_negbin.hip"]
    # exp_full stays in poisson_exp.h, the special functions in negbin_special.h
    assert [f for f, t in src.items() if re.search(r"double\s+exp_full\s*\(\s*double", t)] == ["poisson_exp.h"]
    for fn in ("nb_digamma", "nb_trigamma", "nb_diffs"):
        defs = [f for f, t in src.items() if re.search(r"__device__[^;{}()]*\b%s\s*\(" % fn, t)]
        assert defs == ["negbin_special.h"], (fn, defs)
    # one theta kernel and one fit driver, both negbin.hip's
    assert [f for f, t in src.items() if re.search(r"__global__[^;{]*\bnegbin_theta_kernel\s*\(", t)] == ["negbin.hip"]
    assert [f for f, t in src.items() if re.search(r"\bint\s+nb_fit_core\s*\([^;{]*\)\s*\{", t)] == ["negbin.hip"]
    assert "nb_fit_core(" in src["onehot_negbin.hip"] and "newton_fit_loop" not in src["onehot_negbin.hip"]
