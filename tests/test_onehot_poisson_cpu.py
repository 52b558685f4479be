"""CPU checks of the structured one-hot Poisson map step (csrc/onehot_poisson.hip): the three C-ABI entries are exported and
bound, refuse null / bad arguments before any HIP call, the workspace query is 0 for bad arguments -- and the plan, its sizing
rules and the row passes' helpers are defined once (csrc/onehot_plan.h), for onehot.hip and onehot_poisson.hip alike.  A
dlsa_onehot_plan cannot be created without a device (its level table is uploaded at creation), so the
argument checks that need a plan run in tests/test_gpu_onehot_poisson.py."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "dlsa_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def test_entries_are_exported_and_bound(lib):
    from dlsa_amd import _lib
    import dlsa_amd
    hdr = open(os.path.join(ROOT, "include", "dlsa_hip.h")).read()
    for name in ("dlsa_onehot_poisson_workspace_bytes", "dlsa_onehot_poisson_pass_f64", "dlsa_onehot_poisson_fit_f64"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, hdr)
    assert callable(dlsa_amd.fit_poisson_design)
    from dlsa_amd import engine
    assert callable(engine.onehot_poisson_pass) and callable(engine.onehot_poisson_fit_ex)


def test_null_plan_and_null_pointers_are_refused_before_any_hip_call(lib):
    from dlsa_amd import _lib
    fake = ctypes.c_void_p(256)
    # pass(plan, num, ldn, codes, ldc, y, offset, beta, n, H, ldh, g, loglik, w_out, ws, ws_bytes, stream)
    args = [None, fake, 4, fake, 2, fake, None, fake, 10, fake, 5, None, None, None, fake, 1 << 30, None]
    assert lib.dlsa_onehot_poisson_pass_f64(*args) == 1
    assert "null plan" in _lib.last_error()
    # fit(plan, num, ldn, codes, ldc, y, offset, first, rows, step, K, tol, max_iter, coef, Sig_inv, Sig_invMcoef, n_iter, status,
    #     loglik, ws, ws_bytes, stream)
    first, rows = (ctypes.c_int64 * 2)(0, 5), (ctypes.c_int64 * 2)(5, 5)
    fargs = [None, fake, 4, fake, 2, fake, None, first, rows, 1, 2, 1e-13, 100, fake, fake, fake, None, None, None, fake, 1 << 30, None]
    assert lib.dlsa_onehot_poisson_fit_f64(*fargs) == 1
    assert "null argument" in _lib.last_error()
    # the null checks come first: a non-null plan is never dereferenced when another required pointer is null
    for i in (5, 7):
        a = list(args); a[0] = fake; a[i] = None
        assert lib.dlsa_onehot_poisson_pass_f64(*a) == 1, i
    for i in (5, 7, 8, 13, 14, 15):
        a = list(fargs); a[0] = fake; a[i] = None
        assert lib.dlsa_onehot_poisson_fit_f64(*a) == 1, i


def test_workspace_query_is_zero_for_bad_arguments(lib):
    # (monotonicity in max_rows needs a plan, hence a device: tests/test_gpu_onehot_poisson.py)
    assert lib.dlsa_onehot_poisson_workspace_bytes(None, 1000, 1) == 0
    assert lib.dlsa_onehot_poisson_workspace_bytes(None, -1, 1) == 0
    assert lib.dlsa_onehot_poisson_workspace_bytes(None, 1000, 0) == 0


# ---- one definition of the plan ------------------------------------------------------------------------------------------
SHARED = [("const", n) for n in ("OH_MAXD", "OH_MAXF", "OH_THREADS", "OH_LOGIT_REP", "OH_LOGIT_MAX_BLOCKS")] + \
         [("struct", n) for n in ("OhTable", "OhRole", "OhDesc", "dlsa_onehot_plan")] + \
         [("func", n) for n in ("oh_logit_rep", "oh_logit_blocks", "oh_dense_row", "oh_block_sum", "exp_neg")]


def _strip(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return text


def _braced(text, start):
    """text[start:] up to and including the brace group that opens at or after start"""
    i = text.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
        if depth == 0:
            return text[start:j]


def _definition(text, kind, name):
    """the definition of `name` in comment-free source text, without whitespace"""
    if kind == "const":
        hits = re.findall(r"constexpr\s+int\s+%s\s*=[^;]*;" % name, text)
    elif kind == "struct":
        hits = [_braced(text, m.start()) for m in re.finditer(r"\bstruct\s+%s\s*\{" % name, text)]
    else:
        # a function definition: its declaration specifiers start the line, the name is followed by the parameter list and a body
        hits = []
        for m in re.finditer(r"^[ \t]*((?:static|__device__|__forceinline__|inline)\b[^\n;{}()]*\b%s\s*\()" % name, text, flags=re.M):
            body_at = text.index("{", m.end())
            if ";" not in text[m.end():body_at]:
                hits.append(_braced(text, m.start(1)))
    assert len(hits) == 1, (kind, name, len(hits))
    return re.sub(r"\s+", "", hits[0])


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".inc"))}


def test_the_plan_and_the_pass_helpers_are_defined_once():
    src = _sources()
    everything = _strip("\n".join(src.values()))
    for kind, name in SHARED:
        assert _definition(everything, kind, name), (kind, name)          # (_definition asserts exactly one hit)
    # one row kernel and one launch driver, in onehot_pass.h; the copies they replace are gone
    assert len(re.findall(r"__global__[^;{]*\boh_row_kernel\s*\(", everything)) == 1 and "oh_row_kernel(" in src["onehot_pass.h"]
    assert _definition(everything, "func", "oh_row_pass") and _definition(_strip(src["onehot_pass.h"]), "func", "oh_row_pass")
    assert not any(gone in text for text in src.values() for gone in ("oh_exp_neg", "oh_logit_kernel", "oh_poisson_kernel"))
    for kind, name in SHARED[:-1]:
        assert _definition(_strip(src["onehot_plan.h"]), kind, name), (kind, name)
    assert _definition(_strip(src["logistic.h"]), "func", "exp_neg")


def test_a_second_definition_is_noticed():
    everything = _strip("\n".join(_sources().values()))
    for kind, name, again in (("const", "OH_MAXD", "constexpr int OH_MAXD = 8;"), ("struct", "OhTable", "struct OhTable { int t, u; };"),
                              ("func", "exp_neg", "__device__ __forceinline__ double exp_neg(double a) { return a; }")):
        with pytest.raises(AssertionError):
            _definition(everything + "\n" + again + "\n", kind, name)


def test_both_units_include_the_plan_header_and_exp_full_is_shared():
    for f in ("onehot.hip", "onehot_poisson.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "onehot_plan.h"' in text and '#include "onehot_pass.h"' in text, f
    # one polynomial: exp_full is defined in the shared header only
    defs = [f for f in sorted(os.listdir(CSRC)) if re.search(r"double\s+exp_full\s*\(\s*double", open(os.path.join(CSRC, f)).read())]
    assert defs == ["poisson_exp.h"]
