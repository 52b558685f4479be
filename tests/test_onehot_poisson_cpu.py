"""CPU checks of the structured one-hot Poisson map step (csrc/onehot_poisson.hip): the three C-ABI entries are exported and
bound, refuse null / bad arguments before any HIP call, the workspace query is 0 for bad arguments -- and the mirror header
csrc/onehot_plan.h holds token for token the definitions onehot.hip (whose source is pinned by committed counter evidence)
still carries itself.  A dlsa_onehot_plan cannot be created without a device (its level table is uploaded at creation), so the
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


# ---- the mirror header --------------------------------------------------------------------------------------------------
MIRRORED = [("const", n) for n in ("OH_MAXD", "OH_MAXF", "OH_THREADS", "OH_LOGIT_REP", "OH_LOGIT_MAX_BLOCKS")] + \
           [("struct", n) for n in ("OhTable", "OhRole", "OhDesc", "dlsa_onehot_plan")] + \
           [("func", n) for n in ("oh_logit_rep", "oh_logit_blocks", "oh_dense_row", "oh_block_sum")]


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


def test_mirror_header_is_token_identical_to_onehot_hip():
    src = _strip(open(os.path.join(CSRC, "onehot.hip")).read())
    mir = _strip(open(os.path.join(CSRC, "onehot_plan.h")).read())
    for kind, name in MIRRORED:
        a, b = _definition(src, kind, name), _definition(mir, kind, name)
        assert a and a == b, (kind, name)
    # the header mirrors, it does not add: every struct / function / constant it defines is on the list
    defined = set(re.findall(r"\bstruct\s+(\w+)\s*\{", mir)) | set(re.findall(r"constexpr\s+int\s+(\w+)\s*=", mir)) | \
        set(re.findall(r"^[ \t]*(?:static|__device__)[^\n;{}()]*\b(\w+)\s*\(", mir, flags=re.M))
    assert defined == {n for _, n in MIRRORED}, defined ^ {n for _, n in MIRRORED}


def test_mirror_guard_notices_a_drift():
    src = _strip(open(os.path.join(CSRC, "onehot.hip")).read())
    drifted = src.replace("constexpr int OH_MAXD = 8;", "constexpr int OH_MAXD = 9;")
    assert drifted != src and _definition(drifted, "const", "OH_MAXD") != _definition(src, "const", "OH_MAXD")
    drifted = src.replace("int lt0, ltn;", "int ltn, lt0;")
    assert drifted != src and _definition(drifted, "struct", "OhTable") != _definition(src, "struct", "OhTable")


def test_only_the_new_unit_includes_the_mirror_and_exp_full_is_shared():
    users = [f for f in sorted(os.listdir(CSRC)) if f != "onehot_plan.h" and '#include "onehot_plan.h"' in open(os.path.join(CSRC, f)).read()]
    assert users == ["onehot_poisson.hip"]
    # one polynomial: exp_full is defined in the shared header only
    defs = [f for f in sorted(os.listdir(CSRC)) if re.search(r"double\s+exp_full\s*\(\s*double", open(os.path.join(CSRC, f)).read())]
    assert defs == ["poisson_exp.h"]
