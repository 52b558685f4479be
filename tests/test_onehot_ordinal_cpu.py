"""CPU checks of the structured one-hot ordinal map step: the extension header include/dlsa_hip_onehot_ordinal.h against
_lib.ONEHOT_ORDINAL_SIGNATURES and the built library, the three signature tables apart, what the three entries refuse without a GPU,
and the inputs of tests/test_gpu_onehot_ordinal.py qualified on the reference alone: the fit cases, the extreme case and the case
list's coverage of both border routes and of 8, 4, 2 and 1 histogram copies."""
import ctypes
import os
import re

import numpy as np
import pytest

import onehot_ordinal_cases as cs
import ordinal_reference as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dlsa_hip_onehot_ordinal.h")
ENTRIES = ["dlsa_onehot_ordinal_workspace_bytes", "dlsa_onehot_ordinal_pass_f64", "dlsa_onehot_ordinal_fit_f64"]


def rel(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


# ---- header <-> ONEHOT_ORDINAL_SIGNATURES <-> the library -------------------------------------------------------------------------
def _declarations():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"^\s*(size_t|int)\s+(dlsa_\w+)\s*\(([^;]*)\)\s*;", text, re.M)}


def test_header_declares_exactly_the_bound_table():
    from dlsa_amd import _lib
    decl = _declarations()
    assert sorted(decl) == sorted(_lib.ONEHOT_ORDINAL_SIGNATURES) == sorted(ENTRIES)
    for name, (res, args) in decl.items():
        bound_res, bound_args = _lib.ONEHOT_ORDINAL_SIGNATURES[name]
        assert len(args.split(",")) == len(bound_args), name
        assert bound_res is (_lib.c_sz if res == "size_t" else _lib.c_int), name
        # parameter by parameter: pointers to host ints / doubles, device pointers (the plan handle among them), scalars
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
        assert '#include "dlsa_hip_ordinal.h"' in f.read()


def test_the_old_tables_are_as_they_were_and_the_three_are_disjoint():
    from dlsa_amd import _lib
    tables = [_lib.SIGNATURES, _lib.ORDINAL_SIGNATURES, _lib.ONEHOT_ORDINAL_SIGNATURES]
    assert [len(t) for t in tables] == [111, 3, 3]
    assert len(set().union(*tables)) == 117
    for old in ("dlsa_hip.h", "dlsa_hip_ordinal.h"):
        with open(os.path.join(ROOT, "include", old)) as f:
            assert "onehot_ordinal" not in f.read(), old


@pytest.fixture(scope="module")
def lib():
    from dlsa_amd import _lib
    return _lib.load()


def test_library_exports_and_binds_the_entries(lib):
    from dlsa_amd import _lib
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.ONEHOT_ORDINAL_SIGNATURES[name][1] and fn.restype is _lib.ONEHOT_ORDINAL_SIGNATURES[name][0]


# ---- refusals without a GPU: a null plan, y or theta is refused before any HIP call (and before the plan is followed) ---------------
def test_null_arguments_are_refused_before_any_hip_call(lib):
    from dlsa_amd import _lib
    P = 1 << 20                                                 # pointers that are never followed
    for plan, y, theta in [(None, P, P), (P, None, P), (P, P, None)]:       # the null check comes before the plan is followed
        assert lib.dlsa_onehot_ordinal_pass_f64(plan, P, 2, P, 2, y, theta, 3, 10, None, 0, None, None, None, None, 0, None) == 1
        assert "onehot_ordinal_pass: null plan, y or theta" in _lib.last_error()
    first, rows = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(10)
    assert lib.dlsa_onehot_ordinal_fit_f64(None, P, 2, P, 2, P, first, rows, 1, 1, 3, 1e-13, 100, P, P, P, None, None, None, None, 0, None) == 1
    assert "onehot_ordinal_fit: null argument" in _lib.last_error()


def test_query_is_zero_for_a_null_plan_and_bad_arguments(lib):
    q = lib.dlsa_onehot_ordinal_workspace_bytes
    P = 1 << 20                                                 # never followed: classes, rows and step are judged first
    for args in [(None, 100, 3, 1), (P, 100, 1, 1), (P, 100, 9, 1), (P, -1, 3, 1), (P, 100, 3, 0)]:
        assert q(*args) == 0, args


# ---- the inputs of the GPU tests, qualified on the reference alone ---------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.FIT_CASES + [cs.MASKED_FIT_CASE], ids=lambda c: "%d-%s-C%d-K%d" % (c[0], "x".join(map(str, c[2])), c[3], c[4]))
def test_fit_cases_qualify(case):
    n, q, nlevels, C, K, strided, seed, freq = case
    (p, num, codes, desc, nl, level_col, X, y), fits = cs.fit_reference(case)
    assert not np.any(desc[0] == 0) and p == cs.shape_p(q, nlevels, True)        # no constant column
    sl = cs.parts(n, K, strided)[0]
    for k, (s, (b, H, ll, evals, halvings)) in enumerate(zip(sl, fits)):
        cnt = np.bincount(y[s].astype(int), minlength=C)
        rows = (X[s] != 0).sum(0)
        ref = orf.fit(X[s], y[s], C)
        print("fit case", case, "partition", k, "smallest class", cnt.min(), "fewest rows of a column", rows.min(), "evaluations", evals,
              "halvings", halvings, "condition %.1e" % np.linalg.cond(H))
        assert cnt.min() > 0 and rows.min() >= 5 and halvings == 0 and evals <= 8
        assert ref[3] == evals and np.array_equal(ref[0], b) and np.array_equal(ref[1], H)     # fit_counted is orf.fit
        assert np.all(np.diff(b[:C - 1]) > 0) and np.linalg.eigvalsh(H)[0] > 0
    assert cs.lds_route(p, C)[0] == (case != cs.MASKED_FIT_CASE)


def test_extreme_case_is_finite_and_matches_longdouble():
    from oracle import dlsa_oracle
    p, num, codes, desc, nl, level_col, y, theta = cs.extreme_case()
    C = cs.EXTREME_CLASSES
    X, _ = dlsa_oracle.design_matrix(num, codes, *desc)
    assert X.shape == (2000, 3) and np.array_equal(X[:, 0], num[:, 0]) and set(np.unique(X[:, 1:])) == {0.0, 1.0}
    reach = np.abs(theta[None, :C - 1] - (X @ theta[C - 1:])[:, None]).max()
    assert 590 < reach < 610 and theta[2] - theta[1] < 1.1e-6 and set(range(C)) == set(y.astype(int))
    a, b = orf.terms(X, y, theta, C), orf.terms(X, y, theta, C, np.longdouble)
    assert all(np.isfinite(v).all() for v in a)
    errs = [rel(u, v) for u, v in zip(a, b)]
    print("structured extreme case, reach %.1f, fp64 against longdouble: ll %.1e g %.1e H %.1e w %.1e" % ((reach,) + tuple(errs)))
    assert max(errs) <= 1e-13


def test_the_case_list_holds_both_routes_and_every_copy_count():
    routes = {(cs.shape_p(q, nl, b), C): cs.lds_route(cs.shape_p(q, nl, b), C) for (n, q, nl, C, b) in cs.PASS_CASES}
    # the worked examples of the rule, baselines dropped
    assert routes[(708, 3)][:2] == (True, 1) and routes[(1000, 2)][:2] == (True, 1)
    assert routes[(708, 5)][0] is False and routes[(1405, 3)][0] is False
    assert cs.lds_route(260, 4)[0] and cs.lds_route(260, 8) == (True, 1, 8)       # the airline shape fits at every C
    assert {r[0] for r in routes.values()} == {True, False}
    assert {r[1] for r in routes.values() if r[0]} == {8, 4, 2, 1}                # copies of the C p-cell histogram, borders in the pass
    assert {r[1] for r in routes.values() if not r[0]} >= {2, 1}                  # copies of the p-cell histogram on the masked route
    ns = {n for (n, q, nl, C, b) in cs.PASS_CASES}
    assert 1 in ns and 257 in ns                                                   # one row; a masked second round
    assert all(C - 1 + cs.shape_p(q, nl, b) <= 2048 for (n, q, nl, C, b) in cs.PASS_CASES)
    assert len(cs.PASS_CASES) == 80


def test_the_python_names_exist():
    import dlsa_amd
    from dlsa_amd import engine, models
    assert dlsa_amd.fit_ordinal_design is models.fit_ordinal_design
    assert callable(engine.onehot_ordinal_pass) and callable(engine.onehot_ordinal_fit_ex)
    import inspect
    for fn in (models.ordinal_model, models.ordinal_model_eval):
        assert inspect.signature(fn).parameters["structured"].default is False
    assert inspect.signature(models.fit_ordinal_design).parameters["structured"].default is True
