"""CPU checks of the ordinal (proportional-odds) map step: the numpy reference (tests/ordinal_reference.py) against central differences
and against a longdouble run of itself, C = 2 against the logistic fit, the extreme case, unordered cutpoints, the Newton loop from the
null-model start and the calibration seed; the extension header include/dlsa_hip_ordinal.h against _lib.ORDINAL_SIGNATURES and the
built library; and what the three entries refuse without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import multinomial_reference as mr
import ordinal_reference as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["dlsa_ordinal_workspace_bytes", "dlsa_ordinal_pass_f64", "dlsa_ordinal_fit_f64"]


def rel(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,C", [(300, 4, 4), (200, 3, 2), (400, 5, 8)])
def test_terms_against_central_differences(n, p, C):
    """the score and the observed information are the first and (minus) the second derivatives of loglik: central differences in
    longdouble with h = 1e-6 (truncation ~ h^2)"""
    X, y = orf.data(1, n, p, C)
    theta = orf.away_from_optimum(p, C).astype(np.longdouble)
    ll, g, H, _ = orf.terms(X, y, theta, C, np.longdouble)
    d, h = len(theta), np.longdouble(1e-6)
    gfd, Hfd = np.zeros(d, np.longdouble), np.zeros((d, d), np.longdouble)
    for i in range(d):
        e = np.zeros(d, np.longdouble)
        e[i] = h
        up, dn = orf.terms(X, y, theta + e, C, np.longdouble), orf.terms(X, y, theta - e, C, np.longdouble)
        gfd[i] = (up[0] - dn[0]) / (2 * h)
        Hfd[:, i] = -(up[1] - dn[1]) / (2 * h)
    print("ordinal reference against central differences n=%d p=%d C=%d: g %.1e H %.1e" % (n, p, C, rel(gfd, g), rel(Hfd, H)))
    assert rel(gfd, g) <= 1e-9 and rel(Hfd, H) <= 1e-9


@pytest.mark.parametrize("n,p,C", [(6001, 5, 3), (6001, 5, 8), (4001, 1, 2), (4001, 2, 4), (1003, 129, 3)])
def test_fp64_against_longdouble(n, p, C):
    X, y = orf.data(10 + p, n, p, C)
    theta = orf.away_from_optimum(p, C)
    a, b = orf.terms(X, y, theta, C), orf.terms(X, y, theta, C, np.longdouble)
    errs = [rel(u, v) for u, v in zip(a, b)]
    print("ordinal fp64 against longdouble n=%d p=%d C=%d: ll %.1e g %.1e H %.1e w %.1e" % ((n, p, C) + tuple(errs)))
    assert max(errs) <= 1e-13


@pytest.mark.parametrize("p,C", [(7, 3), (50, 5), (20, 8)])
def test_information_is_symmetric_and_psd(p, C):
    X, y = orf.data(80 + p, 3 * p + 37, p, C)
    H = orf.terms(X, y, orf.away_from_optimum(p, C), C)[2]
    assert np.array_equal(H, H.T)
    ev = np.linalg.eigvalsh(H)
    assert ev[0] >= -1e-12 * ev[-1], ev[0]


@pytest.mark.parametrize("p", [5, 50])
def test_two_classes_are_the_logistic_model(p):
    """theta = [-intercept | beta]"""
    n = 600
    X, y = orf.data(90 + p, n, p, 2)
    b, S, ll, _ = orf.fit(X, y, 2)
    bl, Sl, lll = mr.logistic_fit(X, y, True)
    sgn = np.ones(p + 1)
    sgn[0] = -1.0
    errs = {"coef": rel(b * sgn, bl), "Sig_inv": rel(S * sgn[:, None] * sgn[None, :], Sl), "ll": abs((ll - lll) / lll)}
    print("ordinal C = 2 against the logistic fit p=%d: %s" % (p, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v <= 1e-12 for v in errs.values()), errs


def test_extreme_case_is_finite_and_matches_longdouble():
    X, y, theta = orf.extreme_case()
    C = orf.EXTREME_CLASSES
    reach = np.abs(theta[None, :C - 1] - (X @ theta[C - 1:])[:, None]).max()
    assert 590 < reach < 610 and theta[2] - theta[1] < 1.1e-6 and set(range(C)) == set(y.astype(int))
    # every class but the 1e-6 wide one is the likely one somewhere (and is observed there)
    likely = (X @ theta[C - 1:])[:, None] > theta[None, :C - 1]
    assert set(likely.sum(1)[np.arange(len(y)) % 10 != 0]) == {0, 1, 3, 4}
    a, b = orf.terms(X, y, theta, C), orf.terms(X, y, theta, C, np.longdouble)
    assert all(np.isfinite(v).all() for v in a)
    errs = [rel(u, v) for u, v in zip(a, b)]
    print("ordinal extreme case fp64 against longdouble: ll %.1e g %.1e H %.1e w %.1e" % tuple(errs))
    assert max(errs) <= 1e-13


@pytest.mark.parametrize("C", [3, 5, 8])
def test_unordered_cutpoints_give_nan(C):
    X, y = orf.data(3, 200, 4, C)
    assert np.isnan(orf.terms(X, y, orf.unordered(4, C), C)[0])
    theta = orf.away_from_optimum(4, C)
    theta[1] = theta[0]                                     # equal cutpoints are not strictly increasing either
    assert np.isnan(orf.terms(X, y, theta, C)[0])
    assert np.isfinite(orf.terms(X, y, orf.away_from_optimum(4, C), C)[0])


@pytest.mark.parametrize("n,p,C", orf.FIT_SHAPES)
def test_fit_converges_from_the_start(n, p, C):
    X, y = orf.data(40 + p, n, p, C)
    cnt = np.bincount(y.astype(int), minlength=C)
    b, S, ll, n_iter = orf.fit(X, y, C)
    g = orf.terms(X, y, b, C)[1]
    print("ordinal reference fit n=%d p=%d C=%d: %d evaluations, |g| %.1e, smallest class %d, condition %.1e"
          % (n, p, C, n_iter, np.max(np.abs(g)), cnt.min(), np.linalg.cond(S)))
    assert cnt.min() >= 20 and 5 <= n_iter <= 6 and np.max(np.abs(g)) <= 1e-9 * n
    assert np.linalg.eigvalsh(S)[0] > 0 and np.linalg.cond(S) <= 1.2e2 and np.all(np.diff(b[:C - 1]) > 0)


def test_start_is_the_mle_of_the_null_model():
    X, y = orf.data(5, 400, 3, 4)
    theta = orf.start(y, 3, 4)
    assert np.all(theta[3:] == 0) and np.max(np.abs(orf.terms(X, y, theta, 4)[1][:3])) <= 1e-11


def test_calibration_seed_sits_within_two_sigma():
    """Q is chi-square on 168 degrees of freedom (sigma = sqrt(336) = 18.33): the GPU file asserts 168 +- 73.3 (4 sigma) on the
    engine's blocks; here the reference alone lies within 168 +- 36.7 for the chosen seed, so a 1e-10 difference cannot tip that test"""
    X, y = orf.calibration_case()
    K = orf.CALIBRATION_K
    fits = [orf.fit(X[k::K], y[k::K], orf.CALIBRATION_CLASSES) for k in range(K)]
    q = orf.calibration_q([f[0] for f in fits], [f[1] for f in fits])
    print("ordinal calibration (reference): Q = %.2f on %d" % (q, orf.CALIBRATION_DF))
    assert orf.CALIBRATION_DF == 168 and abs(q - 168.0) <= 36.7 and abs(q - orf.CALIBRATION_Q_REFERENCE) <= 0.01, q


# ---- header <-> ORDINAL_SIGNATURES <-> the library -----------------------------------------------------------------------------------
def _declarations():
    with open(os.path.join(ROOT, "include", "dlsa_hip_ordinal.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"^\s*(size_t|int)\s+(dlsa_\w+)\s*\(([^;]*)\)\s*;", text, re.M)}


def test_header_declares_exactly_the_bound_table():
    from dlsa_amd import _lib
    decl = _declarations()
    assert sorted(decl) == sorted(_lib.ORDINAL_SIGNATURES) == sorted(ENTRIES)
    for name, (res, args) in decl.items():
        bound_res, bound_args = _lib.ORDINAL_SIGNATURES[name]
        assert len(args.split(",")) == len(bound_args), name
        assert bound_res is (_lib.c_sz if res == "size_t" else _lib.c_int), name
        # parameter by parameter: pointers to host ints / doubles, device pointers, scalars
        for text, ctype in zip(args.split(","), bound_args):
            text = " ".join(text.split())
            if "_host" in text:
                want = ctypes.POINTER({"int64_t": _lib.c_i64, "int": _lib.c_int, "double": _lib.c_dbl}[text.replace("const ", "").split("*")[0].strip()])
            elif "*" in text:
                want = _lib.c_vp
            else:
                want = {"int64_t": _lib.c_i64, "int": _lib.c_int, "double": _lib.c_dbl, "size_t": _lib.c_sz}[text.split()[0]]
            assert ctype is want or ctype == want, (name, text)
    with open(os.path.join(ROOT, "include", "dlsa_hip_ordinal.h")) as f:
        assert '#include "dlsa_hip.h"' in f.read()


def test_the_main_table_is_as_it_was_and_the_tables_are_disjoint():
    from dlsa_amd import _lib
    assert len(_lib.SIGNATURES) == 111 and not set(_lib.SIGNATURES) & set(_lib.ORDINAL_SIGNATURES)
    with open(os.path.join(ROOT, "include", "dlsa_hip.h")) as f:
        assert "ordinal" not in f.read()


@pytest.fixture(scope="module")
def lib():
    from dlsa_amd import _lib
    return _lib.load()


def test_library_exports_and_binds_the_entries(lib):
    from dlsa_amd import _lib
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.ORDINAL_SIGNATURES[name][1] and fn.restype is _lib.ORDINAL_SIGNATURES[name][0]


# ---- refusals without a GPU: every argument is judged before any HIP call --------------------------------------------------------------
def _pass(lib, X=1 << 20, classes=3, p=5, n=10, ldx=None):
    return lib.dlsa_ordinal_pass_f64(X, p if ldx is None else ldx, 1 << 20, 1 << 20, classes, n, p, None, 0, None, None, None, None, 0, None)


def _fit(lib, X=1 << 20, classes=3, p=5):
    first, rows = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(10)
    return lib.dlsa_ordinal_fit_f64(X, p, 1 << 20, first, rows, 1, 1, p, classes, 1e-13, 100, 1 << 20, 1 << 20, 1 << 20, None, None, None,
                                    None, 0, None)


@pytest.mark.parametrize("kw,text", [(dict(X=None), "null X"), (dict(classes=1), "classes must lie in 2 .. 8, got 1"),
                                     (dict(classes=9), "classes must lie in 2 .. 8, got 9"), (dict(classes=8, p=2042), "exceed the solver's 2048"),
                                     (dict(p=0), "bad shape p=0")])
def test_refusals_name_the_argument(lib, kw, text):
    """the pointers are never followed: a refusal comes before any HIP call, so it comes on a machine without a GPU"""
    from dlsa_amd import _lib
    for call, who in ((_pass, "ordinal_pass"), (_fit, "ordinal_fit")):
        assert call(lib, **kw) == 1
        msg = _lib.last_error()
        assert who in msg and (text in msg or (text == "null X" and "null argument (X" in msg)), msg


def test_the_workspace_is_judged_before_any_hip_call(lib):
    from dlsa_amd import _lib
    assert _pass(lib) == 3 and "ordinal_pass: workspace" in _lib.last_error()        # DLSA_ERR_WORKSPACE: a null workspace
    assert _fit(lib) == 3 and "ordinal_fit: workspace" in _lib.last_error()
    assert _pass(lib, n=0) == 1 and _pass(lib, ldx=4) == 1


def test_query_is_zero_for_refused_shapes_and_monotone_in_rows(lib):
    q = lib.dlsa_ordinal_workspace_bytes
    for args in [(100, 5, 1, 1), (100, 5, 9, 1), (100, 0, 3, 1), (100, 2042, 8, 1), (-1, 5, 3, 1), (100, 5, 3, 0)]:
        assert q(*args) == 0, args
    assert q(100, 2041, 8, 1) > 0                            # d = 2048 is the last accepted
    for p, C in [(5, 3), (130, 8), (257, 5), (600, 3)]:
        sizes = [q(n, p, C, 1) for n in (0, 1, 1000, 1001, 50_000, 1_000_000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], (p, C, sizes)
        assert q(1000, p, C, 4) >= q(1000, p, C, 1) + 8 * 1000                      # room for the gathered responses


@pytest.mark.parametrize("classes,p,text", [(1, 5, "classes must lie in 2 .. 8"), (9, 5, "classes must lie in 2 .. 8"),
                                            (8, 2042, "exceed the solver's 2048"), (2.5, 5, "must be an integer")])
def test_class_count_is_checked_in_python(classes, p, text):
    engine = pytest.importorskip("dlsa_amd.engine")
    with pytest.raises(ValueError, match=text):
        engine.ordinal_classes("ordinal_fit_ex", classes, p)
    assert engine.ordinal_classes("ordinal_fit_ex", 8, 2041) == 8


def test_column_names_put_the_cutpoints_first():
    models = pytest.importorskip("dlsa_amd.models")
    names = models.ordinal_column_names(["a", "b"], 4)
    assert names == ["intercept:1", "intercept:2", "intercept:3", "a", "b"] and models.intercept_columns(names) == [0, 1, 2]
