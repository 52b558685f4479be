"""CPU checks of the stratified Cox map step: the per-stratum reference (tests/cox_strata_reference.py) checks itself (both
forms agree stratum by stratum, one stratum is the unstratified model, matched pairs give the closed form of conditional
logistic regression), the inputs of the GPU tests separate the stratified model from the unstratified one (so that a build
which ignored `strata` cannot pass them), the new C entries exist and validate their arguments before any HIP call, and the
Python argument errors need no GPU."""
import ctypes
import re

import numpy as np
import pytest

import cox_efron_reference as er
import cox_reference as cr
import cox_strata_cases as cases
import cox_strata_reference as sr


def _agree(a, b, X, tol):
    (l1, U1, H1), (l2, U2, H2) = a, b
    assert abs(l1 - l2) <= tol * max(1.0, abs(l1)), (l1, l2)
    assert np.max(np.abs(U1 - U2)) <= tol * max(1.0, np.abs(X).sum(0).max())
    assert np.max(np.abs(H1 - H2)) <= tol * max(np.max(np.abs(H1)), np.max(X * X))


@pytest.mark.parametrize("name", cases.LAYOUTS)
@pytest.mark.parametrize("p,n", [(1, 7), (5, 7), (1, 300), (5, 300), (50, 300), (130, 300), (5, 5000)])
def test_reference_forms_agree_stratum_by_stratum(p, n, name):
    """the pass cases of the GPU test, every layout; for run time the wide rows (p = 520, and p >= 50 at n = 5000, where the loop
    form builds a p x p matrix per event time and stratum) are left to the narrower ones: both forms treat the columns alike"""
    X, t, ev, beta, strata = cases.pass_case(p, n, name)
    _agree(sr.stratified(er.efron_loop, X, t, ev, strata, beta), sr.stratified(er.efron_cumsum, X, t, ev, strata, beta), X, 1e-12)
    _agree(sr.stratified(cr.breslow_loop, X, t, ev, strata, beta), sr.stratified(cr.breslow_cumsum, X, t, ev, strata, beta), X, 1e-12)


def test_one_stratum_is_the_unstratified_model():
    X, t, ev, beta, _ = cases.pass_case(5, 300, "random7")
    one = np.full(300, -7)
    for form in (er.efron_loop, er.efron_cumsum, cr.breslow_loop, cr.breslow_cumsum):
        l0, U0, H0 = form(X, t, ev, beta)
        l1, U1, H1 = sr.stratified(form, X, t, ev, one, beta)
        assert l0 == l1 and np.array_equal(U0, U1) and np.array_equal(H0, H1)


def test_pairs_give_the_closed_form_of_conditional_logistic_regression():
    X, t, ev, beta, strata = cases.pairs_case()
    assert np.all(np.unique(strata, return_counts=True)[1] == 2)
    ref = sr.clogit_pairs(X, ev, strata, beta)
    for form in (cr.breslow_loop, cr.breslow_cumsum, er.efron_loop, er.efron_cumsum):
        _agree(ref, sr.stratified(form, X, t, ev, strata, beta), X, 1e-12)
    b, H, ll = sr.clogit_pairs_fit(X, ev, strata)
    b2, H2, ll2 = sr.fit(X, t, ev, strata)
    assert np.max(np.abs(b - b2)) <= 1e-12 * np.max(np.abs(b)) and abs(ll - ll2) <= 1e-12 * abs(ll)
    assert np.max(np.abs(H - H2)) <= 1e-12 * np.max(np.abs(H))
    assert np.all(np.linalg.eigvalsh(H) > 0)


def _separated(X, t, ev, beta, strata):
    form = er.efron_loop if len(t) <= 2000 else er.efron_cumsum
    ls, _, Hs = sr.stratified(form, X, t, ev, strata, beta)
    lu, _, Hu = form(X, t, ev, beta)
    return abs(ls - lu) / abs(lu), np.max(np.abs(Hs - Hu)) / np.max(np.abs(Hu))


@pytest.mark.parametrize("name", cases.LAYOUTS)
@pytest.mark.parametrize("p,n", [(1, 300), (5, 300), (50, 300), (130, 300), (520, 300), (1, 5000), (5, 5000), (50, 5000), (520, 5000)])
def test_gpu_pass_inputs_separate_stratified_from_unstratified(p, n, name):
    """the condition behind the GPU pass test, on its arrays.  Left out: n = 7 (in blocks64 its seven rows are a single
    stratum, which is the unstratified model), and p = 130 at n = 5000 for run time (p = 50 and 520 stand on both sides of it)"""
    dl, dH = _separated(*cases.pass_case(p, n, name))
    assert dl > 1e-4 and dH > 1e-4, (dl, dH)


@pytest.mark.parametrize("case", ["empty_strata", "all_tied", "boundary_ties"])
def test_gpu_edge_inputs_separate_stratified_from_unstratified(case):
    dl, dH = _separated(*cases.edge_case(case))
    assert dl > 1e-4 and dH > 1e-4, (dl, dH)


def test_gpu_eta_range_input_separates_stratified_from_unstratified():
    X, t, ev, beta, strata = cases.edge_case("eta_range")
    assert np.ptp(X @ beta) > 700
    dl, dH = _separated(X, t, ev, beta, strata)
    assert dl > 1e-4 and dH > 1e-4, (dl, dH)


def test_gpu_long_and_pairs_inputs_separate_stratified_from_unstratified():
    dl, dH = _separated(*cases.long_case())
    assert dl > 1e-4 and dH > 1e-4, (dl, dH)
    X, t, ev, beta, strata = cases.pairs_case()
    dl, dH = _separated(X, t, ev, beta, strata)
    assert dl > 1e-4 and dH > 1e-4, (dl, dH)


def test_edge_case_layouts_are_what_they_claim():
    X, t, ev, _, strata = cases.edge_case("empty_strata")
    o = cases.sort_order(t, strata)
    so = strata[o]
    assert not ev[strata == so[0]].any() and not ev[strata == so[-1]].any() and not ev[strata == 2].any() and ev[strata == 1].any()
    X, t, ev, _, strata = cases.edge_case("all_tied")
    for s in np.unique(strata):
        assert len(np.unique(t[strata == s])) == 1 and ev[strata == s].sum() >= 100
    X, t, ev, _, strata = cases.edge_case("boundary_ties")
    o = cases.sort_order(t, strata)
    b = np.nonzero(strata[o][1:] != strata[o][:-1])[0]
    assert len(b) == 4 and np.all(t[o][b] == t[o][b + 1])                  # equal times on the two sides of every boundary
    for q in b:
        assert ev[(strata == strata[o][q]) & (t == t[o][q])].any()
        assert ev[(strata == strata[o][q + 1]) & (t == t[o][q + 1])].any()
    strata = cases.layout("blocks64", 300, 1)
    so = np.sort(strata)
    assert np.array_equal(np.nonzero(so[1:] != so[:-1])[0] + 1, np.arange(64, 300, 64))
    sizes = np.unique(cases.layout("mixed", 300, 1), return_counts=True)[1]
    assert (sizes == 1).sum() == 1 and (sizes == 2).sum() == 3 and sizes.max() >= 200
    assert cases.layout("random7", 300, 1).min() < 0 and cases.layout("random7", 300, 1).max() > 2 ** 30


@pytest.mark.parametrize("p", [3, 20])
def test_gpu_fit_inputs_separate_stratified_from_unstratified(p):
    """on the first of the GPU test's two partitions (the second one is drawn the same way; half the run time)"""
    X, t, ev, strata = cases.fit_case(p)
    half = len(t) // 2
    X, t, ev, strata = X[:half], t[:half], ev[:half], strata[:half]
    bs, Hs, ls = sr.fit(X, t, ev, strata)
    bu, Hu, lu = er.fit(X, t, ev)
    assert np.max(np.abs(bs - bu)) / np.max(np.abs(bu)) > 1e-4
    assert abs(ls - lu) / abs(lu) > 1e-4 and np.max(np.abs(Hs - Hu)) / np.max(np.abs(Hu)) > 1e-4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dlsa_amd import _lib
    return _lib.load()


def test_new_symbols_are_exported_bound_and_declared(lib):
    import os
    from dlsa_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dlsa_hip.h")).read()
    for name in ("dlsa_cox_strata_workspace_bytes", "dlsa_cox_pass_strata_f64", "dlsa_cox_fit_strata_f64"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\b%s\(" % name, header)
    # the `_ties` signatures with one pointer after `event`
    for new, old in (("dlsa_cox_pass_strata_f64", "dlsa_cox_pass_ties_f64"), ("dlsa_cox_fit_strata_f64", "dlsa_cox_fit_ties_f64")):
        a, b = _lib.SIGNATURES[new][1], _lib.SIGNATURES[old][1]
        assert a[:4] == b[:4] and a[4] is ctypes.c_void_p and a[5:] == b[4:]
    assert "strata[order[q]] != strata[order[q-1]]" in header          # the adjacency contract is stated


def test_strata_workspace_query(lib):
    for p in (1, 5, 100, 500):
        for ties in (0, 1):
            prev = 0
            for n in (0, 1, 63, 64, 65, 1000, 4096 * 64, 4096 * 64 + 1, 10 ** 6, 10 ** 7):
                b0, b1 = lib.dlsa_cox_strata_workspace_bytes(n, p, ties, 0), lib.dlsa_cox_strata_workspace_bytes(n, p, ties, 1)
                assert b0 == lib.dlsa_cox_ties_workspace_bytes(n, p, ties) and b0 > 0
                assert b1 >= b0 + max(n, 1)                 # one flag byte per position
                assert b1 >= prev, (p, ties, n)
                prev = b1
    for bad in ((-1, 5, 0, 1), (100, 0, 0, 1), (100, 4096, 0, 1), (100, 5, 2, 1), (100, 5, -1, 0), (100, 5, 0, 2), (100, 5, 1, -1)):
        assert lib.dlsa_cox_strata_workspace_bytes(*bad) == 0, bad


# dlsa_cox_strata_workspace_bytes as the library of d1e44ca (the commit before the workspace became one list) returns it:
# (max_rows, p): (Breslow, Breslow stratified, Efron, Efron stratified)
WORKSPACE_BYTES = {
    (0, 1): (772608, 789248, 1084160, 1100800),
    (0, 5): (1165824, 1182464, 1739520, 1756160),
    (0, 500): (68360960, 68377600, 101374976, 101391616),
    (0, 2048): (503810048, 503826688, 638273792, 638290432),
    (1, 1): (772608, 789248, 1084160, 1100800),
    (1, 5): (1165824, 1182464, 1739520, 1756160),
    (1, 500): (68360960, 68377600, 101374976, 101391616),
    (1, 2048): (503810048, 503826688, 638273792, 638290432),
    (65, 1): (776192, 792832, 1088256, 1104896),
    (65, 5): (1171456, 1188096, 1745664, 1762304),
    (65, 500): (68619520, 68636160, 101634048, 101650688),
    (65, 2048): (504861184, 504877824, 639325440, 639342080),
    (4096 * 64 + 1, 1): (31967744, 32246528, 34376448, 34655232),
    (4096 * 64 + 1, 5): (40749568, 41028352, 43420416, 43699200),
    (4096 * 64 + 1, 500): (463156480, 463435264, 498267648, 498546432),
    (4096 * 64 + 1, 2048): (780748544, 781027328, 917309440, 917588224),
    (10 ** 7, 1): (577286144, 587302656, 657597440, 667613952),
    (10 ** 7, 5): (650854144, 660870656, 731427584, 741444096),
    (10 ** 7, 500): (1244527360, 1254543872, 1357541120, 1367557632),
    (10 ** 7, 2048): (11292906240, 11302922752, 11507369728, 11517386240),
}


def test_strata_workspace_bytes_are_pinned(lib):
    """the byte queries and the passes walk one list of the workspace arrays: its sizes, order and alignment are those of the
    three lists it replaced"""
    assert len(WORKSPACE_BYTES) == 5 * 4
    for (n, p), want in WORKSPACE_BYTES.items():
        got = tuple(lib.dlsa_cox_strata_workspace_bytes(n, p, ties, stratified) for ties in (0, 1) for stratified in (0, 1))
        assert got == want, (n, p, got, want)


def test_abi_validates_before_any_hip_call(lib):
    from dlsa_amd import _lib
    fake = ctypes.c_void_p(256)
    args = [fake, 4, fake, fake, fake, fake, 10, 4, 0, fake, fake, 4, None, None, None, fake, 1 << 20, None]
    offs = (ctypes.c_int64 * 3)(0, 5, 10)
    fargs = [fake, 4, fake, fake, fake, fake, offs, 2, 4, 0, 1e-13, 100, fake, fake, fake, None, None, None, fake, 1 << 20, None]
    for strata in (fake, None):                       # null strata are valid: the other checks still run
        for bad in (7, -1, 2):
            a = list(args); a[4] = strata; a[8] = bad
            assert lib.dlsa_cox_pass_strata_f64(*a) == 1 and "ties" in _lib.last_error()
            a = list(fargs); a[4] = strata; a[9] = bad
            assert lib.dlsa_cox_fit_strata_f64(*a) == 1 and "ties" in _lib.last_error()
        a = list(args); a[4] = strata; a[0] = None
        assert lib.dlsa_cox_pass_strata_f64(*a) == 1 and "null" in _lib.last_error()
        a = list(args); a[4] = strata; a[5] = None
        assert lib.dlsa_cox_pass_strata_f64(*a) == 1 and "null" in _lib.last_error()
        a = list(fargs); a[4] = strata; a[7] = 0
        assert lib.dlsa_cox_fit_strata_f64(*a) == 1
    # a workspace sized for the unstratified pass is too small for the stratified one
    n, p = 100_000, 4
    small = lib.dlsa_cox_strata_workspace_bytes(n, p, 0, 0)
    a = list(args); a[6] = n; a[16] = small
    assert lib.dlsa_cox_pass_strata_f64(*a) == 3 and "workspace" in _lib.last_error()      # DLSA_ERR_WORKSPACE


def test_python_argument_errors_need_no_gpu():
    import pandas as pd
    import torch
    import dlsa_amd
    from dlsa_amd import engine, models
    x = torch.zeros(4, 2, dtype=torch.float64)          # (CPU tensors: strata are checked first)
    o = torch.arange(4)
    for bad in (torch.zeros(4), torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.bool), [0, 0, 1, 1], np.zeros(4, int)):
        with pytest.raises(TypeError, match="strata"):
            engine.cox_pass(x, x[:, 0], x[:, 0], o, x[0], strata=bad)
        with pytest.raises(TypeError, match="strata"):
            engine.cox_fit(x, x[:, 0], x[:, 0], o, [0, 4], strata=bad)
        with pytest.raises(TypeError, match="strata"):
            dlsa_amd.fit_cox_partitions(x, x[:, 0], x[:, 0], strata=bad)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int64)):
        with pytest.raises(ValueError, match="strata"):
            engine.cox_pass(x, x[:, 0], x[:, 0], o, x[0], strata=bad)
        with pytest.raises(ValueError, match="strata"):
            engine.cox_fit(x, x[:, 0], x[:, 0], o, [0, 4], strata=bad)
        with pytest.raises(ValueError, match="strata"):
            dlsa_amd.fit_cox_partitions(x, x[:, 0], x[:, 0], strata=bad)
    # the conversion to the C ABI's int32 (once, after the device check) refuses codes that would not survive it
    with pytest.raises(ValueError, match="int32"):
        engine.cox_strata_codes(torch.tensor([0, 1, 2 ** 40, 3]), torch.device("cpu"))
    c = engine.cox_strata_codes(torch.tensor([5, -2 ** 31, 2 ** 31 - 1, 5]), torch.device("cpu"))
    assert c.dtype == torch.int32 and c.tolist() == [5, -2 ** 31, 2 ** 31 - 1, 5]
    i32 = torch.tensor([1, 2], dtype=torch.int32)
    assert engine.cox_strata_codes(i32, torch.device("cpu")) is i32 and engine.cox_strata(i32, 2) is i32
    # the tie method is still checked first, and valid strata get as far as the device check
    with pytest.raises(ValueError, match="ties"):
        engine.cox_pass(x, x[:, 0], x[:, 0], o, x[0], ties="exact", strata=torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.cox_pass(x, x[:, 0], x[:, 0], o, x[0], strata=torch.zeros(4, dtype=torch.int64))
    df = pd.DataFrame({"time": [1.0, 2.0], "event": [1.0, 0.0], "x0": [0.5, 0.1], "clinic": [1, 2]})
    for bad in ("site", ["clinic", "site"], []):
        with pytest.raises(KeyError, match="strata"):
            dlsa_amd.cox_model(df, "time", "event", strata=bad)
    with pytest.raises(ValueError, match="strata"):
        dlsa_amd.simulate_cox(10, 2, 1, strata=0)
    # cox_order: (partition, stratum, -time)
    t = torch.tensor([1.0, 3.0, 2.0, 3.0, 1.0, 2.0])
    pid = torch.tensor([0, 0, 0, 1, 1, 1])
    s = torch.tensor([7, -1, 7, 2, 2, -5])
    assert models.cox_order(t, pid, s).tolist() == [1, 2, 0, 5, 3, 4]
    assert models.cox_order(t, pid).tolist() == [1, 2, 0, 3, 5, 4]
