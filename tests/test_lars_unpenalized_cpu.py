"""CPU: the LARS path with several unpenalised coefficients -- its reference (tests/lars_unpenalized_reference.py) against itself
and against the oracle's reference-pinned intercept branch, and the Python side against a recording fake library: what reaches
dlsa_lars_lsa_f64, the permutation, every refusal, the names helper and the header.  No GPU, no library."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import lars_certificate as lc
import lars_unpenalized_reference as ur
from dlsa_amd import _lib, engine, lsa, models
from oracle import dlsa_oracle as orc

dlsa_mod = importlib.import_module("dlsa_amd.dlsa")          # (the package's attribute `dlsa` is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("beta", "beta0", "theta", "AIC", "BIC")


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ur.PROBLEMS, ids=str)
def test_reference_agrees_with_its_longdouble_reduction(name):
    """float64 reduce against longdouble reduce, the same oracle path behind both: seen <= 2e-13 (bar 1e-12)"""
    r, rl = ur.problem_path(name), ur.problem_path(name, "longdouble")
    errs = {k: ur.rel(r[k], rl[k]) for k in KEYS}
    print(name, errs)
    assert all(v <= 1e-12 for v in errs.values()), errs


@pytest.mark.parametrize("name", ur.CORR_CASES, ids=str)
def test_reduced_lasso_paths_have_drops(name):
    r = ur.problem_path(("corr",) + name)
    steps, m = r["beta"].shape[0] - 1, r["beta"].shape[1]
    assert m == name[0] - 7 and steps > m, (steps, m)


@pytest.mark.parametrize("name", ur.PROBLEMS, ids=str)
def test_nested_identity(name):
    """Eliminating U[1:] on the host in longdouble and U[0] by the oracle's own intercept branch is the same path as eliminating
    all of U at once: seen <= 2e-15 on beta, AIC, BIC (bar 1e-12)."""
    S, b, n, U, typ = ur.problem(name)
    p = S.shape[0]
    keep = [U[0]] + ur.rest(p, U)                                   # the (m + 1)-problem: U[0] leads, the rest in their order
    order = sorted(keep)
    Sig, bR, _, R = ur.reduce(S, b, U[1:], np.longdouble)          # over sorted(keep)
    assert R == order
    at = [order.index(j) for j in keep]
    Sn = np.asarray(Sig, dtype=np.float64)[np.ix_(at, at)]
    bn = np.asarray(bR, dtype=np.float64)[at]
    ro = orc.lars_lsa(Sn, bn, True, n, type=typ)
    r = ur.problem_path(name, "longdouble")
    errs = {k: ur.rel(ro[k], r[k]) for k in ("beta", "AIC", "BIC")}
    print(name, errs)
    assert all(v <= 1e-12 for v in errs.values()), errs


@pytest.mark.parametrize("name", [("multinomial", 2, 6), ("corr", 127, 0.98, 12)], ids=str)
@pytest.mark.parametrize("which", [0, 3])
def test_one_unpenalised_is_the_oracles_intercept(name, which):
    S, b, n, U, typ = ur.problem(name)
    j = U[min(which, len(U) - 1)]
    perm = [j] + ur.rest(S.shape[0], [j])
    ro = orc.lars_lsa(S[np.ix_(perm, perm)], b[perm], True, n, type=typ)
    r = ur.path(S, b, [j], n, typ)
    errs = {"beta": ur.rel(r["beta"], ro["beta"]), "AIC": ur.rel(r["AIC"], ro["AIC"]), "BIC": ur.rel(r["BIC"], ro["BIC"]),
            "beta0": ur.rel(r["beta0"][:, 0], np.asarray(ro["beta0"]).ravel())}
    assert all(v <= 1e-12 for v in errs.values()), errs


@pytest.mark.parametrize("name", ur.PROBLEMS, ids=str)
def test_reference_passes_the_certificate(name):
    S, b, n, U, typ = ur.problem(name)
    Sig, bR, _, _ = ur.reduce(S, b, U)
    r = ur.problem_path(name)
    res = lc.certify(Sig, bR, False, n, typ, {k: r[k] for k in ("beta", "AIC", "BIC")})
    print(name, res)


# ---- marshalling against a recording fake ------------------------------------------------------------------------------------------
STREAM, WS_BYTES = 0x5EA0, 192


class FakeLib:
    def __init__(self):
        self.calls, self.ws_calls, self.ws = [], [], []

    def __getattr__(self, name):
        if not name.startswith("dlsa_"):
            raise AttributeError(name)
        if name.endswith("_workspace_bytes"):
            return lambda *a: (self.ws_calls.append((name, a)), WS_BYTES)[1]

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(engine, "_require_gpu", lambda *t: None)
    monkeypatch.setattr(engine, "_stream", lambda: ctypes.c_void_p(STREAM))

    def workspace(nbytes, device):
        lib.ws.append(torch.empty(int(nbytes), dtype=torch.uint8))
        return lib.ws[-1]
    monkeypatch.setattr(engine, "_workspace", workspace)
    return lib


def _problem(p=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand((4 * p, p), dtype=torch.float64, generator=g)
    return X.T @ X, torch.rand((p,), dtype=torch.float64, generator=g) + 0.1


@pytest.mark.parametrize("icpt,u", [(False, 0), (True, 1), (0, 0), (1, 1), (2, 2), (5, 5), (np.int64(3), 3)])
def test_count_reaches_the_fifth_integer_argument(fake, icpt, u):
    p, ms = 9, 11
    S, b = _problem(p)
    r = engine.lars_path(S, b, icpt, 100.0, type="lasso", max_steps=ms)
    (name, a), = fake.calls
    assert name == "dlsa_lars_lsa_f64" and len(a) == len(_lib.SIGNATURES[name][1])
    assert a[0].value == S.data_ptr() and a[1] == p and a[2].value == b.data_ptr()
    assert a[3] == p and type(a[4]) is int and a[4] == u and a[5] == 100.0 and a[6] == 1 and a[8] == ms
    # the call returned n_steps = 0: one row of each output, views of the buffers handed over
    assert a[9].value == r["beta"].data_ptr() and a[10].value == r["beta0"].data_ptr()
    assert r["beta"].shape == (1, p - u)
    assert r["beta0"].shape == ((1,) if u <= 1 else (1, u))
    base = r["beta0"]._base if r["beta0"]._base is not None else r["beta0"]
    assert base.numel() == (ms + 1) * max(1, u) and base.is_contiguous()
    assert (r["beta"]._base if r["beta"]._base is not None else r["beta"]).numel() == (ms + 1) * (p - u)
    assert fake.ws_calls == [("dlsa_lars_workspace_bytes", (p,))]


def test_default_max_steps_follows_the_penalised_width(fake):
    S, b = _problem(9)
    r = engine.lars_path(S, b, 4, 100.0)
    a = fake.calls[0][1]
    assert a[8] == 8 * 5 and r["beta0"]._base.shape == (8 * 5 + 1, 4)


def test_wrapper_hands_over_the_permuted_problem(fake, monkeypatch):
    p, U = 9, [7, 2, 5]
    S, b = _problem(p)
    seen = {}
    real = engine.lars_path

    def spy(Sp, bp, u, n, **kw):
        seen.update(S=Sp.clone(), b=bp.clone(), u=u, contiguous=Sp.is_contiguous() and bp.is_contiguous())
        return real(Sp, bp, u, n, **kw)
    monkeypatch.setattr(engine, "lars_path", spy)
    monkeypatch.setattr(lsa, "_dev", lambda a: torch.as_tensor(a, dtype=torch.float64).contiguous())
    r = lsa.lars_path_device(S, b, False, 50.0, unpenalized=U, max_steps=3)
    perm = U + [j for j in range(p) if j not in U]
    assert perm == [7, 2, 5, 0, 1, 3, 4, 6, 8]
    assert seen["u"] == 3 and type(seen["u"]) is int and seen["contiguous"]
    assert torch.equal(seen["S"], S[perm][:, perm]) and torch.equal(seen["b"], b[perm])
    assert fake.calls[0][1][4] == 3
    # the fake wrote nothing: beta = 0, beta0 = 0, so theta is b at U and zero elsewhere, in the caller's order
    assert list(r) == ["AIC", "BIC", "beta", "beta0", "theta"]
    assert r["beta"].shape == (1, p - 3) and r["beta0"].shape == (1, 3) and r["theta"].shape == (1, p)
    want = torch.zeros(p, dtype=torch.float64)
    want[U] = b[U]
    assert torch.equal(r["theta"][0], want)


def test_wrapper_scatter_puts_every_coefficient_back(monkeypatch):
    """theta from a made-up engine result: beta over the rest in their original order, b0[U] + beta0 at U in the order given"""
    p, U = 6, [4, 1]
    S, b = _problem(p)
    monkeypatch.setattr(lsa, "_dev", lambda a: torch.as_tensor(a, dtype=torch.float64).contiguous())
    beta = torch.arange(1.0, 9.0, dtype=torch.float64).reshape(2, 4)
    beta0 = torch.tensor([[10.0, 20.0], [30.0, 40.0]], dtype=torch.float64)
    monkeypatch.setattr(engine, "lars_path", lambda *a, **k: {"AIC": torch.zeros(2), "BIC": torch.zeros(2), "beta": beta, "beta0": beta0})
    r = lsa.lars_path_device(S, b, False, 50.0, unpenalized=U)
    want = torch.tensor([[1.0, float(b[1]) + 20.0, 2.0, 3.0, float(b[4]) + 10.0, 4.0],
                         [5.0, float(b[1]) + 40.0, 6.0, 7.0, float(b[4]) + 30.0, 8.0]], dtype=torch.float64)
    assert torch.equal(r["theta"], want) and torch.equal(r["beta0"], beta0)


def test_one_index_gives_a_column_of_beta0(fake, monkeypatch):
    monkeypatch.setattr(lsa, "_dev", lambda a: torch.as_tensor(a, dtype=torch.float64).contiguous())
    S, b = _problem(5)
    r = lsa.lars_path_device(S, b, False, 50.0, unpenalized=[3], max_steps=2)
    assert fake.calls[0][1][4] == 1 and r["beta0"].shape == (1, 1) and r["beta"].shape == (1, 4)
    fake.calls.clear()
    r = lsa.lars_path_device(S, b, False, 50.0, unpenalized=[], max_steps=2)
    assert fake.calls[0][1][4] == 0 and r["beta0"].shape == (1, 0) and r["beta"].shape == (1, 5)


# ---- refusals: before any GPU work -------------------------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was reached")
    monkeypatch.setattr(lsa, "_dev", boom)
    monkeypatch.setattr(engine, "lars_path", boom)
    monkeypatch.setattr(_lib, "load", boom)


BAD_SETS = {"with intercept=True": ([1, 2], True), "duplicates": ([1, 2, 1], False), "past the end": ([1, 40], False),
            "negative": ([-1, 2], False), "not whole": ([1.5], False), "over the cap": (list(range(33)), False),
            "everything": (list(range(40)), False)}


@pytest.mark.parametrize("case", sorted(BAD_SETS))
def test_wrapper_refusals(no_gpu, case):
    U, icpt = BAD_SETS[case]
    S, b = np.eye(40), np.ones(40)
    if case == "everything":
        S, b, U = np.eye(3), np.ones(3), [0, 1, 2]
    for call in (lsa.lars_path_device, lsa.lars_lsa):
        with pytest.raises(ValueError):
            call(S, b, icpt, 10.0, unpenalized=U)
    with pytest.raises(ValueError):
        dlsa_mod.dlsa(S, b, 10.0, fit_intercept=icpt, unpenalized=U)


def test_cap_is_accepted_at_32(monkeypatch):
    got = {}
    monkeypatch.setattr(lsa, "_dev", lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).contiguous())
    monkeypatch.setattr(engine, "lars_path", lambda Sp, bp, u, n, **k: got.update(u=u) or
                        {"AIC": torch.zeros(1), "BIC": torch.zeros(1), "beta": torch.zeros((1, 8), dtype=torch.float64),
                         "beta0": torch.zeros((1, 32), dtype=torch.float64)})
    lsa.lars_path_device(np.eye(40), np.ones(40), False, 10.0, unpenalized=list(range(32)))
    assert got["u"] == 32


@pytest.mark.parametrize("icpt", [-1, 33, 9, 12, 1.5])
def test_engine_refusals(fake, icpt):
    S, b = _problem(9)
    with pytest.raises(ValueError):
        engine.lars_path(S, b, icpt, 10.0)
    assert fake.calls == []


def test_dlsa_name_refusals(no_gpu):
    import pandas as pd
    S = pd.DataFrame(np.eye(4), columns=["intercept:1", "x0:1", "intercept:2", "x0:2"])
    b = np.ones(4)
    with pytest.raises(ValueError, match="intercepts"):
        dlsa_mod.dlsa(S, b, 10.0, unpenalized="intercept")               # a string that is not "intercepts"
    with pytest.raises(ValueError, match="column names"):
        dlsa_mod.dlsa(S.to_numpy(), b, 10.0, unpenalized="intercepts")
    with pytest.raises(ValueError, match="column names"):
        dlsa_mod.dlsa(S.to_numpy(), b, 10.0, unpenalized=["x0:1"])
    with pytest.raises(ValueError, match="0 columns"):
        dlsa_mod.dlsa(S, b, 10.0, unpenalized=["x9"])
    with pytest.raises(ValueError):
        dlsa_mod.dlsa(S, b, 10.0, fit_intercept=True, unpenalized="intercepts")


def test_dlsa_resolves_names_and_keeps_the_frame(monkeypatch):
    import pandas as pd
    names = ["intercept:1", "x0:1", "intercept:2", "x0:2"]
    S = pd.DataFrame(np.eye(4), columns=names)
    seen = {}

    def path(S_, b_, icpt, n, type="lar", unpenalized=None):
        seen.update(U=list(unpenalized), icpt=icpt, type=type)
        theta = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]], dtype=torch.float64)
        return {"AIC": torch.tensor([3.0, 1.0, 2.0]), "BIC": torch.tensor([3.0, 2.0, 1.0]), "theta": theta}
    monkeypatch.setattr(dlsa_mod, "lars_path_device", path)
    out = dlsa_mod.dlsa(S, np.ones(4), 10.0, unpenalized="intercepts", type="lasso")
    assert seen == {"U": [0, 2], "icpt": False, "type": "lasso"}
    assert list(out.columns) == ["beta_byAIC", "beta_byBIC"] and out.shape == (4, 2)
    assert list(out["beta_byAIC"]) == [1.0, 2.0, 3.0, 4.0] and list(out["beta_byBIC"]) == [5.0, 6.0, 7.0, 8.0]
    dlsa_mod.dlsa(S, np.ones(4), 10.0, unpenalized=["x0:2", 0])
    assert seen["U"] == [3, 0]


def test_intercept_columns():
    import dlsa_amd
    assert dlsa_amd.intercept_columns is models.intercept_columns
    assert models.intercept_columns(["intercept", "x0", "x1"]) == [0]
    assert models.intercept_columns(["x0", "x1"]) == []
    names = models.multinomial_column_names(["intercept", "a", "b"], 4)
    assert names[0] == "intercept:1" and models.intercept_columns(names) == [0, 3, 6]
    assert models.intercept_columns(["a:1", "intercept:12", "intercepts", "intercept:x", "intercept:", "my_intercept", "intercept"]) == [1, 6]


# ---- the header ---------------------------------------------------------------------------------------------------------------------
# the C ABI's entries as they were before this feature: it rides dlsa_lars_lsa_f64's `int intercept`
SIGNATURES_BEFORE = 111


def test_header_defines_the_cap_and_declares_no_new_entry():
    text = open(os.path.join(ROOT, "include", "dlsa_hip.h")).read()
    m = re.search(r"^#define\s+DLSA_LARS_MAX_UNPENALIZED\s+(\d+)\s*$", text, re.M)
    assert m and int(m.group(1)) == engine.LARS_MAX_UNPENALIZED == 32
    lars = [name for name in _lib.SIGNATURES if "lars" in name]
    assert sorted(lars) == ["dlsa_lars_grid_barrier_timeout", "dlsa_lars_lsa_f64", "dlsa_lars_workspace_bytes"]
    assert len(_lib.SIGNATURES) == SIGNATURES_BEFORE
    assert len(re.findall(r"\bdlsa_lars_\w+\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))) == 3
