"""CPU: what engine.ordinal_pass and engine.ordinal_fit_ex hand to the C ABI of include/dlsa_hip_ordinal.h, against the recording
fake library of test_engine_marshal_cpu.py: the symbol, every scalar at its position and with its type, every pointer against the
tensor it stands for, the output shapes J + p and (J + p)^2, the workspace query, the host arrays of length K, strided partitions
and the refusals made before any call.  models.fit_ordinal_partitions on top of it: partitions, names, the MappedBlocks."""
import pytest
import torch

from dlsa_amd import _lib, engine, models
from test_engine_marshal_cpu import (HOST3, I64, K, N, OUT3, P, PARTS, TAIL, arr, check_call, check_fit_result, fake, out, ptr,  # noqa: F401
                                     rows, val)


@pytest.fixture
def ofake(fake, monkeypatch):     # noqa: F811
    """check_call looks the argument count up in _lib.SIGNATURES: for this file that table also holds the extension's entries"""
    monkeypatch.setattr(_lib, "SIGNATURES", {**_lib.SIGNATURES, **_lib.ORDINAL_SIGNATURES})
    return fake


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("classes", [2, 3, 8])
def test_ordinal_fit_ex(ofake, step, classes):
    X, y, _ = rows()
    first, nrows = PARTS[step]
    r = engine.ordinal_fit_ex(X, y, first, nrows, row_step=step, classes=classes, tol=1e-9, max_iter=17)
    d = classes - 1 + P
    check_fit_result(r, d)
    assert r["rc"] == 0
    check_call(ofake, "dlsa_ordinal_fit_f64",
               [ptr(X), val(4), ptr(y), arr(I64, first), arr(I64, nrows), val(step), val(K), val(P), val(classes), val(1e-9), val(17)]
               + OUT3 + HOST3 + TAIL, r)
    assert len(ofake.calls[0][1]) == 20
    assert ofake.ws_calls == [("dlsa_ordinal_workspace_bytes", (4, P, classes, step))]


def test_ordinal_fit_ex_defaults_and_refusals(ofake):
    X, y, _ = rows()
    engine.ordinal_fit_ex(X, y, *PARTS[1], classes=3)
    a = ofake.calls[0][1]
    assert a[5:11] == (1, K, P, 3, 1e-13, 100)
    ofake.calls.clear()
    with pytest.raises(ValueError, match="classes .* is required"):
        engine.ordinal_fit_ex(X, y, *PARTS[1])
    for bad in (1, 9):
        with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
            engine.ordinal_fit_ex(X, y, *PARTS[1], classes=bad)
    with pytest.raises(ValueError, match="y must have n = 7 elements"):
        engine.ordinal_fit_ex(X, y[:5], *PARTS[1], classes=3)
    with pytest.raises(TypeError, match="y must be torch.float64"):
        engine.ordinal_fit_ex(X, y.to(torch.int64), *PARTS[1], classes=3)
    with pytest.raises(ValueError, match="partition outside the 7 rows"):
        engine.ordinal_fit_ex(X, y, [0, 1], [4, 4], row_step=2, classes=3)
    assert ofake.calls == []


@pytest.mark.parametrize("classes", [2, 4])
@pytest.mark.parametrize("want_H", [False, True])
@pytest.mark.parametrize("want_w", [False, True])
def test_ordinal_pass(ofake, classes, want_H, want_w):
    X, y, _ = rows()
    d = classes - 1 + P
    theta = torch.zeros(d, dtype=torch.float64)
    H, g, ll, w = engine.ordinal_pass(X, y, theta, classes, want_H=want_H, want_w=want_w)
    assert (H is not None) == want_H and (w is not None) == want_w
    assert tuple(g.shape) == (d,) and tuple(ll.shape) == (1,) and g.dtype == ll.dtype == torch.float64
    if want_H:
        assert tuple(H.shape) == (d, d) and H.is_contiguous()
    if want_w:
        assert tuple(w.shape) == (N,)
    r = {"H": H, "g": g, "ll": ll, "w": w}
    check_call(ofake, "dlsa_ordinal_pass_f64",
               [ptr(X), val(4), ptr(y), ptr(theta), val(classes), val(N), val(P), out("H"), val(d), out("g"), out("ll"), out("w")] + TAIL, r)
    assert len(ofake.calls[0][1]) == 15
    assert ofake.ws_calls == [("dlsa_ordinal_workspace_bytes", (N, P, classes, 1))]


def test_ordinal_pass_refusals(ofake):
    X, y, _ = rows()
    with pytest.raises(ValueError, match="theta with 5 elements"):
        engine.ordinal_pass(X, y, torch.zeros(6, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
        engine.ordinal_pass(X, y, torch.zeros(3, dtype=torch.float64), 1)
    with pytest.raises(TypeError, match="theta must be torch.float64"):
        engine.ordinal_pass(X, y, torch.zeros(5, dtype=torch.float32), 3)
    assert ofake.calls == []


def test_blocks_names_and_partitions(ofake):
    """the pieces fit_ordinal_partitions is made of (the function itself refuses a CPU tensor): i % 2 partitions, the J + p names with
    the cutpoints first, the MappedBlocks of the engine's result"""
    X, y, _ = rows()
    first, nrows, step = models._partitions(N, 2, None)
    r = engine.ordinal_fit_ex(X, y, first, nrows, row_step=step, classes=3)
    names = models.ordinal_column_names(models._column_names(["a", "b", "c"], P, False), 3)
    assert names == ["intercept:1", "intercept:2", "a", "b", "c"] and models.intercept_columns(names) == [0, 1]
    assert models.ordinal_column_names(models._column_names(None, P, False), 2) == ["intercept:1", "x0", "x1", "x2"]
    mb = models._blocks(r, names, N)
    assert tuple(mb.coef.shape) == (2, len(names)) and tuple(mb.Sig_inv.shape) == (2, len(names), len(names))
    a = ofake.calls[0][1]
    assert list(a[3]) == [0, 1] and list(a[4]) == [4, 3] and a[5:9] == (2, 2, P, 3)
    assert mb.columns == ["par_id", "coef", "Sig_invMcoef"] + names
    with pytest.raises(RuntimeError, match="GPU only"):
        models.fit_ordinal_partitions(X, y, 3, partition_num=2)


def test_the_package_exports_the_family():
    import dlsa_amd
    for name in ("fit_ordinal_partitions", "ordinal_column_names", "ordinal_model", "ordinal_model_eval", "simulate_ordinal"):
        assert getattr(dlsa_amd, name) is getattr(models, name)
