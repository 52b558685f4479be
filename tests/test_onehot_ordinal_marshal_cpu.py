"""CPU: what engine.onehot_ordinal_pass and engine.onehot_ordinal_fit_ex hand to the C ABI of include/dlsa_hip_onehot_ordinal.h,
against the recording fake library of test_engine_marshal_cpu.py: the symbol, the plan handle and the raw rows with their pitches,
every scalar at its position and with its type, every pointer against the tensor it stands for, the output shapes J + p and
(J + p)^2, the workspace query, the host arrays of length K, strided partitions and the refusals made before any call."""
import pytest
import torch

from dlsa_amd import _lib, engine, models
from test_engine_marshal_cpu import (HOST3, I64, K, N, OUT3, PARTS, PLAN_P, TAIL, arr, check_call, check_fit_result, fake, out, ptr,  # noqa: F401
                                     raw, raw_spec, rows, val)


@pytest.fixture
def ofake(fake, monkeypatch):     # noqa: F811
    """check_call looks the argument count up in _lib.SIGNATURES: for this file that table also holds the extension's entries"""
    monkeypatch.setattr(_lib, "SIGNATURES", {**_lib.SIGNATURES, **_lib.ONEHOT_ORDINAL_SIGNATURES})
    return fake


@pytest.mark.parametrize("with_num", [True, False])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("classes", [2, 3, 8])
def test_onehot_ordinal_fit_ex(ofake, step, classes, with_num):
    plan, num, codes = raw(with_num)
    _, y, _ = rows()
    first, nrows = PARTS[step]
    r = engine.onehot_ordinal_fit_ex(plan, num, codes, y, first, nrows, row_step=step, classes=classes, tol=1e-9, max_iter=17)
    d = classes - 1 + PLAN_P
    check_fit_result(r, d)
    assert r["rc"] == 0
    check_call(ofake, "dlsa_onehot_ordinal_fit_f64",
               raw_spec(num, codes) + [ptr(y), arr(I64, first), arr(I64, nrows), val(step), val(K), val(classes), val(1e-9), val(17)]
               + OUT3 + HOST3 + TAIL, r)
    assert len(ofake.calls[0][1]) == 22
    assert ofake.ws_calls[0][0] == "dlsa_onehot_ordinal_workspace_bytes" and ofake.ws_calls[0][1][1:] == (4, classes, step)
    assert ofake.ws_calls[0][1][0] is plan._h and len(ofake.ws_calls) == 1


def test_onehot_ordinal_fit_ex_defaults_and_refusals(ofake):
    plan, num, codes = raw()
    _, y, _ = rows()
    engine.onehot_ordinal_fit_ex(plan, num, codes, y, *PARTS[1], classes=3)
    a = ofake.calls[0][1]
    assert a[8:13] == (1, K, 3, 1e-13, 100)
    ofake.calls.clear()
    with pytest.raises(ValueError, match="classes .* is required"):
        engine.onehot_ordinal_fit_ex(plan, num, codes, y, *PARTS[1])
    for bad in (1, 9):
        with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
            engine.onehot_ordinal_fit_ex(plan, num, codes, y, *PARTS[1], classes=bad)
    with pytest.raises(ValueError, match="must have the same n = 5 rows"):
        engine.onehot_ordinal_fit_ex(plan, num, codes, y[:5], *PARTS[1], classes=3)
    with pytest.raises(TypeError, match="y must be torch.float64"):
        engine.onehot_ordinal_fit_ex(plan, num, codes, y.to(torch.int64), *PARTS[1], classes=3)
    with pytest.raises(ValueError, match="codes must be int32"):
        engine.onehot_ordinal_fit_ex(plan, num, codes.to(torch.int64), y, *PARTS[1], classes=3)
    with pytest.raises(ValueError, match="partition outside the 7 rows"):
        engine.onehot_ordinal_fit_ex(plan, num, codes, y, [0, 1], [4, 4], row_step=2, classes=3)
    assert ofake.calls == []


@pytest.mark.parametrize("classes", [2, 4])
@pytest.mark.parametrize("want_H", [False, True])
@pytest.mark.parametrize("want_w", [False, True])
def test_onehot_ordinal_pass(ofake, classes, want_H, want_w):
    plan, num, codes = raw()
    _, y, _ = rows()
    d = classes - 1 + PLAN_P
    theta = torch.zeros(d, dtype=torch.float64)
    H, g, ll, w = engine.onehot_ordinal_pass(plan, num, codes, y, theta, classes, want_H=want_H, want_w=want_w)
    assert (H is not None) == want_H and (w is not None) == want_w
    assert tuple(g.shape) == (d,) and tuple(ll.shape) == (1,) and g.dtype == ll.dtype == torch.float64
    if want_H:
        assert tuple(H.shape) == (d, d) and H.is_contiguous()
    if want_w:
        assert tuple(w.shape) == (N,)
    r = {"H": H, "g": g, "ll": ll, "w": w}
    check_call(ofake, "dlsa_onehot_ordinal_pass_f64",
               raw_spec(num, codes) + [ptr(y), ptr(theta), val(classes), val(N), out("H"), val(d), out("g"), out("ll"), out("w")] + TAIL, r)
    assert len(ofake.calls[0][1]) == 17
    assert ofake.ws_calls[0][0] == "dlsa_onehot_ordinal_workspace_bytes" and ofake.ws_calls[0][1][1:] == (N, classes, 1)


def test_onehot_ordinal_pass_refusals(ofake):
    plan, num, codes = raw()
    _, y, _ = rows()
    with pytest.raises(ValueError, match="theta with 7 elements"):
        engine.onehot_ordinal_pass(plan, num, codes, y, torch.zeros(6, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
        engine.onehot_ordinal_pass(plan, num, codes, y, torch.zeros(5, dtype=torch.float64), 1)
    with pytest.raises(TypeError, match="theta must be torch.float64"):
        engine.onehot_ordinal_pass(plan, num, codes, y, torch.zeros(7, dtype=torch.float32), 3)
    with pytest.raises(ValueError, match="must have the same n = 7 rows"):
        engine.onehot_ordinal_pass(plan, num[:5], codes, y, torch.zeros(7, dtype=torch.float64), 3)
    assert ofake.calls == []


def test_the_package_exports_the_design_fit():
    import dlsa_amd
    assert dlsa_amd.fit_ordinal_design is models.fit_ordinal_design
