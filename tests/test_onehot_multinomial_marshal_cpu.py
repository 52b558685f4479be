"""CPU: what engine.onehot_multinomial_pass and engine.onehot_multinomial_fit_ex hand to the C ABI, against the recording fake
library of test_engine_marshal_cpu.py: the symbol, the plan handle, every scalar at its position and with its type, every pointer
against the tensor it stands for (num absent or present, the row pitches of num and codes), strided and offset partitions, the
output shapes J * p and (J * p)^2, want_H / want_prob, the workspace query and the refusals made before any call."""
import pytest
import torch

from dlsa_amd import engine, models
from test_engine_marshal_cpu import (CD, CI, HOST3, I64, K, N, OFFS, OUT3, PARTS, PLAN_P, TAIL, arr, check_call, check_fit_result, fake,  # noqa: F401
                                     out, ptr, raw, raw_spec, rows, val)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("with_num", [False, True])
@pytest.mark.parametrize("classes", [2, 3, 8])
def test_onehot_multinomial_fit_ex(fake, step, with_num, classes):     # noqa: F811
    plan, num, codes = raw(with_num)
    _, y, _ = rows()
    first, nrows = PARTS[step]
    r = engine.onehot_multinomial_fit_ex(plan, num, codes, y, first, nrows, row_step=step, classes=classes, tol=1e-9, max_iter=17)
    d = (classes - 1) * PLAN_P
    check_fit_result(r, d)
    assert r["rc"] == 0
    check_call(fake, "dlsa_onehot_multinomial_fit_f64",
               raw_spec(num, codes) + [ptr(y), arr(I64, first), arr(I64, nrows), val(step), val(K), val(classes), val(1e-9), val(17)]
               + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_multinomial_workspace_bytes" and fake.ws_calls[0][1][1:] == (4, classes, step)
    assert fake.ws_calls[0][1][0] is plan._h and len(fake.ws_calls) == 1


def test_onehot_multinomial_fit_ex_offset_partitions(fake):     # noqa: F811
    """contiguous partitions given by offsets, as models._partitions turns them into (first, rows, step = 1)"""
    plan, num, codes = raw()
    _, y, _ = rows()
    first, nrows, step = models._partitions(N, None, OFFS)
    r = engine.onehot_multinomial_fit_ex(plan, num, codes, y, first, nrows, row_step=step, classes=3)
    check_fit_result(r, 2 * PLAN_P)
    a = fake.calls[0][1]
    assert list(a[6]) == OFFS[:-1] and list(a[7]) == [OFFS[k + 1] - OFFS[k] for k in range(K)] and a[8:13] == (1, K, 3, 1e-13, 100)
    assert fake.ws_calls[0][1][1:] == (max(nrows), 3, 1)


def test_onehot_multinomial_fit_ex_refusals(fake):     # noqa: F811
    plan, num, codes = raw()
    _, y, _ = rows()
    with pytest.raises(ValueError, match="classes .* is required"):
        engine.onehot_multinomial_fit_ex(plan, num, codes, y, *PARTS[1])
    for bad in (1, 9):
        with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
            engine.onehot_multinomial_fit_ex(plan, num, codes, y, *PARTS[1], classes=bad)
    with pytest.raises(ValueError, match="same n = 5 rows"):
        engine.onehot_multinomial_fit_ex(plan, num, codes, y[:5], *PARTS[1], classes=3)
    with pytest.raises(TypeError, match="y must be torch.float64"):
        engine.onehot_multinomial_fit_ex(plan, num, codes, y.to(torch.int64), *PARTS[1], classes=3)
    with pytest.raises(ValueError, match="partition outside the 7 rows"):
        engine.onehot_multinomial_fit_ex(plan, num, codes, y, [0, 4], [4, 4], classes=3)
    with pytest.raises(ValueError, match="codes must be int32"):
        engine.onehot_multinomial_fit_ex(plan, num, codes.to(torch.int64), y, *PARTS[1], classes=3)
    wide = type(plan)(_h=plan._h, p=300)
    with pytest.raises(ValueError, match="exceed the solver's 2048"):
        engine.onehot_multinomial_fit_ex(wide, num, codes, y, *PARTS[1], classes=8)
    assert fake.calls == []


@pytest.mark.parametrize("with_num", [False, True])
@pytest.mark.parametrize("classes", [2, 4])
@pytest.mark.parametrize("want_H", [False, True])
@pytest.mark.parametrize("want_prob", [False, True])
def test_onehot_multinomial_pass(fake, with_num, classes, want_H, want_prob):     # noqa: F811
    plan, num, codes = raw(with_num)
    _, y, _ = rows()
    J = classes - 1
    d = J * PLAN_P
    theta = torch.zeros(d, dtype=torch.float64)
    H, g, ll, prob = engine.onehot_multinomial_pass(plan, num, codes, y, theta, classes, want_H=want_H, want_prob=want_prob)
    assert (H is not None) == want_H and (prob is not None) == want_prob
    assert tuple(g.shape) == (d,) and tuple(ll.shape) == (1,) and g.dtype == ll.dtype == torch.float64
    if want_H:
        assert tuple(H.shape) == (d, d) and H.is_contiguous()
    if want_prob:                              # [J, n], a view of class rows with a pitch of 32 doubles (256 bytes)
        assert tuple(prob.shape) == (J, N) and prob.stride() == (32, 1)
    r = {"H": H, "g": g, "ll": ll, "prob": prob}
    check_call(fake, "dlsa_onehot_multinomial_pass_f64",
               raw_spec(num, codes) + [ptr(y), ptr(theta), val(classes), val(N), out("H"), val(d), out("g"), out("ll"), out("prob"), val(32)]
               + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_multinomial_workspace_bytes" and fake.ws_calls[0][1][1:] == (N, classes, 1)


def test_onehot_multinomial_pass_refusals(fake):     # noqa: F811
    plan, num, codes = raw()
    _, y, _ = rows()
    with pytest.raises(ValueError, match="theta with 10 elements"):
        engine.onehot_multinomial_pass(plan, num, codes, y, torch.zeros(9, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
        engine.onehot_multinomial_pass(plan, num, codes, y, torch.zeros(5, dtype=torch.float64), 1)
    with pytest.raises(TypeError, match="theta must be torch.float64"):
        engine.onehot_multinomial_pass(plan, num, codes, y, torch.zeros(10, dtype=torch.float32), 3)
    with pytest.raises(ValueError, match="same n = 7 rows"):
        engine.onehot_multinomial_pass(plan, num[:5], codes, y, torch.zeros(10, dtype=torch.float64), 3)
    assert fake.calls == []
