"""CPU: what engine.multinomial_pass and engine.multinomial_fit_ex hand to the C ABI, against the recording fake library of
test_engine_marshal_cpu.py: the symbol, every scalar at its position and with its type, every pointer against the tensor it stands
for, the output shapes J * pe and (J * pe)^2, the workspace query, the host arrays of length K and the refusals made before any
call.  models.fit_multinomial_partitions on top of it: partitions, names, the MappedBlocks."""
import pytest
import torch

from dlsa_amd import engine, models
from test_engine_marshal_cpu import (CD, CI, HOST3, I64, K, N, OUT3, P, PARTS, TAIL, arr, check_call, check_fit_result, fake, out, ptr,  # noqa: F401
                                     rows, val)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("classes", [2, 3, 8])
def test_multinomial_fit_ex(fake, step, icpt, classes):     # noqa: F811
    X, y, _ = rows()
    first, nrows = PARTS[step]
    r = engine.multinomial_fit_ex(X, y, first, nrows, row_step=step, classes=classes, fit_intercept=icpt, tol=1e-9, max_iter=17)
    d = (classes - 1) * (P + int(icpt))
    check_fit_result(r, d)
    assert r["rc"] == 0
    check_call(fake, "dlsa_multinomial_fit_f64",
               [ptr(X), val(4), ptr(y), arr(I64, first), arr(I64, nrows), val(step), val(K), val(P), val(int(icpt)), val(classes),
                val(1e-9), val(17)] + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls == [("dlsa_multinomial_workspace_bytes", (4, P, int(icpt), classes, step))]


def test_multinomial_fit_ex_defaults_and_refusals(fake):     # noqa: F811
    X, y, _ = rows()
    engine.multinomial_fit_ex(X, y, *PARTS[1], classes=3)
    a = fake.calls[0][1]
    assert a[5:12] == (1, K, P, 0, 3, 1e-13, 100)
    fake.calls.clear()
    with pytest.raises(ValueError, match="classes .* is required"):
        engine.multinomial_fit_ex(X, y, *PARTS[1])
    for bad in (1, 9):
        with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
            engine.multinomial_fit_ex(X, y, *PARTS[1], classes=bad)
    with pytest.raises(ValueError, match="y must have n = 7 elements"):
        engine.multinomial_fit_ex(X, y[:5], *PARTS[1], classes=3)
    with pytest.raises(TypeError, match="y must be torch.float64"):
        engine.multinomial_fit_ex(X, y.to(torch.int64), *PARTS[1], classes=3)
    assert fake.calls == []


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("classes", [2, 4])
@pytest.mark.parametrize("want_H", [False, True])
@pytest.mark.parametrize("want_prob", [False, True])
def test_multinomial_pass(fake, icpt, classes, want_H, want_prob):     # noqa: F811
    X, y, _ = rows()
    J = classes - 1
    d = J * (P + int(icpt))
    theta = torch.zeros(d, dtype=torch.float64)
    H, g, ll, prob = engine.multinomial_pass(X, y, theta, classes, fit_intercept=icpt, want_H=want_H, want_prob=want_prob)
    assert (H is not None) == want_H and (prob is not None) == want_prob
    assert tuple(g.shape) == (d,) and tuple(ll.shape) == (1,) and g.dtype == ll.dtype == torch.float64
    if want_H:
        assert tuple(H.shape) == (d, d) and H.is_contiguous()
    if want_prob:                              # [J, n], a view of class rows with a pitch of 32 doubles (256 bytes)
        assert tuple(prob.shape) == (J, N) and prob.stride() == (32, 1)
    r = {"H": H, "g": g, "ll": ll, "prob": prob}
    check_call(fake, "dlsa_multinomial_pass_f64",
               [ptr(X), val(4), ptr(y), ptr(theta), val(classes), val(N), val(P), val(int(icpt)), out("H"), val(d), out("g"), out("ll"),
                out("prob"), val(32)] + TAIL, r)
    assert fake.ws_calls == [("dlsa_multinomial_workspace_bytes", (N, P, int(icpt), classes, 1))]


def test_multinomial_pass_refusals(fake):     # noqa: F811
    X, y, _ = rows()
    with pytest.raises(ValueError, match="theta with 6 elements"):
        engine.multinomial_pass(X, y, torch.zeros(5, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="classes must lie in 2 .. 8"):
        engine.multinomial_pass(X, y, torch.zeros(3, dtype=torch.float64), 1)
    with pytest.raises(TypeError, match="theta must be torch.float64"):
        engine.multinomial_pass(X, y, torch.zeros(6, dtype=torch.float32), 3)
    assert fake.calls == []


@pytest.mark.parametrize("icpt", [False, True])
def test_blocks_names_and_partitions(fake, icpt):     # noqa: F811
    """the pieces fit_multinomial_partitions is made of (the function itself refuses a CPU tensor): i % 2 partitions, the J * pe
    names, the MappedBlocks of the engine's result"""
    X, y, _ = rows()
    first, nrows, step = models._partitions(N, 2, None)
    r = engine.multinomial_fit_ex(X, y, first, nrows, row_step=step, classes=3, fit_intercept=icpt)
    base = models._column_names(["a", "b", "c"], P, icpt)
    names = models.multinomial_column_names(base, 3)
    assert names == [nm + ":1" for nm in base] + [nm + ":2" for nm in base] and names[0] == ("intercept:1" if icpt else "a:1")
    mb = models._blocks(r, names, N)
    assert tuple(mb.coef.shape) == (2, len(names)) and tuple(mb.Sig_inv.shape) == (2, len(names), len(names))
    a = fake.calls[0][1]
    assert list(a[3]) == [0, 1] and list(a[4]) == [4, 3] and a[5:10] == (2, 2, P, int(icpt), 3)
    assert mb.columns == ["par_id", "coef", "Sig_invMcoef"] + names
    with pytest.raises(RuntimeError, match="GPU only"):
        models.fit_multinomial_partitions(X, y, 3, partition_num=2)
