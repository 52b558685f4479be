"""CPU: what the nine fit wrappers and five pass wrappers of dlsa_amd/engine.py hand to the C ABI, with no GPU and no library.
_lib.load returns a recording fake, engine._require_gpu / _stream / _workspace are replaced, and the wrappers run on CPU tensors:
the symbol called, every scalar at its position, every pointer against the data_ptr() of the tensor it stands for, the partition
arrays, the result dict, the soft-failure codes and the partition checks.  The fake writes distinct numbers into every host output
array, so a result list that came from the wrong array shows.  The models.py partition / names helpers are tested at the end."""
import ctypes
import types

import pytest
import torch

from dlsa_amd import _lib, engine, models

N, P, K = 7, 3, 2
STREAM = 0x5EA0
WS_BYTES = 192
PLAN_H = 0x7000
PLAN_P = 5
# (first, rows) of the K = 2 partitions of the N = 7 rows: contiguous halves, and partition_id = i % 2
PARTS = {1: ([0, 3], [3, 4]), 2: ([0, 1], [4, 3])}
OFFS = [0, 3, 7]


class FakeLib:
    """Stands for libdlsa_hip.so: every dlsa_* attribute records (name, args) and returns `rc`; *_workspace_bytes reports a small
    constant (recorded apart); host output arrays (int / double, not the int64 partition arrays) are filled with 100 * position + k."""

    def __init__(self, rc=0):
        self.rc, self.calls, self.ws_calls = rc, [], []

    def __getattr__(self, name):
        if not name.startswith("dlsa_"):
            raise AttributeError(name)
        if name.endswith("_workspace_bytes"):
            return lambda *a: (self.ws_calls.append((name, a)), WS_BYTES)[1]
        if name == "dlsa_last_error":
            def last_error(buf, size):
                buf.value = b"fake failure"
                return 0
            return last_error

        def fn(*args):
            self.calls.append((name, args))
            for i, a in enumerate(args):
                if isinstance(a, ctypes.Array) and a._type_ in (ctypes.c_int, ctypes.c_double):
                    for k in range(len(a)):
                        a[k] = 100 * i + k
            return self.rc
        return fn


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    lib.ws = []
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(engine, "_require_gpu", lambda *t: None)
    monkeypatch.setattr(engine, "_stream", lambda: ctypes.c_void_p(STREAM))

    def workspace(nbytes, device):
        lib.ws.append(torch.empty(int(nbytes), dtype=torch.uint8))
        return lib.ws[-1]
    monkeypatch.setattr(engine, "_workspace", workspace)
    return lib


def addr(a):
    assert isinstance(a, ctypes.c_void_p), a
    return a.value or 0


# ---- what one argument of the C call must be
def ptr(t):
    return ("ptr", t)


def val(v):
    return ("val", v)


def arr(ctype, values):
    return ("arr", ctype, values)


def host(ctype, key):
    return ("host", ctype, key)


def out(key):
    return ("out", key)


TAIL = [("ws",), ("wsn",), ("stream",)]


def check_call(lib, name, spec, result=None, Kparts=K):
    """One non-workspace call, to `name`, whose arguments are `spec`; `result` resolves out(key) / host(key)."""
    assert [c[0] for c in lib.calls] == [name]
    args = lib.calls[0][1]
    assert len(args) == len(_lib.SIGNATURES[name][1]) == len(spec)
    assert len(lib.ws) == 1
    for i, (a, s) in enumerate(zip(args, spec)):
        where = "%s argument %d" % (name, i)
        if s[0] == "ptr":
            assert addr(a) == (s[1].data_ptr() if s[1] is not None else 0), where
        elif s[0] == "val":
            assert type(a) is type(s[1]) and a == s[1], (where, a, s[1])
        elif s[0] == "arr":
            assert isinstance(a, ctypes.Array) and a._type_ is s[1] and list(a) == s[2], (where, list(a))
        elif s[0] == "host":
            assert isinstance(a, ctypes.Array) and a._type_ is s[1] and len(a) == Kparts, where
            assert result[s[2]] == [100 * i + k for k in range(Kparts)], (where, s[2])
        elif s[0] == "out":
            t = result[s[1]]
            assert addr(a) == (t.data_ptr() if t is not None else 0), (where, s[1])
        elif s[0] == "ws":
            assert addr(a) == lib.ws[0].data_ptr(), where
        elif s[0] == "wsn":
            assert a == lib.ws[0].numel() == WS_BYTES, where
        elif s[0] == "stream":
            assert addr(a) == STREAM, where
        elif s[0] == "plan":
            assert addr(a) == PLAN_H, where
        else:
            assert s[0] == "any", s


def check_fit_result(r, pe, dispersion=False, Kparts=K):
    keys = ["coef", "Sig_invMcoef", "Sig_inv", "n_iter", "status", "loglik"]
    keys += ["alpha", "alpha_info", "pearson"] if dispersion else []
    assert list(r) == keys + ["rc"]
    for key, shape in (("coef", (Kparts, pe)), ("Sig_invMcoef", (Kparts, pe)), ("Sig_inv", (Kparts, pe, pe))):
        assert tuple(r[key].shape) == shape and r[key].dtype == torch.float64 and r[key].is_contiguous(), key
    assert len({r[k].data_ptr() for k in keys[:3]}) == 3
    for key in keys[3:]:
        assert isinstance(r[key], list) and len(r[key]) == Kparts, key
    assert all(type(v) is int for v in r["n_iter"] + r["status"]) and all(type(v) is float for v in r["loglik"])


def rows(seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand((N, P + 1), dtype=torch.float64, generator=g)[:, :P]       # row pitch 4: ldx is not p
    y = torch.randint(0, 3, (N,), generator=g).to(torch.float64)
    offset = torch.rand((N,), dtype=torch.float64, generator=g)
    return X, y, offset


def raw(with_num=True):
    plan = types.SimpleNamespace(_h=ctypes.c_void_p(PLAN_H), p=PLAN_P)
    num = torch.rand((N, 2), dtype=torch.float64) if with_num else None
    codes = torch.zeros((N, 3), dtype=torch.int32)[:, :2]                       # row pitch 3
    return plan, num, codes


def raw_spec(num, codes):
    return [("plan",), ptr(num), val(2 if num is not None else 0), ptr(codes), val(3)]


I64, CI, CD = ctypes.c_int64, ctypes.c_int, ctypes.c_double
HOST3 = [host(CI, "n_iter"), host(CI, "status"), host(CD, "loglik")]
DISP3 = [host(CD, "alpha"), host(CD, "alpha_info"), host(CD, "pearson")]
OUT3 = [out("coef"), out("Sig_inv"), out("Sig_invMcoef")]


# ---------------------------------------------------------------------------------------------------------------------
# the six strided-partition fits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("icpt", [False, True])
def test_irls_fit_ex(fake, step, icpt):
    X, y, _ = rows()
    first, nrows = PARTS[step]
    r = engine.irls_fit_ex(X, y, first, nrows, row_step=step, fit_intercept=icpt, tol=1e-9, max_iter=17)
    pe = P + int(icpt)
    check_fit_result(r, pe)
    assert r["rc"] == 0
    check_call(fake, "dlsa_irls_fit_ex_f64",
               [ptr(X), val(4), ptr(y), arr(I64, first), arr(I64, nrows), val(step), val(K), val(P), val(int(icpt)), val(1e-9), val(17)]
               + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls == [("dlsa_irls_ex_workspace_bytes", (4, P, int(icpt), step))]


def test_irls_fit_ex_defaults(fake):
    X, y, _ = rows()
    engine.irls_fit_ex(X, y, *PARTS[1])
    a = fake.calls[0][1]
    assert a[5:11] == (1, K, P, 0, 1e-13, 100)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
def test_poisson_fit_ex(fake, step, icpt, with_offset):
    X, y, offset = rows()
    offset = offset if with_offset else None
    first, nrows = PARTS[step]
    r = engine.poisson_fit_ex(X, y, first, nrows, row_step=step, offset=offset, fit_intercept=icpt, tol=1e-9, max_iter=17)
    check_fit_result(r, P + int(icpt))
    check_call(fake, "dlsa_poisson_fit_f64",
               [ptr(X), val(4), ptr(y), ptr(offset), arr(I64, first), arr(I64, nrows), val(step), val(K), val(P), val(int(icpt)),
                val(1e-9), val(17)] + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls == [("dlsa_poisson_workspace_bytes", (4, P, int(icpt), step))]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("alpha", [None, 0.75])
def test_negbin_fit_ex(fake, step, icpt, with_offset, alpha):
    X, y, offset = rows()
    offset = offset if with_offset else None
    first, nrows = PARTS[step]
    r = engine.negbin_fit_ex(X, y, first, nrows, row_step=step, offset=offset, fit_intercept=icpt, alpha=alpha, tol=1e-9, max_iter=17)
    check_fit_result(r, P + int(icpt), dispersion=True)
    assert all(type(v) is float for v in r["alpha"] + r["alpha_info"] + r["pearson"])
    check_call(fake, "dlsa_negbin_fit_f64",
               [ptr(X), val(4), ptr(y), ptr(offset), arr(I64, first), arr(I64, nrows), val(step), val(K), val(P), val(int(icpt)),
                val(0.0 if alpha is None else alpha), val(1e-9), val(17)] + OUT3 + HOST3 + DISP3 + TAIL, r)
    assert fake.ws_calls == [("dlsa_negbin_workspace_bytes", (4, P, int(icpt), step))]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("with_num", [False, True])
def test_onehot_irls_fit_ex(fake, step, with_num):
    plan, num, codes = raw(with_num)
    _, y, _ = rows()
    first, nrows = PARTS[step]
    r = engine.onehot_irls_fit_ex(plan, num, codes, y, first, nrows, row_step=step, tol=1e-9, max_iter=17)
    check_fit_result(r, PLAN_P)
    check_call(fake, "dlsa_onehot_irls_fit_ex_f64",
               raw_spec(num, codes) + [ptr(y), arr(I64, first), arr(I64, nrows), val(step), val(K), val(1e-9), val(17)]
               + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_irls_ex_workspace_bytes" and fake.ws_calls[0][1][1:] == (4, step)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("with_offset", [False, True])
def test_onehot_poisson_fit_ex(fake, step, with_offset):
    plan, num, codes = raw()
    _, y, offset = rows()
    offset = offset if with_offset else None
    first, nrows = PARTS[step]
    r = engine.onehot_poisson_fit_ex(plan, num, codes, y, first, nrows, row_step=step, offset=offset, tol=1e-9, max_iter=17)
    check_fit_result(r, PLAN_P)
    check_call(fake, "dlsa_onehot_poisson_fit_f64",
               raw_spec(num, codes) + [ptr(y), ptr(offset), arr(I64, first), arr(I64, nrows), val(step), val(K), val(1e-9), val(17)]
               + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_poisson_workspace_bytes" and fake.ws_calls[0][1][1:] == (4, step)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("alpha", [None, 0.75])
def test_onehot_negbin_fit_ex(fake, step, with_offset, alpha):
    plan, num, codes = raw()
    _, y, offset = rows()
    offset = offset if with_offset else None
    first, nrows = PARTS[step]
    r = engine.onehot_negbin_fit_ex(plan, num, codes, y, first, nrows, row_step=step, offset=offset, alpha=alpha, tol=1e-9, max_iter=17)
    check_fit_result(r, PLAN_P, dispersion=True)
    check_call(fake, "dlsa_onehot_negbin_fit_f64",
               raw_spec(num, codes) + [ptr(y), ptr(offset), arr(I64, first), arr(I64, nrows), val(step), val(K),
                                       val(0.0 if alpha is None else alpha), val(1e-9), val(17)] + OUT3 + HOST3 + DISP3 + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_negbin_workspace_bytes" and fake.ws_calls[0][1][1:] == (4, step)


def _ex_callers():
    X, y, _ = rows()
    plan, num, codes = raw()
    return {
        "irls_fit_ex": lambda f, r, s: engine.irls_fit_ex(X, y, f, r, row_step=s),
        "poisson_fit_ex": lambda f, r, s: engine.poisson_fit_ex(X, y, f, r, row_step=s),
        "negbin_fit_ex": lambda f, r, s: engine.negbin_fit_ex(X, y, f, r, row_step=s),
        "onehot_irls_fit_ex": lambda f, r, s: engine.onehot_irls_fit_ex(plan, num, codes, y, f, r, row_step=s),
        "onehot_poisson_fit_ex": lambda f, r, s: engine.onehot_poisson_fit_ex(plan, num, codes, y, f, r, row_step=s),
        "onehot_negbin_fit_ex": lambda f, r, s: engine.onehot_negbin_fit_ex(plan, num, codes, y, f, r, row_step=s),
    }


EX_NAMES = sorted(_ex_callers())
BAD_PARTS = {"K = 0": ([], [], 1), "unequal lengths": ([0, 3], [3], 1), "step 0": ([0, 3], [3, 4], 0), "step -1": ([0, 3], [3, 4], -1),
             "negative first": ([-1, 3], [3, 4], 1), "negative rows": ([0, 3], [-1, 4], 1), "past n": ([0, 3], [3, 5], 1),
             "past n, strided": ([0, 1], [4, 4], 2), "first = n": ([0, 7], [3, 1], 1)}


@pytest.mark.parametrize("who", EX_NAMES)
@pytest.mark.parametrize("case", sorted(BAD_PARTS))
def test_strided_partitions_refused(fake, who, case):
    first, nrows, step = BAD_PARTS[case]
    with pytest.raises(ValueError, match="^%s: " % who):
        _ex_callers()[who](first, nrows, step)
    assert fake.calls == []


@pytest.mark.parametrize("who", EX_NAMES)
def test_strided_partitions_accepted_at_the_edge(fake, who):
    """The last row as a partition's last, an empty partition anywhere (even with its first row past the end's check: rows = 0 reads
    nothing), iterables of integer-likes and a float step that is a whole number."""
    _ex_callers()[who]((0, torch.tensor(6)), iter([0, 1]), 2.0)
    a = fake.calls[0][1]
    arrays = [list(v) for v in a if isinstance(v, ctypes.Array) and v._type_ is I64]
    assert arrays == [[0, 6], [0, 1]]
    step = a[5 if who in ("irls_fit_ex",) else 6 if not who.startswith("onehot") else (8 if who == "onehot_irls_fit_ex" else 9)]
    assert type(step) is int and step == 2
    fake.calls.clear()
    _ex_callers()[who]([0, 100], [7, 0], 1)
    assert len(fake.calls) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the three offset-form fits
# ---------------------------------------------------------------------------------------------------------------------
def test_irls_fit(fake):
    X, y, _ = rows()
    r = engine.irls_fit(X, y, OFFS, tol=1e-9, max_iter=17)
    check_fit_result(r, P)
    check_call(fake, "dlsa_irls_fit_f64", [ptr(X), val(4), ptr(y), arr(I64, OFFS), val(K), val(P), val(1e-9), val(17)] + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls == [("dlsa_irls_workspace_bytes", (4, P))]


@pytest.mark.parametrize("with_num", [False, True])
def test_onehot_irls_fit(fake, with_num):
    plan, num, codes = raw(with_num)
    _, y, _ = rows()
    r = engine.onehot_irls_fit(plan, num, codes, y, OFFS, tol=1e-9, max_iter=17)
    check_fit_result(r, PLAN_P)
    check_call(fake, "dlsa_onehot_irls_fit_f64", raw_spec(num, codes) + [ptr(y), arr(I64, OFFS), val(K), val(1e-9), val(17)] + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_irls_workspace_bytes" and fake.ws_calls[0][1][1:] == (4,)


def cox_rows():
    X, _, _ = rows()
    time = torch.arange(N, dtype=torch.float64)
    event = torch.ones(N, dtype=torch.float64)
    order = torch.arange(N - 1, -1, -1, dtype=torch.int64)
    return X, time, event, order


@pytest.mark.parametrize("ties", ["breslow", "Efron"])
@pytest.mark.parametrize("strata", [None, torch.int32, torch.int64])
def test_cox_fit(fake, ties, strata):
    X, time, event, order = cox_rows()
    codes = None if strata is None else (torch.arange(N) % 2).to(strata)
    r = engine.cox_fit(X, time, event, order, OFFS, tol=1e-9, max_iter=17, ties=ties, strata=codes)
    check_fit_result(r, P)
    code = 0 if ties == "breslow" else 1
    a = fake.calls[0][1]
    if strata is torch.int32:
        assert addr(a[4]) == codes.data_ptr()
    elif strata is torch.int64:           # converted: a tensor of the wrapper's own
        assert addr(a[4]) not in (0, codes.data_ptr())
    check_call(fake, "dlsa_cox_fit_strata_f64",
               [ptr(X), val(4), ptr(time), ptr(event), ptr(None) if strata is None else ("any",), ptr(order), arr(I64, OFFS), val(K), val(P),
                val(code), val(1e-9), val(17)] + OUT3 + HOST3 + TAIL, r)
    assert fake.ws_calls == [("dlsa_cox_strata_workspace_bytes", (4, P, code, 0 if strata is None else 1))]


def _offset_callers():
    X, y, _ = rows()
    plan, num, codes = raw()
    Xc, time, event, order = cox_rows()
    return {"irls_fit": lambda o: engine.irls_fit(X, y, o),
            "onehot_irls_fit": lambda o: engine.onehot_irls_fit(plan, num, codes, y, o),
            "cox_fit": lambda o: engine.cox_fit(Xc, time, event, order, o)}


# which offsets each offset-form wrapper takes: irls_fit and onehot_irls_fit check the range of the two ends only, cox_fit demands
# a start at 0 and non-decreasing offsets as well
OFFSET_CASES = {
    "halves": ([0, 3, 7], True, True),
    "one partition": ([0, 7], True, True),
    "an empty partition": ([0, 0, 7], True, True),
    "ends before n": ([0, 3, 5], True, True),
    "starts after 0": ([2, 5], True, False),
    "decreasing": ([0, 5, 3], True, False),
    "negative start": ([-1, 7], False, False),
    "past n": ([0, 8], False, False),
    "K = 0": ([0], False, False),
}


@pytest.mark.parametrize("who", ["irls_fit", "onehot_irls_fit", "cox_fit"])
@pytest.mark.parametrize("case", sorted(OFFSET_CASES))
def test_offset_partitions_acceptance(fake, who, case):
    offs, range_only, cox = OFFSET_CASES[case]
    call = _offset_callers()[who]
    if cox if who == "cox_fit" else range_only:
        r = call(offs)
        Kp = len(offs) - 1
        check_fit_result(r, PLAN_P if who == "onehot_irls_fit" else P, Kparts=Kp)
        a = fake.calls[0][1]
        assert [list(v) for v in a if isinstance(v, ctypes.Array) and v._type_ is I64] == [offs]
        assert fake.ws_calls[0][1][0 if who != "onehot_irls_fit" else 1] == max(offs[k + 1] - offs[k] for k in range(Kp))
    else:
        with pytest.raises(ValueError):
            call(offs)
        assert fake.calls == []


def test_offset_partitions_take_integer_likes(fake):
    X, y, _ = rows()
    engine.irls_fit(X, y, torch.tensor(OFFS))
    assert list(fake.calls[0][1][3]) == OFFS


# ---------------------------------------------------------------------------------------------------------------------
# soft failures, hard failures
# ---------------------------------------------------------------------------------------------------------------------
def _fit_callers():
    ex, off = _ex_callers(), _offset_callers()
    out = {k: (lambda f=f: f(*PARTS[1], 1)) for k, f in ex.items()}
    out.update({k: (lambda f=f: f(OFFS)) for k, f in off.items()})
    return out


FIT_NAMES = sorted(_fit_callers())


@pytest.mark.parametrize("who", FIT_NAMES)
@pytest.mark.parametrize("rc", [4, 5, 6])
def test_fit_soft_failure_codes_return(fake, who, rc):
    fake.rc = rc
    r = _fit_callers()[who]()
    assert r["rc"] == rc and len(r["status"]) == K


@pytest.mark.parametrize("who", FIT_NAMES)
@pytest.mark.parametrize("rc", [1, 2, 3, 7])
def test_fit_hard_failure_raises(fake, who, rc):
    fake.rc = rc
    with pytest.raises(_lib.DlsaError, match="fake failure") as e:
        _fit_callers()[who]()
    assert e.value.code == rc


# ---------------------------------------------------------------------------------------------------------------------
# the five pass wrappers
# ---------------------------------------------------------------------------------------------------------------------
def check_pass_outputs(res, pe, n, want_H, want_w, negbin=False, want_theta=False):
    assert isinstance(res, tuple) and len(res) == (6 if negbin else 4)
    H, g, ll, w = res[:4]
    shapes = [(H, (pe, pe), want_H), (g, (pe,), True), (ll, (1,), True), (w, (n,), want_w)]
    if negbin:
        shapes += [(res[4], (n,), want_w), (res[5], (3,), want_theta)]
    for t, shape, want in shapes:
        if not want:
            assert t is None
        else:
            assert tuple(t.shape) == shape and t.dtype == torch.float64 and t.is_contiguous()
    return dict(zip(["H", "g", "ll", "w", "mu", "tt"], res))


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w", [(True, False), (False, True)])
def test_poisson_pass(fake, icpt, with_offset, want_H, want_w):
    X, y, offset = rows()
    offset = offset if with_offset else None
    pe = P + int(icpt)
    beta = torch.zeros(pe, dtype=torch.float64)
    res = engine.poisson_pass(X, y, beta, offset=offset, fit_intercept=icpt, want_H=want_H, want_w=want_w)
    r = check_pass_outputs(res, pe, N, want_H, want_w)
    check_call(fake, "dlsa_poisson_pass_f64",
               [ptr(X), val(4), ptr(y), ptr(offset), ptr(beta), val(N), val(P), val(int(icpt)), out("H"), val(pe), out("g"), out("ll"),
                out("w")] + TAIL, r)
    assert fake.ws_calls == [("dlsa_poisson_workspace_bytes", (N, P, int(icpt), 1))]


def test_pass_defaults(fake):
    X, y, _ = rows()
    beta = torch.zeros(P, dtype=torch.float64)
    H, g, ll, w = engine.poisson_pass(X, y, beta)
    assert H is not None and w is None
    fake.calls.clear(); fake.ws.clear()
    H, g, ll, w, mu, tt = engine.negbin_pass(X, y, beta, 0.5)
    assert H is not None and w is None and mu is None and tt is None


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w,want_theta", [(True, False, False), (False, True, False), (False, False, True)])
def test_negbin_pass(fake, icpt, with_offset, want_H, want_w, want_theta):
    X, y, offset = rows()
    offset = offset if with_offset else None
    pe = P + int(icpt)
    beta = torch.zeros(pe, dtype=torch.float64)
    res = engine.negbin_pass(X, y, beta, 0.75, offset=offset, fit_intercept=icpt, want_H=want_H, want_w=want_w, want_theta=want_theta)
    r = check_pass_outputs(res, pe, N, want_H, want_w, negbin=True, want_theta=want_theta)
    check_call(fake, "dlsa_negbin_pass_f64",
               [ptr(X), val(4), ptr(y), ptr(offset), ptr(beta), val(0.75), val(N), val(P), val(int(icpt)), out("H"), val(pe), out("g"),
                out("ll"), out("w"), out("mu"), out("tt")] + TAIL, r)
    assert fake.ws_calls == [("dlsa_negbin_workspace_bytes", (N, P, int(icpt), 1))]


@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w", [(True, False), (False, True)])
def test_onehot_poisson_pass(fake, with_offset, want_H, want_w):
    plan, num, codes = raw()
    _, y, offset = rows()
    offset = offset if with_offset else None
    beta = torch.zeros(PLAN_P, dtype=torch.float64)
    res = engine.onehot_poisson_pass(plan, num, codes, y, beta, offset=offset, want_H=want_H, want_w=want_w)
    r = check_pass_outputs(res, PLAN_P, N, want_H, want_w)
    check_call(fake, "dlsa_onehot_poisson_pass_f64",
               raw_spec(num, codes) + [ptr(y), ptr(offset), ptr(beta), val(N), out("H"), val(PLAN_P), out("g"), out("ll"), out("w")] + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_poisson_workspace_bytes" and fake.ws_calls[0][1][1:] == (N, 1)


@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("want_H,want_w,want_theta", [(True, False, False), (False, True, False), (False, False, True)])
def test_onehot_negbin_pass(fake, with_offset, want_H, want_w, want_theta):
    plan, num, codes = raw()
    _, y, offset = rows()
    offset = offset if with_offset else None
    beta = torch.zeros(PLAN_P, dtype=torch.float64)
    res = engine.onehot_negbin_pass(plan, num, codes, y, beta, 0.75, offset=offset, want_H=want_H, want_w=want_w, want_theta=want_theta)
    r = check_pass_outputs(res, PLAN_P, N, want_H, want_w, negbin=True, want_theta=want_theta)
    check_call(fake, "dlsa_onehot_negbin_pass_f64",
               raw_spec(num, codes) + [ptr(y), ptr(offset), ptr(beta), val(0.75), val(N), out("H"), val(PLAN_P), out("g"), out("ll"), out("w"),
                                       out("mu"), out("tt")] + TAIL, r)
    assert fake.ws_calls[0][0] == "dlsa_onehot_negbin_workspace_bytes" and fake.ws_calls[0][1][1:] == (N, 1)


@pytest.mark.parametrize("ties", ["breslow", "efron"])
@pytest.mark.parametrize("with_strata", [False, True])
@pytest.mark.parametrize("want_w", [False, True])
def test_cox_pass(fake, ties, with_strata, want_w):
    X, time, event, _ = cox_rows()
    order = torch.tensor([5, 3, 1, 0], dtype=torch.int64)       # m = 4 of the 7 rows
    codes = (torch.arange(N) % 2).to(torch.int32) if with_strata else None
    beta = torch.zeros(P, dtype=torch.float64)
    res = engine.cox_pass(X, time, event, order, beta, want_w=want_w, ties=ties, strata=codes)
    r = check_pass_outputs(res, P, 4, True, want_w)
    code = engine.COX_TIES[ties]
    check_call(fake, "dlsa_cox_pass_strata_f64",
               [ptr(X), val(4), ptr(time), ptr(event), ptr(codes), ptr(order), val(4), val(P), val(code), ptr(beta), out("H"), val(P), out("g"),
                out("ll"), out("w")] + TAIL, r)
    assert fake.ws_calls == [("dlsa_cox_strata_workspace_bytes", (4, P, code, int(with_strata)))]


def _pass_callers():
    X, y, _ = rows()
    plan, num, codes = raw()
    Xc, time, event, order = cox_rows()
    b, bp = torch.zeros(P, dtype=torch.float64), torch.zeros(PLAN_P, dtype=torch.float64)
    return {"poisson_pass": lambda: engine.poisson_pass(X, y, b),
            "negbin_pass": lambda: engine.negbin_pass(X, y, b, 0.5),
            "onehot_poisson_pass": lambda: engine.onehot_poisson_pass(plan, num, codes, y, bp),
            "onehot_negbin_pass": lambda: engine.onehot_negbin_pass(plan, num, codes, y, bp, 0.5),
            "cox_pass": lambda: engine.cox_pass(Xc, time, event, order, b)}


@pytest.mark.parametrize("who", sorted(_pass_callers()))
@pytest.mark.parametrize("rc", [1, 4])
def test_pass_failure_raises(fake, who, rc):
    """A pass has no per-partition status to report through: every non-zero code raises."""
    fake.rc = rc
    with pytest.raises(_lib.DlsaError) as e:
        _pass_callers()[who]()
    assert e.value.code == rc


# ---------------------------------------------------------------------------------------------------------------------
# NB2 dispersion checks, and which of two errors wins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("who,other", [("negbin_fit_ex", "poisson_fit_ex"), ("onehot_negbin_fit_ex", "onehot_poisson_fit_ex")])
def test_fixed_alpha_checks(fake, who, other):
    X, y, _ = rows()
    plan, num, codes = raw()

    def fit(alpha, first=PARTS[1][0]):
        if who == "negbin_fit_ex":
            return engine.negbin_fit_ex(X, y, first, PARTS[1][1], alpha=alpha)
        return engine.onehot_negbin_fit_ex(plan, num, codes, y, first, PARTS[1][1], alpha=alpha)
    with pytest.raises(ValueError, match="^%s: alpha = 0 is the Poisson model: use %s$" % (who, other)):
        fit(0)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="^%s: .*positive and finite" % who):
            fit(bad)
    with pytest.raises(ValueError, match="Poisson"):        # the dispersion is checked before the partitions
        fit(0.0, first=[])
    assert fake.calls == []
    fit("0.25")
    assert fake.calls[0][1][10 if who == "negbin_fit_ex" else 11] == 0.25


@pytest.mark.parametrize("who,other", [("negbin_pass", "poisson_pass"), ("onehot_negbin_pass", "onehot_poisson_pass")])
def test_pass_alpha_checks(fake, who, other):
    X, y, _ = rows()
    plan, num, codes = raw()

    def run(alpha):
        if who == "negbin_pass":
            return engine.negbin_pass(X, y, torch.zeros(P, dtype=torch.float64), alpha)
        return engine.onehot_negbin_pass(plan, num, codes, y, torch.zeros(PLAN_P, dtype=torch.float64), alpha)
    for bad in (0, -0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="^%s: alpha must be positive and finite \\(alpha = 0 is %s\\)$" % (who, other)):
            run(bad)
    with pytest.raises(TypeError):
        run(None)
    assert fake.calls == []


def test_row_count_checks_come_first(fake):
    X, y, offset = rows()
    plan, num, codes = raw()
    for call in (lambda: engine.irls_fit_ex(X, y[:5], [], [], 0),
                 lambda: engine.poisson_fit_ex(X, y, [], [], 0, offset=offset[:5]),
                 lambda: engine.negbin_fit_ex(X, y[:5], [], [], 0, alpha=0.0),
                 lambda: engine.onehot_poisson_fit_ex(plan, num, codes, y, [], [], 0, offset=offset[:5]),
                 lambda: engine.onehot_negbin_fit_ex(plan, num[:5], codes, y, [], [], 0, alpha=0.0)):
        with pytest.raises(ValueError, match="n = 7"):
            call()
    with pytest.raises(TypeError, match="float64"):
        engine.irls_fit_ex(X, y.to(torch.float32), [], [], 0)
    with pytest.raises(ValueError, match="ties must be"):
        engine.cox_fit(X, y, y, torch.arange(N), [5, 3], ties="exact")
    for call in (lambda b: engine.poisson_pass(X, y, b), lambda b: engine.negbin_pass(X, y, b, 0.0),
                 lambda b: engine.onehot_poisson_pass(plan, num, codes, y, b), lambda b: engine.onehot_negbin_pass(plan, num, codes, y, b, 0.0),
                 lambda b: engine.cox_pass(X, y, y, torch.arange(N), b)):
        with pytest.raises(ValueError, match="beta|elements"):
            call(torch.zeros(PLAN_P + 1, dtype=torch.float64))
    assert fake.calls == []


# ---------------------------------------------------------------------------------------------------------------------
# models.py: the partition and column-name helpers
# ---------------------------------------------------------------------------------------------------------------------
def test_models_partitions():
    assert models._partitions(7, None, None) == ([0], [7], 1)
    assert models._partitions(7, 0, None) == ([0], [7], 1)
    assert models._partitions(7, 2, None) == ([0, 1], [4, 3], 2)
    first, nrows, step = models._partitions(10, 4, None)
    assert (first, step) == ([0, 1, 2, 3], 4) and nrows == [len(range(k, 10, 4)) for k in range(4)] == [3, 3, 2, 2]
    assert models._partitions(3, 5, None) == ([0, 1, 2, 3, 4], [1, 1, 1, 0, 0], 5)
    assert models._partitions(7, 2, [0, 3, 7]) == ([0, 3], [3, 4], 1)            # the offsets win
    assert models._partitions(7, None, torch.tensor([0, 0, 7])) == ([0, 0], [0, 7], 1)
    first, nrows, step = models._partitions(7, None, (2.0, 5))
    assert all(type(v) is int for v in first + nrows) and (first, nrows, step) == ([2], [3], 1)


def test_models_column_names():
    assert models._column_names(None, 3, False) == ["x0", "x1", "x2"]
    assert models._column_names(None, 2, True) == ["intercept", "x0", "x1"]
    assert models._column_names(("a", "b"), 2, False) == ["a", "b"]
    given = ["a", "b"]
    assert models._column_names(given, 2, True) == ["intercept", "a", "b"] and given == ["a", "b"]
    assert models._column_names(None, 0, True) == ["intercept"]
