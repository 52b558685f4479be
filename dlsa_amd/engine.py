"""Tensor-level front end of the HIP engine.

PyTorch-ROCm is used for device memory and streams only: every function here hands raw
device pointers to libdlsa_hip.so through the C ABI of include/dlsa_hip.h and returns torch
tensors that own the results.  There is no CPU path -- a CPU tensor raises.
"""
import contextlib
import ctypes
import dataclasses
import threading
from typing import Callable, NamedTuple, Optional

import numpy as np

import torch

from . import _lib
from ._lib import check

SYNTH_UNIFORM = 0
SYNTH_GAUSSIAN = 1

PART_STATUS = {0: "OK", 1: "NOT_CONVERGED", 2: "NOT_SPD", 3: "NAN", 4: "EMPTY"}

_ws_cache = {}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("dlsa_amd runs on the GPU only: got a %s tensor (no CPU fallback)" % t.device)


def _f64(t, name, dtype=torch.float64):
    """The C ABI reads raw pointers: refuse anything that is not what the entry point expects -- the wrong dtype
    would be reinterpreted (an fp32 X read as n*ldx doubles runs past the buffer; integer labels read as ~0.0), a
    strided vector read as if it were contiguous.  2-D: row-major with unit column stride (any row pitch);
    1-D: contiguous.  None passes (nullable arguments)."""
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch tensor on the GPU" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s (no implicit casts at the C ABI: convert with .to(%s))"
                        % (name, dtype, t.dtype, dtype))
    if t.dim() == 2:
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError("%s must be row-major (stride(1) == 1)" % name)
        if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
            raise ValueError("%s: row pitch %d smaller than its %d columns" % (name, t.stride(0), t.shape[1]))
    elif not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


_WS_MAX_STREAMS = 4


def _workspace(nbytes, device):
    """Scratch buffer per (device, current stream), 256-byte aligned by the torch allocator.  The C ABI is re-entrant across
    streams as long as concurrent calls bring their own workspace: work enqueued on two streams must not share scratch, and
    work on ONE stream is ordered, so a buffer per stream is exactly enough.  The cache is an LRU of _WS_MAX_STREAMS streams
    (a Gram scratch is ~0.5 GB at p = 500: a stream-per-request caller must not pin one per short-lived stream forever);
    an evicted buffer goes back to torch's stream-aware allocator, which keeps it alive until the work queued on it is done.
    release_workspace() drops everything."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.pop(key, None)
    if buf is None or buf.numel() < nbytes:
        buf = None
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
    _ws_cache[key] = buf                     # (re)inserted last: dict order is the LRU order
    while len(_ws_cache) > _WS_MAX_STREAMS:
        old = next(iter(_ws_cache))
        victim = _ws_cache.pop(old)
        victim.record_stream(torch.cuda.current_stream(device))      # conservative: not reused before this stream's queued work
        del victim
    return buf


def release_workspace():
    _ws_cache.clear()


release_workspaces = release_workspace


def _rowmajor(X):
    # (a single column is row-major whatever stride(1) says: torch and numpy keep the parent's pitch on a size-1 dimension)
    if X.dim() != 2 or (X.shape[1] > 1 and X.stride(1) != 1):
        raise ValueError("X must be a 2-D row-major tensor (stride(1) == 1)")
    return max(X.stride(0), X.shape[1]) if X.shape[0] > 1 else max(X.stride(0), X.shape[1])


def rows_to_device(a, device="cuda"):
    """Host matrix [n, p] -> row-major device tensor.  pandas keeps the columns of one dtype as ONE [p, n] block, so
    `frame.to_numpy()` is a column-major VIEW of it; making that row-major on the host is a strided single-threaded copy
    (76 ms for 1e6 x 100 doubles), so a column-major array goes over the link as it lies and is transposed in HBM."""
    if isinstance(a, np.ndarray) and a.ndim == 2 and a.size > 0 and not a.flags.c_contiguous and a.flags.f_contiguous:
        t = torch.from_numpy(a.T).to(device).t()
    else:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if t.dim() == 2 and (t.stride(1) != 1 or t.stride(0) != t.shape[1]) and t.numel() > 0:
        # (a size-1 dimension counts as contiguous with ANY stride, for numpy and torch alike: an [n, 1] column view keeps its parent's pitch)
        out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        out.copy_(t)
        return out
    return t


def empty_rows(n, p, dtype=torch.float64, device="cuda"):
    """[n, p] row-major matrix whose row pitch is a whole number of 16-byte units (an odd fp64 p gets one pad
    element per row, zeroed): the Gram kernels stage such rows with vector loads / the LDS-DMA for any p, whereas
    rows that start at odd multiples of 8 bytes take the scalar staging path (p=501: 28.8 vs 20.6 ms per 5e6 rows).
    Exception (round 5): an odd fp64 width of the fused Newton pass's class (49 .. 120) stays PACKED -- that kernel streams packed
    odd rows (the piece of a row's last column carries the next row's first element: data, where a pad element would be bytes the
    library cannot vouch for), and a fit at these widths takes every Hessian from it."""
    unit = 16 // torch.empty((), dtype=dtype).element_size()
    ld = (p + unit - 1) // unit * unit
    if ld == p or (dtype == torch.float64 and (p & 1) and 49 <= p <= 120):
        return torch.empty((n, p), dtype=dtype, device=device)
    buf = torch.empty((n, ld), dtype=dtype, device=device)
    buf[:, p:] = 0
    return buf[:, :p]


def with_ones_column(X):
    """[1 | X] (the intercept column of dlsa/models.py:121-122) in an aligned row pitch."""
    out = empty_rows(X.shape[0], X.shape[1] + 1, X.dtype, X.device)
    out[:, 0] = 1
    out[:, 1:] = X
    return out


def row_major(X):
    """X itself when it is row-major with unit column stride (any row pitch), else a contiguous copy."""
    return X if (X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]) else X.contiguous()


def synth(seed, row0, n, p, kind=SYNTH_UNIFORM, ones_col=False, labels=True, dtype=torch.float64,
          device="cuda", beta_true=None, out=None):
    """Seeded synthetic logistic rows (replaces simulate_logistic, dlsa/models.py:6-40).
    Returns (X [n, p + ones_col], y [n] or None)."""
    lib = _lib.load()
    cols = p + (1 if ones_col else 0)
    X = out if out is not None else empty_rows(n, cols, dtype, device)
    _require_gpu(X)
    y = torch.empty((n,), dtype=dtype, device=X.device) if labels else None
    fn = lib.dlsa_synth_f64 if dtype == torch.float64 else lib.dlsa_synth_f32
    # one launch handles < 2^31 workgroups: chunk the rows
    chunk = max(1, (1 << 28) // max(1, (p + 1) // 2))
    ld = _rowmajor(X)
    for r in range(0, n, chunk):
        m = min(chunk, n - r)
        check(fn(seed, row0 + r, m, p, kind, 1 if ones_col else 0,
                 _ptr(X[r:]), ld, _ptr(y[r:]) if labels else ctypes.c_void_p(0),
                 _ptr(beta_true), _stream()))
    return X, y


def synth_response(seed, row0, X, sigma=1.0, ones_col=False, beta_true=None, out=None):
    """Linear-model response y = X beta* + sigma N(0,1) for rows `synth` wrote (config 5; dlsa_synth_response_*): the noise of
    row i is a function of (seed, row0 + i) only.  X [n, p (+1 with ones_col)] fp64 / fp32 on the GPU; returns y [n]."""
    lib = _lib.load()
    _require_gpu(X, beta_true, out)
    if X.dtype not in (torch.float64, torch.float32):
        raise TypeError("synth_response: X must be float64 or float32")
    _f64(X, "X", X.dtype); _f64(beta_true, "beta_true", X.dtype); _f64(out, "out", X.dtype)
    n, cols = X.shape
    p = cols - (1 if ones_col else 0)
    y = out if out is not None else torch.empty((n,), dtype=X.dtype, device=X.device)
    if y.numel() != n or (beta_true is not None and beta_true.numel() != cols):
        raise ValueError("synth_response: y must have n and beta_true p (+1) elements")
    fn = lib.dlsa_synth_response_f64 if X.dtype == torch.float64 else lib.dlsa_synth_response_f32
    chunk = 1 << 30
    ld = _rowmajor(X)
    for r in range(0, n, chunk):
        m = min(chunk, n - r)
        check(fn(seed, row0 + r, m, p, 1 if ones_col else 0, _ptr(X[r:]), ld, _ptr(beta_true), float(sigma), _ptr(y[r:]), _stream()))
    return y


def synth_linear32(seed, row0, n, p, sigma=1.0, ones_col=False, beta_true=None, out=None, out_y=None, response=True):
    """fp32-native linear rows, features AND response in one launch (dlsa_synth_linear_f32: x ~ N(0, 1/12) from four 24-bit
    uniforms per Philox call, y = x . beta* + sigma N(0,1), everything in fp32 with the device's transcendental instructions).
    The chunk generator of the streaming map step at config 5's size: 4x cheaper than synth(kind=GAUSSIAN, float32) +
    synth_response.  Returns (X [n, p (+1)], y [n] or None)."""
    lib = _lib.load()
    cols = p + (1 if ones_col else 0)
    X = out if out is not None else empty_rows(n, cols, torch.float32, "cuda")
    _require_gpu(X, beta_true, out_y)
    _f64(X, "X", torch.float32); _f64(beta_true, "beta_true", torch.float32); _f64(out_y, "out_y", torch.float32)
    if tuple(X.shape) != (n, cols) or (beta_true is not None and beta_true.numel() != cols):
        raise ValueError("synth_linear32: X must be [n, p (+1)] and beta_true have p (+1) elements")
    y = None
    if response:
        y = out_y if out_y is not None else torch.empty((n,), dtype=torch.float32, device=X.device)
        if y.numel() != n:
            raise ValueError("synth_linear32: y must have n elements")
    check(lib.dlsa_synth_linear_f32(seed, row0, n, p, 1 if ones_col else 0, _ptr(X), _rowmajor(X), _ptr(beta_true), float(sigma),
                                    _ptr(y), _stream()))
    return X, y


def design(num, codes, kind, src, level, shift, scale, dtype=torch.float64, out=None):
    """Dense design matrix from raw numeric columns + integer level codes (models.py:56-104,121-122).
    num [n,q] (dtype) or None, codes [n,f] int32 or None; kind/src/level int32 [p], shift/scale fp64 [p]
    (device).  Returns (X [n,p], seen int32 [p]: 1 where the column has a non-zero entry)."""
    lib = _lib.load()
    _require_gpu(num, codes, kind, src, level, shift, scale, out)
    p = kind.numel()
    n = num.shape[0] if num is not None else codes.shape[0]
    q = num.shape[1] if num is not None else 0
    f = codes.shape[1] if codes is not None else 0
    if num is not None and num.dtype != dtype:
        raise ValueError("num must have the output dtype")
    if codes is not None and codes.dtype != torch.int32:
        raise ValueError("codes must be int32")
    dev = kind.device
    X = out if out is not None else empty_rows(n, p, dtype, dev)
    seen = torch.empty((p,), dtype=torch.int32, device=dev)
    fn = lib.dlsa_design_f64 if dtype == torch.float64 else lib.dlsa_design_f32
    check(fn(_ptr(num), _rowmajor(num) if num is not None else 0, q,
             _ptr(codes), _rowmajor(codes) if codes is not None else 0, f, n,
             _ptr(kind), _ptr(src), _ptr(level), _ptr(shift), _ptr(scale), p, _ptr(X), _rowmajor(X), _ptr(seen),
             _stream()))
    return X, seen


def gram(X, w=None, out=None, accumulate=False):
    """H = X' diag(w) X (dlsa/models.py:130) on the MFMA Gram kernel.  X [n,p] fp64/fp32."""
    lib = _lib.load()
    _require_gpu(X, w, out)
    if X.dtype not in (torch.float64, torch.float32):
        raise TypeError("gram: X must be float64 or float32, got %s" % X.dtype)
    _f64(X, "X", X.dtype); _f64(out, "out", X.dtype)
    n, p = X.shape
    ldx = _rowmajor(X)
    if out is not None and (out.dim() != 2 or tuple(out.shape) != (p, p)):
        raise ValueError("gram: out must be p x p")
    H = out if out is not None else torch.empty((p, p), dtype=X.dtype, device=X.device)
    es = X.element_size()
    nb = lib.dlsa_gram_workspace_bytes(n, p, es)
    ws = _workspace(nb, X.device)
    fn = lib.dlsa_gram_f64 if X.dtype == torch.float64 else lib.dlsa_gram_f32
    if w is not None and (w.dtype != X.dtype or not w.is_contiguous() or w.numel() != n):
        raise ValueError("w must be a contiguous vector of n elements with X's dtype")
    check(fn(_ptr(X), ldx, _ptr(w), n, p, _ptr(H), _rowmajor(H), 1 if accumulate else 0,
             _ptr(ws), ws.numel(), _stream()))
    return H


def gram_acc64(X, w=None, out=None, accumulate=False):
    """fp32 rows, fp64 result (dlsa_gram_f32_acc64): the MFMA passes of gram() on fp32 rows with the slab partials summed in
    fp64 and stored / added (accumulate) into the fp64 matrix `out` [p, p] (any row pitch: a sub-block view works).  The
    streaming linear map step adds chunk after chunk this way."""
    lib = _lib.load()
    _require_gpu(X, w, out)
    _f64(X, "X", torch.float32); _f64(w, "w", torch.float32); _f64(out, "out")
    n, p = X.shape
    H = out if out is not None else torch.empty((p, p), dtype=torch.float64, device=X.device)
    if H.dim() != 2 or tuple(H.shape) != (p, p):
        raise ValueError("gram_acc64: out must be p x p")
    if w is not None and w.numel() != n:
        raise ValueError("gram_acc64: w must have n elements")
    ws = _workspace(lib.dlsa_gram_workspace_bytes(n, p, 4), X.device)
    check(lib.dlsa_gram_f32_acc64(_ptr(X), _rowmajor(X), _ptr(w), n, p, _ptr(H), _rowmajor(H), 1 if accumulate else 0,
                                  _ptr(ws), ws.numel(), _stream()))
    return H


def xtv_stats(X, v, g=None, colsum=None, stats=None, want_colsum=False, accumulate=False):
    """One read of X: g = X'v, colsum = X'1 (optional: the implicit intercept's border), stats = [v'v, sum v], all fp64
    whatever X's type (dlsa_xtv_stats_*); accumulate adds to the given outputs.  Returns (g, colsum or None, stats)."""
    lib = _lib.load()
    _require_gpu(X, v, g, colsum, stats)
    if X.dtype not in (torch.float64, torch.float32):
        raise TypeError("xtv_stats: X must be float64 or float32")
    _f64(X, "X", X.dtype); _f64(v, "v", X.dtype); _f64(g, "g"); _f64(colsum, "colsum"); _f64(stats, "stats")
    n, p = X.shape
    if v.numel() != n:
        raise ValueError("xtv_stats: v must have n = %d elements" % n)
    dev = X.device
    if accumulate and (g is None or stats is None or (want_colsum and colsum is None)):
        raise ValueError("xtv_stats: accumulate needs the outputs to add to")
    g = g if g is not None else torch.empty((p,), dtype=torch.float64, device=dev)
    stats = stats if stats is not None else torch.empty((2,), dtype=torch.float64, device=dev)
    if want_colsum and colsum is None:
        colsum = torch.empty((p,), dtype=torch.float64, device=dev)
    if g.numel() != p or stats.numel() != 2 or (colsum is not None and colsum.numel() != p):
        raise ValueError("xtv_stats: g / colsum must have p and stats 2 elements")
    es = X.element_size()
    ws = _workspace(lib.dlsa_xtv_stats_workspace_bytes(p, es), dev)
    fn = lib.dlsa_xtv_stats_f64 if es == 8 else lib.dlsa_xtv_stats_f32
    check(fn(_ptr(X), _rowmajor(X), _ptr(v), n, p, _ptr(g), _ptr(colsum if want_colsum else None), _ptr(stats),
             1 if accumulate else 0, _ptr(ws), ws.numel(), _stream()))
    return g, (colsum if want_colsum else None), stats


def gram_last_kernel(want_cycles=False):
    """(name, shader cycles) of the Gram kernel this thread's last Gram launch dispatched (dlsa_gram_last_kernel):
    which of the kernels of DESIGN.md section 4.1 ran, and -- want_cycles, which synchronises -- the s_memtime delta of
    wave 0 of workgroup 0 (0 for kernels without the probe).  cycles / kernel time = the sustained shader clock."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(160)
    cyc = ctypes.c_uint64(0)
    check(lib.dlsa_gram_last_kernel(buf, 160, ctypes.byref(cyc) if want_cycles else None))
    return buf.value.decode(), int(cyc.value)


def logit_pass(X, y, beta, want_w=True, want_g=True, want_loglik=True, fit_intercept=False):
    """One fused pass: w = mu(1-mu), g = X'(y-mu), loglik.  Returns (w, g, loglik) tensors.  fit_intercept: the ones
    column is implicit -- beta and g have p + 1 entries, intercept first."""
    lib = _lib.load()
    _require_gpu(X, y, beta)
    _f64(X, "X"); _f64(y, "y"); _f64(beta, "beta")
    n, p = X.shape
    pe = p + (1 if fit_intercept else 0)
    if y.numel() != n or beta.numel() != pe:
        raise ValueError("logit_pass: y must have n = %d and beta %d elements" % (n, pe))
    ldx = _rowmajor(X)
    w = torch.empty((n,), dtype=torch.float64, device=X.device) if want_w else None
    g = torch.empty((pe,), dtype=torch.float64, device=X.device) if want_g else None
    ll = torch.empty((1,), dtype=torch.float64, device=X.device) if want_loglik else None
    nb = lib.dlsa_logit_workspace_bytes(n, p)
    ws = _workspace(nb, X.device)
    fn = lib.dlsa_logit_pass_icpt_f64 if fit_intercept else lib.dlsa_logit_pass_f64
    check(fn(_ptr(X), ldx, _ptr(y), _ptr(beta), n, p, _ptr(w), _ptr(g), _ptr(ll), _ptr(ws), ws.numel(), _stream()))
    return w, g, ll


def irls_pass(X, y, beta, want_w=False):
    """One Newton pass in ONE call (dlsa_irls_pass_f64): w = mu(1-mu) at beta, g = X'(y-mu), loglik and H = X' diag(w) X.
    Narrow designs (49 <= p <= 120, even, aligned rows, n >= 8192) run the FUSED kernel -- one read of X; every other shape
    the logit pass + the Gram pass behind the same entry (gram_last_kernel() names what ran).  Returns (H, g, loglik, w or None)."""
    lib = _lib.load()
    _require_gpu(X, y, beta)
    _f64(X, "X"); _f64(y, "y"); _f64(beta, "beta")
    n, p = X.shape
    if y.numel() != n or beta.numel() != p:
        raise ValueError("irls_pass: y must have n = %d and beta p = %d elements" % (n, p))
    dev = X.device
    H = torch.empty((p, p), dtype=torch.float64, device=dev)
    g = torch.empty((p,), dtype=torch.float64, device=dev)
    ll = torch.empty((1,), dtype=torch.float64, device=dev)
    w = torch.empty((n,), dtype=torch.float64, device=dev) if want_w else None
    ws = _workspace(lib.dlsa_irls_pass_workspace_bytes(n, p), dev)
    check(lib.dlsa_irls_pass_f64(_ptr(X), _rowmajor(X), _ptr(y), _ptr(beta), n, p, _ptr(H), p, _ptr(g), _ptr(ll), _ptr(w),
                                 _ptr(ws), ws.numel(), _stream()))
    return H, g, ll, w


def newton_wide_pass(X, y, beta, fit_intercept=False, want_w=False):
    """The wide Newton pass (dlsa_newton_wide_pass_f64): g, loglik (and w) of the logit pass at beta plus, from the SAME read of
    the rows, the reduced-precision Hessian that preconditions the fit's Newton steps (bf16 products, fp32 accumulation; never a
    result: exported for diagnostics and tests).  Returns (H_approx, g, loglik, w or None); raises when the shape is not served
    (121 <= p + intercept <= 512, >= 32768 rows; any pitch or alignment -- unaligned / odd-pitch rows take the scalar-load form)."""
    lib = _lib.load()
    _require_gpu(X, y, beta)
    _f64(X, "X"); _f64(y, "y"); _f64(beta, "beta")
    n, p = X.shape
    icpt = 1 if fit_intercept else 0
    pe = p + icpt
    if y.numel() != n or beta.numel() != pe:
        raise ValueError("newton_wide_pass: y must have n = %d and beta %d elements" % (n, pe))
    dev = X.device
    H = torch.empty((pe, pe), dtype=torch.float64, device=dev)
    g = torch.empty((pe,), dtype=torch.float64, device=dev)
    ll = torch.empty((1,), dtype=torch.float64, device=dev)
    w = torch.empty((n,), dtype=torch.float64, device=dev) if want_w else None
    ws = _workspace(lib.dlsa_newton_wide_workspace_bytes(n, p, icpt), dev)
    check(lib.dlsa_newton_wide_pass_f64(_ptr(X), _rowmajor(X), _ptr(y), _ptr(beta), n, p, icpt, _ptr(w), _ptr(g),
                                        _ptr(ll), _ptr(H), pe, _ptr(ws), ws.numel(), _stream()))
    return H, g, ll, w


def gram_icpt(X, w=None, out=None):
    """H = [1 | X]' diag(w) [1 | X], (p + 1) x (p + 1), without materialising the ones column (models.py:121-130)."""
    lib = _lib.load()
    _require_gpu(X, w, out)
    _f64(X, "X"); _f64(w, "w"); _f64(out, "out")
    n, p = X.shape
    if w is not None and w.numel() != n:
        raise ValueError("gram_icpt: w must have n elements")
    H = out if out is not None else torch.empty((p + 1, p + 1), dtype=torch.float64, device=X.device)
    if tuple(H.shape) != (p + 1, p + 1):
        raise ValueError("gram_icpt: out must be (p + 1) x (p + 1)")
    ws = _workspace(lib.dlsa_gram_icpt_workspace_bytes(n, p), X.device)
    check(lib.dlsa_gram_icpt_f64(_ptr(X), _rowmajor(X), _ptr(w), n, p, _ptr(H), _rowmajor(H), _ptr(ws), ws.numel(), _stream()))
    return H


def loglik(X, y, par, fit_intercept=False):
    """Log-likelihood of each column of par [p, c] (dlsa/models.py:217-222).  fit_intercept: par has p + 1 rows, the
    first one the intercepts; the ones column is implicit."""
    lib = _lib.load()
    _require_gpu(X, y, par)
    _f64(X, "X"); _f64(y, "y")
    n, p = X.shape
    par = par.contiguous()
    _f64(par, "par")
    if par.dim() != 2 or par.shape[0] != p + (1 if fit_intercept else 0) or y.numel() != n:
        raise ValueError("loglik: par must be [p (+1), c] and y [n]")
    c = par.shape[1]
    out = torch.empty((c,), dtype=torch.float64, device=X.device)
    nb = lib.dlsa_logit_workspace_bytes(n, p)
    ws = _workspace(nb, X.device)
    fn = lib.dlsa_loglik_icpt_f64 if fit_intercept else lib.dlsa_loglik_f64
    check(fn(_ptr(X), _rowmajor(X), _ptr(y), n, p, _ptr(par), par.stride(0), c, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def xtv(X, v):
    """g = X'v and v'v in one read of X (linear-model map step).  Returns (g [p], vv [1]) in X's dtype."""
    lib = _lib.load()
    _require_gpu(X, v)
    if X.dtype not in (torch.float64, torch.float32):
        raise TypeError("xtv: X must be float64 or float32")
    _f64(X, "X", X.dtype)
    v = _f64(v.contiguous(), "v", X.dtype)
    n, p = X.shape
    if v.numel() != n:
        raise ValueError("xtv: v must have n = %d elements" % n)
    g = torch.empty((p,), dtype=X.dtype, device=X.device)
    vv = torch.empty((1,), dtype=X.dtype, device=X.device)
    nb = lib.dlsa_logit_workspace_bytes(n, p) * (2 if X.dtype == torch.float32 else 1)
    ws = _workspace(nb, X.device)
    if X.dtype == torch.float32:
        check(lib.dlsa_xtv_f32(_ptr(X), _rowmajor(X), _ptr(v.contiguous()), n, p, _ptr(g), _ptr(vv),
                               _ptr(ws), ws.numel(), _stream()))
        return g, vv
    check(lib.dlsa_xtv_f64(_ptr(X), _rowmajor(X), _ptr(v.contiguous()), n, p, _ptr(g), _ptr(vv),
                           _ptr(ws), ws.numel(), _stream()))
    return g, vv


@dataclasses.dataclass
class IrlsOptions:
    """Policy of the IRLS driver for the fits made inside `with engine.irls_options(opts):` (or passed as `options=` to
    fit_logistic_partitions / fit_logistic_design / logistic_model): include/dlsa_hip.h dlsa_irls_options, field for field.  None =
    automatic (the measured default for the shapes); every setting returns the same MLE and Hessian to the parity tolerance."""
    chains: Optional[int] = None            # partition chains of one call (host threads + streams), 1..8
    seeded: Optional[bool] = None           # partition 0 alone first, every chain seeded with its state
    subsample_div: Optional[int] = None     # cold start on rows / d of a partition; 0 or 1: none
    factor_div: Optional[int] = None
    warm: Optional[bool] = None             # partition k + 1 starts from partition k's MLE
    inherit: Optional[bool] = None
    pool: Optional[bool] = None
    secant: Optional[bool] = None
    inverse: Optional[bool] = None
    predict: Optional[bool] = None          # predicted convergence
    fused: Optional[bool] = None            # fused Newton pass (one read of the rows per fresh Hessian)
    fuse_last: Optional[bool] = None
    small: Optional[bool] = None            # one-launch kernel for many small partitions
    batched: Optional[bool] = None          # lock-step fit of all partitions together (narrow designs)
    qn_threads: Optional[int] = None
    trace: Optional[bool] = None
    lean: Optional[bool] = None             # fits at fused widths write no weight vector
    small_cluster: Optional[int] = None     # workgroups per partition of the one-launch kernel, 1..16
    own_hessian: Optional[bool] = None      # wide designs: Newton steps preconditioned by the partition's own reduced-precision Hessian
    pooled_start: Optional[bool] = None     # lock step: full-row iterations start from one fit on the leading rows of all partitions
    grad_passes: Optional[int] = None       # lock step: at most this many gradient-only passes before the Newton passes; 0: none
    freeze_at: Optional[float] = None       # 0: never freeze the factor

    def as_c(self):
        lib = _lib.load()
        c = _lib.IrlsOptionsC()
        lib.dlsa_irls_options_init(ctypes.byref(c))
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if v is not None:
                setattr(c, f.name, float(v) if f.name == "freeze_at" else int(v))
        return c


_options_stack = threading.local()          # the calling thread's active IrlsOptions, innermost last


@contextlib.contextmanager
def irls_options(options=None, **fields):
    """The calling thread's IRLS driver options for the fits (and workspace sizes) inside the block: an IrlsOptions, or its fields as
    keyword arguments (`with engine.irls_options(chains=1, fused=False): ...`).  Blocks nest: the fields set here are merged over the
    enclosing block's, and the enclosing options are restored on exit (automatic only when the outermost block ends)."""
    if options is None:
        options = IrlsOptions(**fields) if fields else None
    elif fields:
        options = dataclasses.replace(options, **fields)
    if options is None:
        yield
        return
    lib = _lib.load()
    stack = getattr(_options_stack, "items", None)
    if stack is None:
        stack = _options_stack.items = []
    if stack:           # merge over the enclosing block's options
        outer = stack[-1]
        options = dataclasses.replace(outer, **{f.name: getattr(options, f.name) for f in dataclasses.fields(options)
                                               if getattr(options, f.name) is not None})
    c = options.as_c()
    check(lib.dlsa_irls_set_options(ctypes.byref(c)))
    stack.append(options)
    try:
        yield
    finally:
        stack.pop()
        if stack:
            c = stack[-1].as_c()
            lib.dlsa_irls_set_options(ctypes.byref(c))
        else:
            lib.dlsa_irls_set_options(None)


@dataclasses.dataclass
class KernelOptions:
    """Which build of a kernel runs (never what it returns) for the calls inside `with engine.kernel_options(...)`:
    include/dlsa_hip.h dlsa_kernel_options, field for field.  None = automatic.  The library reads no environment variable for these."""
    lars_q: Optional[int] = None            # LARS form: 0 lars.hip everywhere; 1 lars_q.hip up to 1020 variables, lars_c.hip beyond; 2 lars_c.hip from 64; None: the measured hand-over (448)
    lars_q_wgs: Optional[int] = None        # workgroups that share its fused pass, 1..8
    lars_q_threads: Optional[int] = None    # 256 | 512 | 1024
    lars_q_lds: Optional[bool] = None
    lars_wgs: Optional[int] = None          # workgroups of lars.hip's grid kernel (1..32) / of lars_c.hip's column split (2..64)
    lars_threads: Optional[int] = None      # 512 | 1024
    logit_ring: Optional[bool] = None       # narrow designs' logit pass through the LDS-DMA ring
    chol_small: Optional[bool] = None       # one-launch SPD inverse for p <= 112
    gram_wide_f32: Optional[bool] = None    # the fp32 wide Gram kernel (p >= 768)
    onehot_ordered: Optional[int] = None    # 0 unordered, 1 ordered floating point
    gram_variant: Optional[int] = None      # valid-result A/B bits of the fp64 Gram dispatch (2 | 4 | 8 | 32 | 64 | 256; 16 = the cyclic kernel's two-wave twin)
    cooperative: Optional[bool] = None      # multi-workgroup kernels launched cooperatively

    def as_c(self):
        lib = _lib.load()
        c = _lib.KernelOptionsC()
        lib.dlsa_kernel_options_init(ctypes.byref(c))
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if v is not None:
                setattr(c, f.name, int(v))
        return c


_kernel_options_stack = threading.local()

# the environment variables earlier rounds' A/B scripts used for these switches, honoured by the HOST layer only (bench/ scripts call
# kernel_options_from_env(); the library itself never reads them)
_KERNEL_ENV = {"DLSA_LARS_Q": "lars_q", "DLSA_LARS_Q_WGS": "lars_q_wgs", "DLSA_LARS_Q_THREADS": "lars_q_threads", "DLSA_LARS_Q_LDS": "lars_q_lds",
               "DLSA_LARS_WGS": "lars_wgs", "DLSA_LARS_THREADS": "lars_threads", "DLSA_LOGIT_RING": "logit_ring", "DLSA_CHOL_SMALL": "chol_small",
               "DLSA_GRAM_WIDE_F32": "gram_wide_f32", "DLSA_OH_ORDERED": "onehot_ordered", "DLSA_GRAM_DBG": "gram_variant", "DLSA_COOPERATIVE": "cooperative"}


def kernel_options_from_env(environ=None):
    """A KernelOptions from the DLSA_* variables of the A/B scripts (None when none is set)."""
    import os
    environ = os.environ if environ is None else environ
    fields = {f: int(environ[k]) for k, f in _KERNEL_ENV.items() if environ.get(k, "") != ""}
    return KernelOptions(**fields) if fields else None


@contextlib.contextmanager
def kernel_options(options=None, **fields):
    """The calling thread's kernel switches for the calls inside the block (a KernelOptions, or its fields as keyword arguments);
    blocks nest like irls_options."""
    if options is None:
        options = KernelOptions(**fields) if fields else None
    elif fields:
        options = dataclasses.replace(options, **fields)
    if options is None:
        yield
        return
    lib = _lib.load()
    stack = getattr(_kernel_options_stack, "items", None)
    if stack is None:
        stack = _kernel_options_stack.items = []
    if stack:
        options = dataclasses.replace(stack[-1], **{f.name: getattr(options, f.name) for f in dataclasses.fields(options)
                                                    if getattr(options, f.name) is not None})
    c = options.as_c()
    check(lib.dlsa_kernel_set_options(ctypes.byref(c)))
    stack.append(options)
    try:
        yield
    finally:
        stack.pop()
        if stack:
            c = stack[-1].as_c()
            lib.dlsa_kernel_set_options(ctypes.byref(c))
        else:
            lib.dlsa_kernel_set_options(None)


IRLS_PATH_CHAINS, IRLS_PATH_SMALL, IRLS_PATH_BATCHED = 0, 1, 2


def irls_last_fit_path():
    """Which driver this thread's last irls_fit / irls_fit_ex took (dlsa_irls_last_fit_path): IRLS_PATH_CHAINS (host-driven partition
    chains), IRLS_PATH_SMALL (one launch, a workgroup per partition) or IRLS_PATH_BATCHED (lock step: all partitions together)."""
    return int(_lib.load().dlsa_irls_last_fit_path())


# Codes a fit returns after it has written every block (include/dlsa_hip.h): DLSA_OK, and the soft failures DLSA_ERR_NOT_SPD (4),
# DLSA_ERR_NOT_CONVERGED (5) and DLSA_ERR_NAN (6), which the per-partition `status` list names partition by partition.
FIT_WROTE_BLOCKS = (0, 4, 5, 6)


def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def _strided_partitions(who, part_first, part_rows, row_step, n):
    """Partitions given as (first row, rows, common row step) of n rows, checked.  Returns (K, step, the largest partition's rows,
    part_first and part_rows as int64 arrays for the C ABI)."""
    first, rows = [int(v) for v in part_first], [int(v) for v in part_rows]
    K, step = len(first), int(row_step)
    if len(rows) != K or K == 0 or step < 1:
        raise ValueError("%s: part_first / part_rows must have K >= 1 entries each, row_step >= 1" % who)
    for f, r in zip(first, rows):
        if f < 0 or r < 0 or (r > 0 and f + (r - 1) * step >= n):
            raise ValueError("%s: partition outside the %d rows" % (who, n))
    return K, step, max(rows), _i64(first), _i64(rows)


def _offset_partitions(who, part_offsets, n, ascending_from_zero=False):
    """Partitions given as K + 1 offsets into n rows (or into an order of n entries), checked: the two ends within 0 .. n, and with
    ascending_from_zero (the Cox fit, whose segments tile the order) a start at 0 and no decreasing step as well.  Returns (K, the
    largest partition's rows, the offsets as an int64 array for the C ABI)."""
    offs = [int(v) for v in part_offsets]
    K = len(offs) - 1
    if ascending_from_zero:
        if K < 1 or offs[0] != 0 or offs[-1] > n or any(offs[k + 1] < offs[k] for k in range(K)):
            raise ValueError("%s: part_offsets must be K+1 non-decreasing ints from 0 within the order" % who)
    elif offs[0] < 0 or offs[-1] > n or K < 1:
        raise ValueError("%s: part_offsets out of range" % who)
    return K, max(offs[k + 1] - offs[k] for k in range(K)), _i64(offs)


class _FitOut:
    """What a per-partition fit of K partitions with pe coefficients writes: coef / Sig_invMcoef [K, pe] and Sig_inv [K, pe, pe] on the
    device, n_iter / status / loglik on the host, and with a log-link `family` (a GLM_FAMILIES record) its own host lists
    (family.fit_lists).  `args` is the run of output arguments every dlsa_*_fit_* entry takes, in the C ABI's order; result(rc) is the
    wrappers' result dict."""

    def __init__(self, K, pe, device, family=None):
        self.coef = torch.empty((K, pe), dtype=torch.float64, device=device)
        self.smc = torch.empty((K, pe), dtype=torch.float64, device=device)
        self.sig = torch.empty((K, pe, pe), dtype=torch.float64, device=device)
        self.host = {"n_iter": (ctypes.c_int * K)(), "status": (ctypes.c_int * K)(), "loglik": (ctypes.c_double * K)()}
        if family is not None:
            self.host.update({k: (ctypes.c_double * K)() for k in family.fit_lists})
        self.args = (_ptr(self.coef), _ptr(self.sig), _ptr(self.smc)) + tuple(self.host.values())

    def result(self, rc, df_rows=None):
        """df_rows: the partitions' row counts of a family whose result carries `df` = rows - pe per partition (what the Pearson
        estimate of the dispersion divides by)."""
        if rc not in FIT_WROTE_BLOCKS:
            check(rc)
        r = {"coef": self.coef, "Sig_invMcoef": self.smc, "Sig_inv": self.sig, **{k: list(v) for k, v in self.host.items()}, "rc": rc}
        if df_rows is not None:
            r["df"] = [int(m) - self.coef.shape[1] for m in df_rows]
        return r


def _pass_out(pe, n, device, want_H, want_w, family=None, want=None):
    """The outputs of one pass at a fixed beta, in the order the pass wrappers return them: (H [pe, pe] or None, g [pe], loglik [1],
    w [n] or None), and with a log-link `family` (a GLM_FAMILIES record) its extra outputs family.pass_extra, each asked for by its flag
    in `want` (or by want_w): NB2's (..., mu [n] or None, theta_terms [3] or None), Gamma's and Tweedie's (..., stats [2] or None)."""
    def new(shape, want=True):
        return torch.empty(shape, dtype=torch.float64, device=device) if want else None
    out = (new((pe, pe), want_H), new((pe,)), new((1,)), new((n,), want_w))
    if family is None:
        return out
    return out + tuple([new((n if size is None else size,), want_w if flag == "want_w" else want[flag]) for size, flag in family.pass_extra])


def _alpha_positive(who, alpha, other):
    """The dispersion of an NB2 pass: a positive finite float."""
    alpha = float(alpha)
    if not 0.0 < alpha < float("inf"):
        raise ValueError("%s: alpha must be positive and finite (alpha = 0 is %s)" % (who, other))
    return alpha


def _alpha_fixed(who, alpha, other):
    """The dispersion argument of an NB2 fit as the C ABI takes it: 0.0 for None (estimate it), else a positive finite float."""
    if alpha is None:
        return 0.0
    alpha = float(alpha)
    if alpha == 0.0:
        raise ValueError("%s: alpha = 0 is the Poisson model: use %s" % (who, other))
    if not 0.0 < alpha < float("inf"):
        raise ValueError("%s: a fixed alpha must be positive and finite" % who)
    return alpha


def _dispersion_positive(who, dispersion):
    """The dispersion of a Gamma pass: a positive finite float."""
    dispersion = float(dispersion)
    if not 0.0 < dispersion < float("inf"):
        raise ValueError("%s: dispersion must be positive and finite" % who)
    return dispersion


def _dispersion_fixed(who, dispersion):
    """The dispersion argument of a Gamma fit as the C ABI takes it: 0.0 for None (estimate it), else a positive finite float."""
    return 0.0 if dispersion is None else _dispersion_positive(who, dispersion)


def tweedie_power(who, power):
    """The variance power of a Tweedie entry: a float strictly between 1 and 2 (ValueError otherwise; NaN fails)."""
    power = float(power)
    if not 1.0 < power < 2.0:
        raise ValueError("%s: power must lie strictly between 1 and 2, got %r" % (who, power))
    return power


GAMMA_LISTS = ("dispersion", "pearson", "deviance")


class _Scalar(NamedTuple):
    """One scalar parameter of a log-link family: its keyword name and its checks (who, value) -> the double the C ABI takes, at a pass
    and at a fit."""
    name: str
    at_pass: Callable
    at_fit: Callable


class _Family(NamedTuple):
    """What varies between the log-link families behind the {,onehot_}<name>_{pass,fit_ex} wrappers; everything else is the four bodies
    below.  The C entries are dlsa_[onehot_]<name>_{workspace_bytes,pass_f64,fit_f64}."""
    name: str
    scalars: tuple = ()         # in the C ABI's order: after beta in a pass, after K, [p, icpt] in a fit
    pass_extra: tuple = ()      # a pass's outputs after w: (length, or None for n; the want_* flag that asks for it)
    fit_lists: tuple = ()       # a fit's host lists after loglik, doubles
    df: bool = False            # a fit's result carries `df`
    other: Optional[str] = None  # the family a refused parameter value belongs to: the checks get `who` with its name as a third argument

    def checked(self, who, values, fit):
        """The scalars `values` as the C ABI takes them, checked in its order."""
        other = (who.replace(self.name, self.other),) if self.other else ()
        return tuple([(s.at_fit if fit else s.at_pass)(who, v, *other) for s, v in zip(self.scalars, values)])


_DISPERSION = _Scalar("dispersion", _dispersion_positive, _dispersion_fixed)
GLM_FAMILIES = {f.name: f for f in (
    _Family("poisson"),
    _Family("negbin", (_Scalar("alpha", _alpha_positive, _alpha_fixed),), ((None, "want_w"), (3, "want_theta")),
            ("alpha", "alpha_info", "pearson"), other="poisson"),
    _Family("gamma", (_DISPERSION,), ((2, "want_stats"),), GAMMA_LISTS, df=True),
    _Family("tweedie", (_Scalar("power", tweedie_power, tweedie_power), _DISPERSION), ((2, "want_stats"),), GAMMA_LISTS, df=True),
    # the two binary links beside the logit (include/dlsa_hip_binary.h): dense entries only so far
    _Family("probit"),
    _Family("cloglog"),
)}


def _glm_pass(fam, X, y, beta, scalars, offset, fit_intercept, want_H, want_w, **want):
    """The body of <name>_pass: dlsa_<name>_pass_f64 on the rows X."""
    family, who = fam.name, fam.name + "_pass"
    lib = _lib.load()
    _require_gpu(X, y, beta, offset)
    _f64(X, "X"); _f64(y, "y"); _f64(beta, "beta"); _f64(offset, "offset")
    n, p = X.shape
    icpt = 1 if fit_intercept else 0
    pe = p + icpt
    if n < 1 or y.numel() != n or beta.numel() != pe or (offset is not None and offset.numel() != n):
        raise ValueError("%s: need n >= 1 rows, y and offset with n = %d and beta with %d elements" % (who, n, pe))
    scalars = fam.checked(who, scalars, fit=False)
    out = _pass_out(pe, n, X.device, want_H, want_w, fam, want)
    ws = _workspace(getattr(lib, "dlsa_%s_workspace_bytes" % family)(n, p, icpt, 1), X.device)
    check(getattr(lib, "dlsa_%s_pass_f64" % family)(_ptr(X), _rowmajor(X), _ptr(y), _ptr(offset), _ptr(beta), *scalars, n, p, icpt, _ptr(out[0]),
                                                    pe, *[_ptr(t) for t in out[1:]], _ptr(ws), ws.numel(), _stream()))
    return out


def _glm_fit(fam, X, y, part_first, part_rows, row_step, offset, fit_intercept, scalars, tol, max_iter):
    """The body of <name>_fit_ex: dlsa_<name>_fit_f64 on strided partitions of the rows X."""
    family, who = fam.name, fam.name + "_fit_ex"
    lib = _lib.load()
    _require_gpu(X, y, offset)
    _f64(X, "X"); _f64(y, "y"); _f64(offset, "offset")
    n, p = X.shape
    if y.numel() != n or (offset is not None and offset.numel() != n):
        raise ValueError("%s: y and offset must have n = %d elements" % (who, n))
    scalars = fam.checked(who, scalars, fit=True)
    K, step, max_rows, c_first, c_rows = _strided_partitions(who, part_first, part_rows, row_step, n)
    icpt = 1 if fit_intercept else 0
    out = _FitOut(K, p + icpt, X.device, fam)
    ws = _workspace(getattr(lib, "dlsa_%s_workspace_bytes" % family)(max_rows, p, icpt, step), X.device)
    rc = getattr(lib, "dlsa_%s_fit_f64" % family)(_ptr(X), _rowmajor(X), _ptr(y), _ptr(offset), c_first, c_rows, step, K, p, icpt, *scalars,
                                                  tol, max_iter, *out.args, _ptr(ws), ws.numel(), _stream())
    return out.result(rc, c_rows if fam.df else None)


def irls_fit_ex(X, y, part_first, part_rows, row_step=1, fit_intercept=False, tol=1e-13, max_iter=100):
    """irls_fit without copies of the shard: partition k = rows part_first[k] + j * row_step, j < part_rows[k] (a strided
    view: partition_id = i % K is part_first = 0..K-1, row_step = K), and an IMPLICIT intercept column (fit_intercept:
    results have p + 1 columns, intercept first).  Same result dict as irls_fit."""
    lib = _lib.load()
    _require_gpu(X, y)
    _f64(X, "X"); _f64(y, "y")
    n, p = X.shape
    if y.numel() != n:
        raise ValueError("irls_fit_ex: y must have n = %d elements" % n)
    K, step, max_rows, c_first, c_rows = _strided_partitions("irls_fit_ex", part_first, part_rows, row_step, n)
    icpt = 1 if fit_intercept else 0
    out = _FitOut(K, p + icpt, X.device)
    ws = _workspace(lib.dlsa_irls_ex_workspace_bytes(max_rows, p, icpt, step), X.device)
    rc = lib.dlsa_irls_fit_ex_f64(_ptr(X), _rowmajor(X), _ptr(y), c_first, c_rows, step, K, p, icpt, tol, max_iter, *out.args,
                                  _ptr(ws), ws.numel(), _stream())
    return out.result(rc)


def irls_fit(X, y, part_offsets, tol=1e-13, max_iter=100):
    """Per-partition exact-MLE fit + local quadratic approximation (dlsa/models.py:110-131).
    part_offsets: K+1 ints; partition k = rows [off[k], off[k+1]).  Returns a dict with
    coef [K,p], Sig_invMcoef [K,p], Sig_inv [K,p,p] (device) and n_iter/status/loglik (host)."""
    lib = _lib.load()
    _require_gpu(X, y)
    _f64(X, "X"); _f64(y, "y")
    n, p = X.shape
    if y.numel() != n:
        raise ValueError("irls_fit: y must have n = %d elements" % n)
    K, max_rows, c_offs = _offset_partitions("irls_fit", part_offsets, n)
    out = _FitOut(K, p, X.device)
    ws = _workspace(lib.dlsa_irls_workspace_bytes(max_rows, p), X.device)
    rc = lib.dlsa_irls_fit_f64(_ptr(X), _rowmajor(X), _ptr(y), c_offs, K, p, tol, max_iter, *out.args, _ptr(ws), ws.numel(), _stream())
    return out.result(rc)


def _cox_args(X, time, event, order):
    _require_gpu(X, time, event, order)
    _f64(X, "X"); _f64(time, "time"); _f64(event, "event"); _f64(order, "order", torch.int64)
    n = X.shape[0]
    if time.numel() != n or event.numel() != n:
        raise ValueError("cox: time and event must have n = %d elements" % n)
    return X.shape[1]


COX_TIES = {"breslow": 0, "efron": 1}      # include/dlsa_hip.h: DLSA_COX_TIES_*


def cox_ties(ties):
    """The C ABI's code of a tie method name ("breslow" or "efron", any letter case); ValueError for anything else."""
    code = COX_TIES.get(ties.lower()) if isinstance(ties, str) else None
    if code is None:
        raise ValueError("cox: ties must be 'breslow' or 'efron', got %r" % (ties,))
    return code


def cox_strata(strata, n):
    """Argument check of the stratum codes, with no GPU work: None, or an integer tensor with one code per row of X.  TypeError
    for anything but an integer tensor, ValueError for a wrong length.  Returns its argument."""
    if strata is None:
        return None
    if not torch.is_tensor(strata) or strata.dtype.is_floating_point or strata.dtype.is_complex or strata.dtype == torch.bool:
        raise TypeError("cox: strata must be an integer tensor of stratum codes, got %s"
                        % (strata.dtype if torch.is_tensor(strata) else type(strata).__name__))
    if strata.dim() != 1 or strata.numel() != n:
        raise ValueError("cox: strata must have n = %d elements" % n)
    return strata


def cox_strata_codes(strata, device):
    """The C ABI's form of checked stratum codes: contiguous int32 on X's device.  An int32 tensor passes as it is; any other
    integer type is range-checked (one device reduction) and converted, so callers that loop convert once and pass the result."""
    if strata is None:
        return None
    if strata.device != device:
        raise RuntimeError("cox: strata must be on X's device %s, got %s" % (device, strata.device))
    if strata.dtype != torch.int32:
        # (only equality of codes is read; codes within int32 keep their value)
        lo, hi = torch.aminmax(strata) if strata.numel() else (strata.new_zeros(()), strata.new_zeros(()))
        if int(hi) > 2 ** 31 - 1 or int(lo) < -2 ** 31:
            raise ValueError("cox: stratum codes must fit int32")
        strata = strata.to(torch.int32)
    return strata.contiguous()


def cox_pass(X, time, event, order, beta, want_w=False, ties="breslow", strata=None):
    """One Cox partition at a fixed beta (dlsa_cox_pass_strata_f64): `order` [m] int64 holds the partition's absolute row
    indices in DESCENDING time.  ties: "breslow" or "efron".  strata: None, or an integer tensor with one stratum code per row
    of X; `order` then lists the rows grouped by stratum, descending time inside each (models.cox_order), and every stratum
    has its own baseline hazard.  Returns (H [p,p] observed information, g [p] score, loglik [1] log partial likelihood,
    w [m] or None -- the weights of the rows order[i] in H's X'diag(w)X term), all of the chosen method."""
    code = cox_ties(ties)
    cox_strata(strata, X.shape[0])
    lib = _lib.load()
    p = _cox_args(X, time, event, order)
    strata = cox_strata_codes(strata, X.device)
    _f64(beta, "beta")
    m = order.numel()
    if m < 1 or beta.numel() != p:
        raise ValueError("cox_pass: need at least one row and beta with p = %d entries" % p)
    H, g, ll, w = out = _pass_out(p, m, X.device, True, want_w)
    ws = _workspace(lib.dlsa_cox_strata_workspace_bytes(m, p, code, 0 if strata is None else 1), X.device)
    check(lib.dlsa_cox_pass_strata_f64(_ptr(X), _rowmajor(X), _ptr(time), _ptr(event), _ptr(strata), _ptr(order), m, p, code, _ptr(beta),
                                       _ptr(H), p, _ptr(g), _ptr(ll), _ptr(w), _ptr(ws), ws.numel(), _stream()))
    return out


def cox_fit(X, time, event, order, part_offsets, tol=1e-13, max_iter=100, ties="breslow", strata=None):
    """Per-partition Cox fit (dlsa_cox_fit_strata_f64): partition k = rows order[off[k]:off[k+1]] (each segment in descending
    time; with `strata`, as cox_pass: grouped by stratum, descending time inside each).  ties: "breslow" or "efron".  Same
    result dict as irls_fit; `loglik` holds the log partial likelihood of the chosen method at coef."""
    code = cox_ties(ties)
    cox_strata(strata, X.shape[0])
    lib = _lib.load()
    p = _cox_args(X, time, event, order)
    strata = cox_strata_codes(strata, X.device)
    K, max_rows, c_offs = _offset_partitions("cox_fit", part_offsets, order.numel(), ascending_from_zero=True)
    out = _FitOut(K, p, X.device)
    ws = _workspace(lib.dlsa_cox_strata_workspace_bytes(max_rows, p, code, 0 if strata is None else 1), X.device)
    rc = lib.dlsa_cox_fit_strata_f64(_ptr(X), _rowmajor(X), _ptr(time), _ptr(event), _ptr(strata), _ptr(order), c_offs, K, p, code, tol,
                                     max_iter, *out.args, _ptr(ws), ws.numel(), _stream())
    return out.result(rc)


def poisson_pass(X, y, beta, offset=None, fit_intercept=False, want_H=True, want_w=False):
    """One Poisson partition at a fixed beta (dlsa_poisson_pass_f64): eta = [1 | X] beta + offset, mu = exp(eta).  fit_intercept: the
    ones column is implicit -- beta, g and H have p + 1 entries, intercept first.  Returns (H [pe,pe] = [1 | X]' diag(mu) [1 | X] or
    None, g [pe] = [1 | X]'(y - mu), loglik [1] = sum y eta - mu - lgamma(y + 1), w [n] = mu or None)."""
    return _glm_pass(GLM_FAMILIES["poisson"], X, y, beta, (), offset, fit_intercept, want_H, want_w)


def poisson_fit_ex(X, y, part_first, part_rows, row_step=1, offset=None, fit_intercept=False, tol=1e-13, max_iter=100):
    """Per-partition Poisson fit (dlsa_poisson_fit_f64): partition k = rows part_first[k] + j * row_step, j < part_rows[k] (a strided
    view: partition_id = i % K is part_first = 0..K-1, row_step = K), log link, optional offset [n], implicit intercept with
    fit_intercept.  Same result dict as irls_fit_ex; `loglik` is the full log-likelihood at coef."""
    return _glm_fit(GLM_FAMILIES["poisson"], X, y, part_first, part_rows, row_step, offset, fit_intercept, (), tol, max_iter)


def negbin_pass(X, y, beta, alpha, offset=None, fit_intercept=False, want_H=True, want_w=False, want_theta=False):
    """One negative-binomial (NB2) partition at a fixed beta and alpha > 0 (dlsa_negbin_pass_f64): eta = [1 | X] beta + offset,
    mu = exp(eta), Var y = mu + alpha mu^2.  Arguments as poisson_pass.  Returns (H [pe,pe] = [1 | X]' diag(mu / (1 + alpha mu)) [1 | X]
    or None, g [pe], loglik [1] = the full log-likelihood, w [n] = mu / (1 + alpha mu) or None, mu [n] or None (with want_w),
    theta_terms [3] = (s, i, pearson) at theta = 1 / alpha or None (with want_theta))."""
    return _glm_pass(GLM_FAMILIES["negbin"], X, y, beta, (alpha,), offset, fit_intercept, want_H, want_w, want_theta=want_theta)


def negbin_fit_ex(X, y, part_first, part_rows, row_step=1, offset=None, fit_intercept=False, alpha=None, tol=1e-13, max_iter=100):
    """Per-partition negative-binomial fit (dlsa_negbin_fit_f64): partitions, offset and intercept as poisson_fit_ex.  alpha=None
    estimates the dispersion of every partition (0 for a partition that is not overdispersed: its block is the Poisson block);
    alpha > 0 fits beta at that fixed dispersion.  The result dict of poisson_fit_ex plus the per-partition lists `alpha`,
    `alpha_info` (the information about log alpha) and `pearson`; `loglik` is the full log-likelihood at (coef, alpha)."""
    return _glm_fit(GLM_FAMILIES["negbin"], X, y, part_first, part_rows, row_step, offset, fit_intercept, (alpha,), tol, max_iter)


def gamma_pass(X, y, beta, dispersion=1.0, offset=None, fit_intercept=False, want_H=True, want_w=False, want_stats=False):
    """One Gamma partition (log link) at a fixed beta and dispersion > 0 (dlsa_gamma_pass_f64): eta = [1 | X] beta + offset, mu = exp(eta),
    r = y / mu.  Arguments as poisson_pass.  Returns (H [pe,pe] = [1 | X]' diag(r) [1 | X] / dispersion or None, g [pe] = [1 | X]'(r - 1)
    / dispersion, loglik [1] = the full log-likelihood at that dispersion, w [n] = r or None, stats [2] = (Pearson sum (r - 1)^2,
    deviance 2 sum (r - 1 - log r)) or None (with want_stats))."""
    return _glm_pass(GLM_FAMILIES["gamma"], X, y, beta, (dispersion,), offset, fit_intercept, want_H, want_w, want_stats=want_stats)


def gamma_fit_ex(X, y, part_first, part_rows, row_step=1, offset=None, fit_intercept=False, dispersion=None, tol=1e-13, max_iter=100):
    """Per-partition Gamma fit with a log link (dlsa_gamma_fit_f64): partitions, offset and intercept as poisson_fit_ex.
    dispersion=None estimates every partition's own dispersion (Pearson: P / (rows - pe)); dispersion > 0 gives every block that
    fixed dispersion.  The result dict of poisson_fit_ex -- Sig_inv is the information divided by the dispersion used, `loglik` the
    full log-likelihood at (coef, that dispersion) -- plus the per-partition lists `dispersion`, `pearson`, `deviance` and `df`."""
    return _glm_fit(GLM_FAMILIES["gamma"], X, y, part_first, part_rows, row_step, offset, fit_intercept, (dispersion,), tol, max_iter)


def tweedie_pass(X, y, beta, power, dispersion=1.0, offset=None, fit_intercept=False, want_H=True, want_w=False, want_stats=False):
    """One Tweedie partition (log link, Var y = dispersion * mu^power, 1 < power < 2) at a fixed beta and dispersion > 0
    (dlsa_tweedie_pass_f64): eta = [1 | X] beta + offset, mu = exp(eta), a = mu^(1 - power), b = mu^(2 - power).  Arguments as
    poisson_pass, y >= 0.  Returns (H [pe,pe] = [1 | X]' diag(w) [1 | X] / dispersion or None, g [pe] = [1 | X]'(y a - b) / dispersion,
    loglik [1] = the QUASI-log-likelihood sum (y a / (1 - power) - b / (2 - power)) / dispersion -- the series factor of the density
    is not computed, so it compares values of beta at one (power, dispersion) only --, w [n] = (power - 1) y a + (2 - power) b or
    None, stats [2] = (Pearson sum (y - mu)^2 mu^-power, deviance) or None (with want_stats))."""
    return _glm_pass(GLM_FAMILIES["tweedie"], X, y, beta, (power, dispersion), offset, fit_intercept, want_H, want_w, want_stats=want_stats)


def tweedie_fit_ex(X, y, part_first, part_rows, row_step=1, offset=None, fit_intercept=False, power=1.5, dispersion=None, tol=1e-13,
                   max_iter=100):
    """Per-partition Tweedie fit with a log link at the variance power `power` (dlsa_tweedie_fit_f64; 1 < power < 2, given, not
    estimated): partitions, offset and intercept as poisson_fit_ex, dispersion as gamma_fit_ex.  The result dict of gamma_fit_ex
    (`dispersion`, `pearson`, `deviance`, `df`); `loglik` is the quasi-log-likelihood at (coef, the dispersion used)."""
    return _glm_fit(GLM_FAMILIES["tweedie"], X, y, part_first, part_rows, row_step, offset, fit_intercept, (power, dispersion), tol, max_iter)


def probit_pass(X, y, beta, offset=None, fit_intercept=False, want_H=True, want_w=False):
    """One probit partition at a fixed beta (dlsa_probit_pass_f64, include/dlsa_hip_binary.h): y [n] holds 0.0 / 1.0, P(y = 1) =
    Phi(eta), eta = [1 | X] beta + offset.  Arguments as poisson_pass.  Returns (H [pe,pe] = the OBSERVED information [1 | X]' diag(w)
    [1 | X] or None, g [pe], loglik [1] = sum log Phi((2y - 1) eta) -- NaN when a response is not 0 or 1 --, w [n] or None)."""
    return _glm_pass(GLM_FAMILIES["probit"], X, y, beta, (), offset, fit_intercept, want_H, want_w)


def probit_fit_ex(X, y, part_first, part_rows, row_step=1, offset=None, fit_intercept=False, tol=1e-13, max_iter=100):
    """Per-partition probit fit (dlsa_probit_fit_f64): partitions, offset and intercept as poisson_fit_ex, y in {0, 1}.  The result dict
    of poisson_fit_ex; Sig_inv is the observed information at coef.  A partition with an intercept and a single response value is
    EMPTY with the all-zero block."""
    return _glm_fit(GLM_FAMILIES["probit"], X, y, part_first, part_rows, row_step, offset, fit_intercept, (), tol, max_iter)


def cloglog_pass(X, y, beta, offset=None, fit_intercept=False, want_H=True, want_w=False):
    """One complementary log-log partition at a fixed beta (dlsa_cloglog_pass_f64, include/dlsa_hip_binary.h): y [n] holds 0.0 / 1.0,
    P(y = 1) = 1 - exp(-e^eta), eta = [1 | X] beta + offset (offset = log interval length or exposure, as in poisson_pass).  Arguments and
    results as probit_pass; on rows with y = 0 it is poisson_pass bit for bit."""
    return _glm_pass(GLM_FAMILIES["cloglog"], X, y, beta, (), offset, fit_intercept, want_H, want_w)


def cloglog_fit_ex(X, y, part_first, part_rows, row_step=1, offset=None, fit_intercept=False, tol=1e-13, max_iter=100):
    """Per-partition complementary log-log fit (dlsa_cloglog_fit_f64): as probit_fit_ex."""
    return _glm_fit(GLM_FAMILIES["cloglog"], X, y, part_first, part_rows, row_step, offset, fit_intercept, (), tol, max_iter)


MULTINOMIAL_MAX_CLASSES = 8


def _class_count(who, classes, coefficients, formula):
    """The body of multinomial_classes / ordinal_classes: `classes` as an int in 2 .. 8 whose coefficients(classes), named `formula`
    in the refusal, do not exceed the solver's 2048 (ValueError otherwise)."""
    if isinstance(classes, bool) or int(classes) != classes:
        raise ValueError("%s: classes must be an integer, got %r" % (who, classes))
    classes = int(classes)
    if not 2 <= classes <= MULTINOMIAL_MAX_CLASSES:
        raise ValueError("%s: classes must lie in 2 .. %d, got %d" % (who, MULTINOMIAL_MAX_CLASSES, classes))
    if coefficients(classes) > 2048:
        raise ValueError("%s: %s = %d coefficients exceed the solver's 2048" % (who, formula, coefficients(classes)))
    return classes


def multinomial_classes(who, classes, pe):
    """The class count of a multinomial entry: an int in 2 .. 8 with (classes - 1) * pe <= 2048 coefficients (ValueError otherwise)."""
    return _class_count(who, classes, lambda c: (c - 1) * pe, "(classes - 1) * (p + intercept)")


def ordinal_classes(who, classes, p):
    """The class count of an ordinal entry: an int in 2 .. 8 with (classes - 1) + p <= 2048 coefficients (ValueError otherwise)."""
    return _class_count(who, classes, lambda c: c - 1 + p, "(classes - 1) + p")


class _ClassFamily(NamedTuple):
    """What varies between the families whose response is a class code behind the {,onehot_}<name>_fit_ex wrappers.  The C entries
    are dlsa_[onehot_]<name>_{workspace_bytes,fit_f64}."""
    name: str
    classes: Callable           # (who, classes, pe) -> the checked class count
    d: Callable                 # (classes, pe) -> the coefficients of a partition's block
    intercept: bool             # the dense entries take an intercept argument after p


CLASS_FAMILIES = {f.name: f for f in (
    _ClassFamily("multinomial", multinomial_classes, lambda c, pe: (c - 1) * pe, True),
    _ClassFamily("ordinal", ordinal_classes, lambda c, pe: c - 1 + pe, False),
)}


def _class_fit(fam, rows, y, part_first, part_rows, row_step, classes, fit_intercept, tol, max_iter):
    """The body of <name>_fit_ex (rows: the dense X) and onehot_<name>_fit_ex (rows: (plan, num, codes)): dlsa_[onehot_]<name>_fit_f64
    on strided partitions of the rows."""
    onehot = isinstance(rows, tuple)
    entry = ("onehot_" if onehot else "") + fam.name
    who = entry + "_fit_ex"
    lib = _lib.load()
    if onehot:
        n = _oh_poisson_rows(*rows, y, None, who)
        pe, device, rows_at, plan_at, shape = rows[0].p, y.device, (rows[0]._h, *_oh_args(*rows)), (rows[0]._h,), ()
    else:
        _require_gpu(rows, y)
        _f64(rows, "X"); _f64(y, "y")
        n, p = rows.shape
        if y.numel() != n:
            raise ValueError("%s: y must have n = %d elements" % (who, n))
        shape = (p, 1 if fit_intercept else 0) if fam.intercept else (p,)
        pe, device, rows_at, plan_at = sum(shape), rows.device, (_ptr(rows), _rowmajor(rows)), ()
    if classes is None:
        raise ValueError("%s: classes (the number of classes, 2 .. %d) is required" % (who, MULTINOMIAL_MAX_CLASSES))
    classes = fam.classes(who, classes, pe)
    K, step, max_rows, c_first, c_rows = _strided_partitions(who, part_first, part_rows, row_step, n)
    out = _FitOut(K, fam.d(classes, pe), device)
    ws = _workspace(getattr(lib, "dlsa_%s_workspace_bytes" % entry)(*plan_at, max_rows, *shape, classes, step), device)
    rc = getattr(lib, "dlsa_%s_fit_f64" % entry)(*rows_at, _ptr(y), c_first, c_rows, step, K, *shape, classes, tol, max_iter, *out.args,
                                                 _ptr(ws), ws.numel(), _stream())
    return out.result(rc)


def multinomial_pass(X, y, theta, classes, fit_intercept=False, want_H=True, want_prob=False):
    """One multinomial logistic (softmax) partition at a fixed theta (dlsa_multinomial_pass_f64): y [n] holds the class codes
    0 .. classes - 1 as fp64, class 0 is the reference (eta_0 = 0), J = classes - 1.  theta [J * pe] is class-major, [beta_1 | ... |
    beta_J], intercept first in each with fit_intercept (pe = p + 1).  Returns (H [J pe, J pe] with the blocks H_jk = [1 | X]'
    diag(p_j (delta_jk - p_k)) [1 | X] or None, g [J pe] with g_j = [1 | X]'(1[y = j] - p_j), loglik [1] = sum log p_y -- NaN when a
    response is no class code --, P [J, n] the probabilities of the non-reference classes or None)."""
    lib = _lib.load()
    _require_gpu(X, y, theta)
    _f64(X, "X"); _f64(y, "y"); _f64(theta, "theta")
    n, p = X.shape
    icpt = 1 if fit_intercept else 0
    classes = multinomial_classes("multinomial_pass", classes, p + icpt)
    d = (classes - 1) * (p + icpt)
    if n < 1 or y.numel() != n or theta.numel() != d:
        raise ValueError("multinomial_pass: need n >= 1 rows, y with n = %d and theta with %d elements" % (n, d))
    H, g, ll, _ = _pass_out(d, n, X.device, want_H, False)
    ld = (n + 31) // 32 * 32                      # 256-byte aligned class rows
    P = torch.empty((classes - 1, ld), dtype=torch.float64, device=X.device) if want_prob else None
    ws = _workspace(lib.dlsa_multinomial_workspace_bytes(n, p, icpt, classes, 1), X.device)
    check(lib.dlsa_multinomial_pass_f64(_ptr(X), _rowmajor(X), _ptr(y), _ptr(theta), classes, n, p, icpt, _ptr(H), d, _ptr(g), _ptr(ll),
                                        _ptr(P), ld, _ptr(ws), ws.numel(), _stream()))
    return H, g, ll, (P[:, :n] if want_prob else None)


def multinomial_fit_ex(X, y, part_first, part_rows, row_step=1, classes=None, fit_intercept=False, tol=1e-13, max_iter=100):
    """Per-partition multinomial logistic fit (dlsa_multinomial_fit_f64): partitions and intercept as poisson_fit_ex, y and the
    class-major layout as multinomial_pass; `classes` (2 .. 8) is required -- a partition cannot discover the classes it lacks, and one
    that lacks a class is refused with the partition and the class named, as is a response that is no class code.  Same result dict
    as irls_fit_ex with J * pe columns; `loglik` is the log-likelihood at coef.  classes = 2 is the logistic fit."""
    return _class_fit(CLASS_FAMILIES["multinomial"], X, y, part_first, part_rows, row_step, classes, fit_intercept, tol, max_iter)


def ordinal_pass(X, y, theta, classes, want_H=True, want_w=False):
    """One ordinal (proportional-odds) partition at a fixed theta (dlsa_ordinal_pass_f64, include/dlsa_hip_ordinal.h): y [n] holds
    the class codes 0 .. classes - 1 as fp64, J = classes - 1, logit P(y <= j) = alpha_{j+1} - x'beta.  theta [J + p] = [alpha_1 ..
    alpha_J | beta], cutpoints first; there is no intercept argument, the cutpoints are the intercepts.  Returns (H [d, d] the
    observed information or None, g [d] the score, loglik [1] = sum log P(y_i) -- NaN when the cutpoints are not strictly increasing
    or a response is no class code --, w [n] = -d2l/deta2 per row or None)."""
    lib = _lib.load()
    _require_gpu(X, y, theta)
    _f64(X, "X"); _f64(y, "y"); _f64(theta, "theta")
    n, p = X.shape
    classes = ordinal_classes("ordinal_pass", classes, p)
    d = classes - 1 + p
    if n < 1 or y.numel() != n or theta.numel() != d:
        raise ValueError("ordinal_pass: need n >= 1 rows, y with n = %d and theta with %d elements" % (n, d))
    H, g, ll, w = _pass_out(d, n, X.device, want_H, want_w)
    ws = _workspace(lib.dlsa_ordinal_workspace_bytes(n, p, classes, 1), X.device)
    check(lib.dlsa_ordinal_pass_f64(_ptr(X), _rowmajor(X), _ptr(y), _ptr(theta), classes, n, p, _ptr(H), d, _ptr(g), _ptr(ll), _ptr(w),
                                    _ptr(ws), ws.numel(), _stream()))
    return H, g, ll, w


def ordinal_fit_ex(X, y, part_first, part_rows, row_step=1, classes=None, tol=1e-13, max_iter=100):
    """Per-partition ordinal (proportional-odds) fit (dlsa_ordinal_fit_f64): partitions as poisson_fit_ex, y and the layout
    [alpha_1 .. alpha_J | beta] as ordinal_pass; `classes` (2 .. 8) is required -- a partition cannot discover the classes it lacks,
    and one that lacks a class is refused with the partition and the class named, as is a response that is no class code.  Same result
    dict as multinomial_fit_ex with J + p columns; `loglik` is the log-likelihood at coef.  classes = 2 is the logistic fit with
    theta = [-intercept | beta]."""
    return _class_fit(CLASS_FAMILIES["ordinal"], X, y, part_first, part_rows, row_step, classes, False, tol, max_iter)


def negbin_special(theta, y):
    """The dispersion kernel's special functions (dlsa_negbin_special_f64, a test entry): theta [m] > 0, y [m] >= 0 on the GPU;
    returns [m, 4] = psi(theta), psi'(theta), psi(y + theta) - psi(theta), lgamma(y + theta) - lgamma(theta) - y log(theta)."""
    lib = _lib.load()
    _require_gpu(theta, y)
    _f64(theta, "theta"); _f64(y, "y")
    m = theta.numel()
    if m < 1 or y.numel() != m:
        raise ValueError("negbin_special: theta and y must have the same number (>= 1) of elements")
    theta, y = theta.contiguous(), y.contiguous()
    out = torch.empty((m, 4), dtype=torch.float64, device=theta.device)
    check(lib.dlsa_negbin_special_f64(_ptr(theta), _ptr(y), m, _ptr(out), _stream()))
    return out


def sum_blocks(coef, smc, sig, mask=None):
    """[sum Sig_inv | sum Sig_invMcoef | sum coef]: the rank's all-reduce message (dlsa.py:30-34)."""
    lib = _lib.load()
    _require_gpu(coef, smc, sig)
    _f64(coef, "coef"); _f64(smc, "Sig_invMcoef")
    if sig.dtype != torch.float64:
        raise TypeError("Sig_inv must be float64, got %s" % sig.dtype)
    K, p = coef.shape
    if tuple(smc.shape) != (K, p) or tuple(sig.shape) != (K, p, p):
        raise ValueError("sum_blocks: expected coef / Sig_invMcoef [K, p] and Sig_inv [K, p, p]")
    out = torch.empty((p * p + 2 * p,), dtype=torch.float64, device=coef.device)
    cmask = (ctypes.c_int * K)(*[int(v) for v in mask]) if mask is not None else None
    check(lib.dlsa_sum_blocks_f64(_ptr(coef.contiguous()), _ptr(sig.contiguous()), _ptr(smc.contiguous()),
                                  K, p, cmask, _ptr(out), _stream()))
    return out


def spd_solve(S, v):
    """theta = S^{-1} v by device Cholesky (the WLS combine, dlsa/dlsa.py:48-49)."""
    lib = _lib.load()
    _require_gpu(S, v)
    _f64(S, "S")
    v = _f64(v.contiguous(), "v")
    p = S.shape[0]
    if S.dim() != 2 or S.shape[1] != p or v.numel() != p:
        raise ValueError("spd_solve: S must be p x p and v of length p")
    theta = torch.empty((p,), dtype=torch.float64, device=S.device)
    nb = lib.dlsa_solve_workspace_bytes(p)
    ws = _workspace(nb, S.device)
    check(lib.dlsa_spd_solve_f64(_ptr(S), _rowmajor(S), _ptr(v), p, _ptr(theta),
                                 _ptr(ws), ws.numel(), _stream()))
    return theta


NEWTON_ROUTES = {"factor": 0, "reuse": 1, "inverse": 2, "sweep": 3, "sweep_batched": 4}


def newton_solve_probe(route, S, v, p, lds, count=1, ref=None, v2=None, active=None, ss=0, sv=0, sm=0, st=0,
                       x=None, M=None, stats=None):
    """Test hook (dlsa_newton_solve_probe_f64): one route of the Newton-step solver on caller-supplied systems, raw results.
    S, v, ref, v2 are flat fp64 device buffers: system b is the p x p matrix at S[b ss:] with row pitch lds and the vectors at
    v / ref / x[b sv:]; route "sweep_batched" takes `count` systems and an int32 `active` mask, every other route one.
    x, M (L, Linv or Hinv by route; count blocks of p x p at pitch sm) and stats (3 doubles at pitch st) may be passed
    pre-filled: the outputs of an inactive system are left as they are.  Returns (x, M, stats) as flat tensors."""
    lib = _lib.load()
    r = NEWTON_ROUTES[route] if isinstance(route, str) else int(route)
    _require_gpu(S, v, ref, v2, active, x, M, stats)
    p, lds, count = int(p), int(lds), int(count)
    if p <= 0 or lds < p or count <= 0:
        raise ValueError("newton_solve_probe: bad shape p=%d lds=%d count=%d" % (p, lds, count))
    last = count - 1
    need = {"S": last * ss + (p - 1) * lds + p, "v": last * sv + p, "M": last * sm + p * p, "stats": last * st + 3}
    dev = S.device
    x = torch.empty((need["v"],), dtype=torch.float64, device=dev) if x is None else x
    M = torch.empty((need["M"],), dtype=torch.float64, device=dev) if M is None else M
    stats = torch.empty((need["stats"],), dtype=torch.float64, device=dev) if stats is None else stats
    for name, t, n in (("S", S, need["S"]), ("v", v, need["v"]), ("ref", ref, need["v"]), ("v2", v2, p), ("x", x, need["v"]),
                       ("M", M, need["M"]), ("stats", stats, need["stats"])):
        if t is None:
            continue
        if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < n:
            raise ValueError("newton_solve_probe: %s must be a contiguous float64 buffer of at least %d elements" % (name, n))
    if active is not None and (active.dtype != torch.int32 or not active.is_contiguous() or active.numel() < count):
        raise ValueError("newton_solve_probe: active must be a contiguous int32 tensor of count entries")
    ws = _workspace(lib.dlsa_newton_solve_probe_workspace_bytes(r, p, count), dev)
    check(lib.dlsa_newton_solve_probe_f64(r, _ptr(S), lds, p, count, ss, _ptr(v), _ptr(v2), _ptr(ref), sv, _ptr(x), _ptr(M), sm,
                                          _ptr(stats), st, _ptr(active), _ptr(ws), ws.numel(), _stream()))
    return x, M, stats


def _solve_args(S, v, who):
    _require_gpu(S, v)
    _f64(S, "S")
    v = _f64(v.contiguous(), "v")
    p = S.shape[0]
    if S.dim() != 2 or S.shape[1] != p or v.numel() != p:
        raise ValueError("%s: S must be p x p and v of length p" % who)
    return v, p


def wls_solve(S, v):
    """theta = lstsq(S, v, rcond=None)[0] (dlsa/dlsa.py:48-49): Cholesky solve when S is SPD, the minimum-norm
    least-squares solution (device Jacobi eigendecomposition) when it is singular.  Returns (theta, rank)."""
    lib = _lib.load()
    v, p = _solve_args(S, v, "wls_solve")
    theta = torch.empty((p,), dtype=torch.float64, device=S.device)
    ws = _workspace(lib.dlsa_wls_solve_workspace_bytes(p), S.device)
    rank = ctypes.c_int(0)
    check(lib.dlsa_wls_solve_f64(_ptr(S), _rowmajor(S), _ptr(v), p, _ptr(theta), ctypes.byref(rank),
                                 _ptr(ws), ws.numel(), _stream()))
    return theta, rank.value


def sym_pinv_solve(S, v, rcond=None):
    """theta = pinv(S) v for a symmetric S through its eigendecomposition (parallel Jacobi on the device), with
    lstsq's singular-value cut (rcond=None -> eps * p).  Returns (theta, rank, eigenvalues as a host list)."""
    lib = _lib.load()
    v, p = _solve_args(S, v, "sym_pinv_solve")
    theta = torch.empty((p,), dtype=torch.float64, device=S.device)
    ws = _workspace(lib.dlsa_sym_pinv_workspace_bytes(p), S.device)
    rank = ctypes.c_int(0)
    eig = (ctypes.c_double * p)()
    check(lib.dlsa_sym_pinv_solve_f64(_ptr(S), _rowmajor(S), _ptr(v), p, -1.0 if rcond is None else float(rcond),
                                      _ptr(theta), ctypes.byref(rank), eig, _ptr(ws), ws.numel(), _stream()))
    return theta, rank.value, list(eig)


def sym_pinv_probe(S, v, p, lds, rcond=None, ldv=None):
    """Test hook (dlsa_sym_pinv_probe_f64): sym_pinv_solve with the sweep count and the eigenvectors.  S is a flat fp64 device
    buffer holding the p x p matrix at row pitch lds.  Returns (theta, rank, eigenvalues as a host list, sweeps, V) with V a
    [p, ldv] device tensor whose column i (i < p) is the eigenvector of eigenvalue i; columns beyond p keep NaN."""
    lib = _lib.load()
    _require_gpu(S, v)
    p, lds = int(p), int(lds)
    ldv = p if ldv is None else int(ldv)
    if p <= 0 or lds < p or ldv < p:
        raise ValueError("sym_pinv_probe: bad shape p=%d lds=%d ldv=%d" % (p, lds, ldv))
    for name, t, n in (("S", S, (p - 1) * lds + p), ("v", v, p)):
        if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < n:
            raise ValueError("sym_pinv_probe: %s must be a contiguous float64 buffer of at least %d elements" % (name, n))
    theta = torch.empty((p,), dtype=torch.float64, device=S.device)
    V = torch.full((p, ldv), float("nan"), dtype=torch.float64, device=S.device)
    ws = _workspace(lib.dlsa_sym_pinv_workspace_bytes(p), S.device)
    rank, sweeps = ctypes.c_int(0), ctypes.c_int(-1)
    eig = (ctypes.c_double * p)()
    check(lib.dlsa_sym_pinv_probe_f64(_ptr(S), lds, _ptr(v), p, -1.0 if rcond is None else float(rcond), _ptr(theta),
                                      ctypes.byref(rank), eig, ctypes.byref(sweeps), _ptr(V), ldv, _ptr(ws), ws.numel(), _stream()))
    return theta, rank.value, list(eig), sweeps.value, V


LARS_MAX_UNPENALIZED = 32      # include/dlsa_hip.h: DLSA_LARS_MAX_UNPENALIZED


def lars_unpenalized_count(who, intercept, p):
    """`intercept` of lars_path as the count u of leading unpenalised coefficients: a bool (True is 1) or an integer with
    0 <= u <= LARS_MAX_UNPENALIZED and u < p."""
    if isinstance(intercept, bool) or intercept is None:
        u = 1 if intercept else 0
    else:
        u = int(intercept)
        if u != intercept:
            raise ValueError("%s: intercept must be a bool or a whole number, got %r" % (who, intercept))
    if u < 0 or u > LARS_MAX_UNPENALIZED:
        raise ValueError("%s: %d unpenalised coefficients asked for (0 .. %d)" % (who, u, LARS_MAX_UNPENALIZED))
    if u >= p:
        raise ValueError("%s: %d unpenalised coefficients leave nothing to select among p = %d" % (who, u, p))
    return u


def lars_path(Sigma0, b0, intercept, n, type="lar", eps=2.220446049250313e-16, max_steps=None):
    """LARS / lasso path of the LSA objective on the device (dlsa/lsa.py:90-212).  `intercept` is a bool or the count u of LEADING
    coefficients that are not penalised (True is 1); m = p - u.
    Returns dict of device tensors AIC, BIC [steps+1], beta [steps+1, m], beta0 [steps+1] for u <= 1 and [steps+1, u] for u >= 2
    (beta0 excludes b0[:u], as the reference's does: the caller adds it)."""
    lib = _lib.load()
    _require_gpu(Sigma0, b0)
    _f64(Sigma0, "Sigma0")
    b0 = _f64(b0.contiguous(), "b0")
    p = Sigma0.shape[0]
    if Sigma0.dim() != 2 or Sigma0.shape[1] != p or b0.numel() != p:
        raise ValueError("lars_path: Sigma0 must be p x p and b0 of length p")
    u = lars_unpenalized_count("lars_path", intercept, p)
    m = p - u
    # lsa.py:93-94: max_steps defaults to 8 m; the C ABI reads <= 0 as that default, so the buffers are sized for it too
    ms = 8 * m if (max_steps is None or int(max_steps) <= 0) else int(max_steps)
    dev = Sigma0.device
    beta = torch.zeros((ms + 1, m), dtype=torch.float64, device=dev)
    beta0 = torch.zeros((ms + 1,) if u <= 1 else (ms + 1, u), dtype=torch.float64, device=dev)
    aic = torch.zeros((ms + 1,), dtype=torch.float64, device=dev)
    bic = torch.zeros((ms + 1,), dtype=torch.float64, device=dev)
    nb = lib.dlsa_lars_workspace_bytes(p)
    ws = _workspace(nb, dev)
    steps = ctypes.c_int(0)
    check(lib.dlsa_lars_lsa_f64(_ptr(Sigma0), _rowmajor(Sigma0), _ptr(b0), p, u,
                                float(n), {"lar": 0, "lasso": 1}[type], float(eps), ms,
                                _ptr(beta), _ptr(beta0), _ptr(aic), _ptr(bic), ctypes.byref(steps),
                                _ptr(ws), ws.numel(), _stream()))
    k = steps.value
    return {"AIC": aic[: k + 1], "BIC": bic[: k + 1], "beta": beta[: k + 1], "beta0": beta0[: k + 1]}


class OnehotPlan:
    """Handle of a structured one-hot design (include/dlsa_hip.h, dlsa_onehot_plan_create).  Host descriptor arrays:
    dense_kind/src/col int32 [D], dense_shift/scale fp64 [D], nlevels int32 [f], level_col int32 [sum nlevels]."""

    def __init__(self, p, dense_kind, dense_src, dense_shift, dense_scale, dense_col, nlevels, level_col):
        import numpy as np
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("dlsa_amd runs on the GPU only (no CPU fallback)")
        a = lambda v, t: np.ascontiguousarray(np.asarray(v, dtype=t))
        dk, dsrc, dcol = a(dense_kind, np.int32), a(dense_src, np.int32), a(dense_col, np.int32)
        dsh, dsc = a(dense_shift, np.float64), a(dense_scale, np.float64)
        nl, lc = a(nlevels, np.int32), a(level_col, np.int32)
        P = lambda x: ctypes.c_void_p(x.ctypes.data) if x.size else ctypes.c_void_p(0)
        h = ctypes.c_void_p(0)
        check(lib.dlsa_onehot_plan_create(int(p), int(dk.size), P(dk), P(dsrc), P(dsh), P(dsc), P(dcol), int(nl.size),
                                          P(nl), P(lc), ctypes.byref(h)))
        self._h, self._lib = h, lib
        self.p, self.D, self.f = int(p), int(dk.size), int(nl.size)
        self.roles = lib.dlsa_onehot_plan_roles(h)

    def __del__(self):
        try:
            if self._h:
                self._lib.dlsa_onehot_plan_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _oh_args(plan, num, codes):
    _require_gpu(num, codes)
    if num is not None and num.dtype != torch.float64:
        raise ValueError("num must be fp64")
    if codes is not None and codes.dtype != torch.int32:
        raise ValueError("codes must be int32")
    return (_ptr(num), _rowmajor(num) if num is not None else 0, _ptr(codes), _rowmajor(codes) if codes is not None else 0)


def onehot_logit_pass(plan, num, codes, y, beta, want_w=True, want_g=True, want_loglik=True):
    """logit_pass on the raw representation of a one-hot design (num [n,q] fp64, codes [n,f] int32)."""
    lib = _lib.load()
    _require_gpu(y, beta)
    _f64(y, "y"); _f64(beta, "beta")
    n = y.numel()
    dev = y.device
    w = torch.empty((n,), dtype=torch.float64, device=dev) if want_w else None
    g = torch.empty((plan.p,), dtype=torch.float64, device=dev) if want_g else None
    ll = torch.empty((1,), dtype=torch.float64, device=dev) if want_loglik else None
    ws = _workspace(lib.dlsa_onehot_workspace_bytes(plan._h, n), dev)
    pn, ldn, pc, ldc = _oh_args(plan, num, codes)
    check(lib.dlsa_onehot_logit_pass_f64(plan._h, pn, ldn, pc, ldc, _ptr(y), _ptr(beta), n, _ptr(w), _ptr(g), _ptr(ll),
                                         _ptr(ws), ws.numel(), _stream()))
    return w, g, ll


def onehot_gram(plan, num, codes, w, n=None):
    """X' diag(w) X of a one-hot design from its raw representation: the same p x p matrix as gram()."""
    lib = _lib.load()
    _require_gpu(w)
    _f64(w, "w")
    n = int(n if n is not None else (w.numel() if w is not None else (codes.shape[0] if codes is not None else num.shape[0])))
    dev = (codes if codes is not None else num).device
    H = torch.empty((plan.p, plan.p), dtype=torch.float64, device=dev)
    ws = _workspace(lib.dlsa_onehot_workspace_bytes(plan._h, n), dev)
    pn, ldn, pc, ldc = _oh_args(plan, num, codes)
    check(lib.dlsa_onehot_gram_f64(plan._h, pn, ldn, pc, ldc, _ptr(w), n, _ptr(H), H.stride(0), _ptr(ws), ws.numel(), _stream()))
    return H


def onehot_irls_fit(plan, num, codes, y, part_offsets, tol=1e-13, max_iter=100):
    """irls_fit on the raw representation of a one-hot design; same result dict."""
    lib = _lib.load()
    _require_gpu(y)
    _f64(y, "y")
    K, max_rows, c_offs = _offset_partitions("onehot_irls_fit", part_offsets, y.numel())
    out = _FitOut(K, plan.p, y.device)
    ws = _workspace(lib.dlsa_onehot_irls_workspace_bytes(plan._h, max_rows), y.device)
    rc = lib.dlsa_onehot_irls_fit_f64(plan._h, *_oh_args(plan, num, codes), _ptr(y), c_offs, K, tol, max_iter, *out.args,
                                      _ptr(ws), ws.numel(), _stream())
    return out.result(rc)


def onehot_irls_fit_ex(plan, num, codes, y, part_first, part_rows, row_step=1, tol=1e-13, max_iter=100):
    """onehot_irls_fit for partitions given as (first row, rows, common row step): partition_id = i % K is part_first = 0..K-1,
    row_step = K -- strided views of num / codes, no gather (dlsa_onehot_irls_fit_ex_f64).  Same result dict."""
    lib = _lib.load()
    _require_gpu(y)
    _f64(y, "y")
    K, step, max_rows, c_first, c_rows = _strided_partitions("onehot_irls_fit_ex", part_first, part_rows, row_step, y.numel())
    out = _FitOut(K, plan.p, y.device)
    ws = _workspace(lib.dlsa_onehot_irls_ex_workspace_bytes(plan._h, max_rows, step), y.device)
    rc = lib.dlsa_onehot_irls_fit_ex_f64(plan._h, *_oh_args(plan, num, codes), _ptr(y), c_first, c_rows, step, K, tol, max_iter, *out.args,
                                         _ptr(ws), ws.numel(), _stream())
    return out.result(rc)


def _oh_poisson_rows(plan, num, codes, y, offset, who):
    _require_gpu(y, offset)
    _f64(y, "y"); _f64(offset, "offset")
    n = y.numel()
    if (offset is not None and offset.numel() != n) or (num is not None and num.shape[0] != n) or \
            (codes is not None and codes.shape[0] != n):
        raise ValueError("%s: num, codes, y and offset must have the same n = %d rows" % (who, n))
    return n


def _glm_onehot_pass(fam, plan, num, codes, y, beta, scalars, offset, want_H, want_w, **want):
    """The body of onehot_<name>_pass: dlsa_onehot_<name>_pass_f64 on the raw representation (num, codes) of the plan's design."""
    family, who = fam.name, "onehot_%s_pass" % fam.name
    lib = _lib.load()
    _require_gpu(beta)
    _f64(beta, "beta")
    n = _oh_poisson_rows(plan, num, codes, y, offset, who)
    p = plan.p
    if n < 1 or beta.numel() != p:
        raise ValueError("%s: need n >= 1 rows and beta with %d elements" % (who, p))
    scalars = fam.checked(who, scalars, fit=False)
    out = _pass_out(p, n, y.device, want_H, want_w, fam, want)
    ws = _workspace(getattr(lib, "dlsa_onehot_%s_workspace_bytes" % family)(plan._h, n, 1), y.device)
    check(getattr(lib, "dlsa_onehot_%s_pass_f64" % family)(plan._h, *_oh_args(plan, num, codes), _ptr(y), _ptr(offset), _ptr(beta), *scalars, n,
                                                           _ptr(out[0]), p, *[_ptr(t) for t in out[1:]], _ptr(ws), ws.numel(), _stream()))
    return out


def _glm_onehot_fit(fam, plan, num, codes, y, part_first, part_rows, row_step, offset, scalars, tol, max_iter):
    """The body of onehot_<name>_fit_ex: dlsa_onehot_<name>_fit_f64 on strided partitions of the raw representation."""
    family, who = fam.name, "onehot_%s_fit_ex" % fam.name
    lib = _lib.load()
    n = _oh_poisson_rows(plan, num, codes, y, offset, who)
    scalars = fam.checked(who, scalars, fit=True)
    K, step, max_rows, c_first, c_rows = _strided_partitions(who, part_first, part_rows, row_step, n)
    out = _FitOut(K, plan.p, y.device, fam)
    ws = _workspace(getattr(lib, "dlsa_onehot_%s_workspace_bytes" % family)(plan._h, max_rows, step), y.device)
    rc = getattr(lib, "dlsa_onehot_%s_fit_f64" % family)(plan._h, *_oh_args(plan, num, codes), _ptr(y), _ptr(offset), c_first, c_rows, step, K,
                                                         *scalars, tol, max_iter, *out.args, _ptr(ws), ws.numel(), _stream())
    return out.result(rc, c_rows if fam.df else None)


def onehot_poisson_pass(plan, num, codes, y, beta, offset=None, want_H=True, want_w=False):
    """poisson_pass on the raw representation of a one-hot design (dlsa_onehot_poisson_pass_f64): num [n,q] fp64, codes [n,f]
    int32, counts y [n], optional offset [n]; beta has plan.p entries in the plan's column order (an intercept is the plan's
    constant column).  Returns (H [p,p] = X' diag(mu) X or None, g [p] = X'(y - mu), loglik [1], w [n] = mu or None) of the matrix
    dlsa_design_f64 would build -- which is never built."""
    return _glm_onehot_pass(GLM_FAMILIES["poisson"], plan, num, codes, y, beta, (), offset, want_H, want_w)


def onehot_poisson_fit_ex(plan, num, codes, y, part_first, part_rows, row_step=1, offset=None, tol=1e-13, max_iter=100):
    """poisson_fit_ex on the raw representation of a one-hot design (dlsa_onehot_poisson_fit_f64): partition k = rows
    part_first[k] + j * row_step, j < part_rows[k] -- strided views of num / codes, only the counts and offsets of a strided
    partition are gathered.  Same result dict as poisson_fit_ex, plan.p columns in the plan's order."""
    return _glm_onehot_fit(GLM_FAMILIES["poisson"], plan, num, codes, y, part_first, part_rows, row_step, offset, (), tol, max_iter)


def onehot_negbin_pass(plan, num, codes, y, beta, alpha, offset=None, want_H=True, want_w=False, want_theta=False):
    """negbin_pass on the raw representation of a one-hot design (dlsa_onehot_negbin_pass_f64): rows and beta as
    onehot_poisson_pass, alpha > 0 as negbin_pass.  Returns (H [p,p] = X' diag(mu / (1 + alpha mu)) X or None, g [p], loglik [1] = the
    full log-likelihood, w [n] or None, mu [n] or None (with want_w), theta_terms [3] = (s, i, pearson) or None (with want_theta))
    of the matrix dlsa_design_f64 would build -- which is never built."""
    return _glm_onehot_pass(GLM_FAMILIES["negbin"], plan, num, codes, y, beta, (alpha,), offset, want_H, want_w, want_theta=want_theta)


def onehot_negbin_fit_ex(plan, num, codes, y, part_first, part_rows, row_step=1, offset=None, alpha=None, tol=1e-13, max_iter=100):
    """negbin_fit_ex on the raw representation of a one-hot design (dlsa_onehot_negbin_fit_f64): partitions as
    onehot_poisson_fit_ex, alpha as negbin_fit_ex.  Same result dict as negbin_fit_ex, plan.p columns in the plan's order."""
    return _glm_onehot_fit(GLM_FAMILIES["negbin"], plan, num, codes, y, part_first, part_rows, row_step, offset, (alpha,), tol, max_iter)


def onehot_gamma_pass(plan, num, codes, y, beta, dispersion=1.0, offset=None, want_H=True, want_w=False, want_stats=False):
    """gamma_pass on the raw representation of a one-hot design (dlsa_onehot_gamma_pass_f64): rows and beta as onehot_poisson_pass,
    dispersion > 0 as gamma_pass.  Returns (H [p,p] = X' diag(r) X / dispersion or None, g [p], loglik [1] = the full log-likelihood,
    w [n] = r or None, stats [2] = (Pearson, deviance) or None (with want_stats)) of the matrix dlsa_design_f64 would build -- which is
    never built."""
    return _glm_onehot_pass(GLM_FAMILIES["gamma"], plan, num, codes, y, beta, (dispersion,), offset, want_H, want_w, want_stats=want_stats)


def onehot_gamma_fit_ex(plan, num, codes, y, part_first, part_rows, row_step=1, offset=None, dispersion=None, tol=1e-13, max_iter=100):
    """gamma_fit_ex on the raw representation of a one-hot design (dlsa_onehot_gamma_fit_f64): partitions as onehot_poisson_fit_ex,
    dispersion as gamma_fit_ex.  Same result dict as gamma_fit_ex, plan.p columns in the plan's order."""
    return _glm_onehot_fit(GLM_FAMILIES["gamma"], plan, num, codes, y, part_first, part_rows, row_step, offset, (dispersion,), tol, max_iter)


def onehot_tweedie_pass(plan, num, codes, y, beta, power, dispersion=1.0, offset=None, want_H=True, want_w=False, want_stats=False):
    """tweedie_pass on the raw representation of a one-hot design (dlsa_onehot_tweedie_pass_f64): rows and beta as
    onehot_poisson_pass, power and dispersion as tweedie_pass.  Returns (H [p,p] or None, g [p], loglik [1] = the
    quasi-log-likelihood, w [n] or None, stats [2] = (Pearson, deviance) or None (with want_stats)) of the matrix dlsa_design_f64
    would build -- which is never built."""
    return _glm_onehot_pass(GLM_FAMILIES["tweedie"], plan, num, codes, y, beta, (power, dispersion), offset, want_H, want_w,
                            want_stats=want_stats)


def onehot_tweedie_fit_ex(plan, num, codes, y, part_first, part_rows, row_step=1, offset=None, power=1.5, dispersion=None, tol=1e-13,
                          max_iter=100):
    """tweedie_fit_ex on the raw representation of a one-hot design (dlsa_onehot_tweedie_fit_f64): partitions as
    onehot_poisson_fit_ex, power and dispersion as tweedie_fit_ex.  Same result dict as tweedie_fit_ex, plan.p columns in the plan's
    order."""
    return _glm_onehot_fit(GLM_FAMILIES["tweedie"], plan, num, codes, y, part_first, part_rows, row_step, offset, (power, dispersion), tol,
                           max_iter)


def onehot_multinomial_pass(plan, num, codes, y, theta, classes, want_H=True, want_prob=False):
    """multinomial_pass on the raw representation of a one-hot design (dlsa_onehot_multinomial_pass_f64): rows as
    onehot_poisson_pass, y and `classes` as multinomial_pass.  theta [J * plan.p] is class-major, theta[j * p + c] the coefficient of
    class j + 1 on the plan's column c (an intercept is the plan's constant column, one column of every class block).  Returns
    (H [J p, J p] or None, g [J p], loglik [1] -- NaN when a response is no class code --, P [J, n] or None) of the matrix
    dlsa_design_f64 would build -- which is never built."""
    lib = _lib.load()
    _require_gpu(theta)
    _f64(theta, "theta")
    n = _oh_poisson_rows(plan, num, codes, y, None, "onehot_multinomial_pass")
    classes = multinomial_classes("onehot_multinomial_pass", classes, plan.p)
    d = (classes - 1) * plan.p
    if n < 1 or theta.numel() != d:
        raise ValueError("onehot_multinomial_pass: need n >= 1 rows and theta with %d elements" % d)
    H, g, ll, _ = _pass_out(d, n, y.device, want_H, False)
    ld = (n + 31) // 32 * 32                      # 256-byte aligned class rows
    P = torch.empty((classes - 1, ld), dtype=torch.float64, device=y.device) if want_prob else None
    ws = _workspace(lib.dlsa_onehot_multinomial_workspace_bytes(plan._h, n, classes, 1), y.device)
    check(lib.dlsa_onehot_multinomial_pass_f64(plan._h, *_oh_args(plan, num, codes), _ptr(y), _ptr(theta), classes, n, _ptr(H), d, _ptr(g),
                                               _ptr(ll), _ptr(P), ld, _ptr(ws), ws.numel(), _stream()))
    return H, g, ll, (P[:, :n] if want_prob else None)


def onehot_multinomial_fit_ex(plan, num, codes, y, part_first, part_rows, row_step=1, classes=None, tol=1e-13, max_iter=100):
    """multinomial_fit_ex on the raw representation of a one-hot design (dlsa_onehot_multinomial_fit_f64): partitions as
    onehot_poisson_fit_ex, `classes` (2 .. 8, required) and the refusals as multinomial_fit_ex.  Same result dict as
    multinomial_fit_ex with J * plan.p columns, class-major in the plan's column order."""
    return _class_fit(CLASS_FAMILIES["multinomial"], (plan, num, codes), y, part_first, part_rows, row_step, classes, False, tol, max_iter)


def onehot_ordinal_pass(plan, num, codes, y, theta, classes, want_H=True, want_w=False):
    """ordinal_pass on the raw representation of a one-hot design (dlsa_onehot_ordinal_pass_f64, include/dlsa_hip_onehot_ordinal.h):
    rows as onehot_poisson_pass, y and `classes` as ordinal_pass.  The plan must have no constant column -- the cutpoints are the
    intercepts.  theta [J + plan.p] = [alpha_1 .. alpha_J | beta], beta in the plan's column order.  Returns (H [d, d] or None, g [d],
    loglik [1] -- NaN when the cutpoints are not strictly increasing or a response is no class code --, w [n] or None) of the matrix
    dlsa_design_f64 would build -- which is never built."""
    lib = _lib.load()
    _require_gpu(theta)
    _f64(theta, "theta")
    n = _oh_poisson_rows(plan, num, codes, y, None, "onehot_ordinal_pass")
    classes = ordinal_classes("onehot_ordinal_pass", classes, plan.p)
    d = classes - 1 + plan.p
    if n < 1 or theta.numel() != d:
        raise ValueError("onehot_ordinal_pass: need n >= 1 rows and theta with %d elements" % d)
    H, g, ll, w = _pass_out(d, n, y.device, want_H, want_w)
    ws = _workspace(lib.dlsa_onehot_ordinal_workspace_bytes(plan._h, n, classes, 1), y.device)
    check(lib.dlsa_onehot_ordinal_pass_f64(plan._h, *_oh_args(plan, num, codes), _ptr(y), _ptr(theta), classes, n, _ptr(H), d, _ptr(g),
                                           _ptr(ll), _ptr(w), _ptr(ws), ws.numel(), _stream()))
    return H, g, ll, w


def onehot_ordinal_fit_ex(plan, num, codes, y, part_first, part_rows, row_step=1, classes=None, tol=1e-13, max_iter=100):
    """ordinal_fit_ex on the raw representation of a one-hot design (dlsa_onehot_ordinal_fit_f64): partitions as
    onehot_poisson_fit_ex, `classes` (2 .. 8, required) and the refusals as ordinal_fit_ex; a plan with a constant column is refused.
    Same result dict as ordinal_fit_ex with J + plan.p columns, cutpoints first, then the plan's column order."""
    return _class_fit(CLASS_FAMILIES["ordinal"], (plan, num, codes), y, part_first, part_rows, row_step, classes, False, tol, max_iter)


class RcclComm:
    """An RCCL communicator opened through the C ABI (dlsa_comm_unique_id / dlsa_comm_init_rank), for hosts that do not
    use torch.distributed: rank 0 creates `RcclComm.unique_id()`, ships the 128 bytes to the other ranks out of band, every
    rank constructs RcclComm(nranks, id, rank) after selecting its device; `allreduce(msg)` is the algorithm's one round
    of communication (dlsa/dlsa.py:30-34), in place on the current stream."""

    def __init__(self, nranks, unique_id, rank):
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("dlsa_amd runs on the GPU only (no CPU fallback)")
        torch.cuda.current_device()         # the HIP context of this rank's device must exist before ncclCommInitRank
        h = ctypes.c_void_p(0)
        check(lib.dlsa_comm_init_rank(ctypes.byref(h), int(nranks), bytes(unique_id), int(rank)))
        self._h, self._lib, self.nranks, self.rank = h, lib, int(nranks), int(rank)

    @staticmethod
    def unique_id():
        lib = _lib.load()
        buf = ctypes.create_string_buffer(128)
        check(lib.dlsa_comm_unique_id(buf))
        return buf.raw

    def allreduce(self, msg):
        _require_gpu(msg)
        _f64(msg, "msg")
        if msg.dim() != 1:
            raise ValueError("allreduce: msg must be a contiguous vector")
        check(self._lib.dlsa_allreduce_f64(self._h, _ptr(msg), msg.numel(), _stream()))
        return msg

    def close(self):
        if self._h:
            self._lib.dlsa_comm_destroy(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
