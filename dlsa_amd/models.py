"""Map step of DLSA on the GPU -- the host-side mirror of the reference's dlsa/models.py.

Same function names, argument meaning, output columns and soft-fail behaviour as the
reference (`simulate_logistic` models.py:6-40, `logistic_model` :42-147,
`logistic_model_eval` :151-225); the numeric core (fit, weights, Gram, Sig_inv.coef,
log-likelihood) runs in the HIP engine.  pandas is used exactly where the reference uses it:
for the column bookkeeping of the frames that cross the operator boundary.

Fitting difference (deliberate, SURVEY.md finding 1): the reference stops sklearn's newton-cg at
tol=1e-4, ~1e-3 away from the MLE; this engine returns the exact MLE (Newton/IRLS to a 1e-13
step), which is what the reference computes when its tolerance is tightened.
"""
import os
import warnings

import numpy as np
import pandas as pd
import torch

from . import engine
from .design import DesignSpec


class MappedBlocks:
    """Device-resident result of the map step for K partitions:
    coef [K,p], Sig_invMcoef [K,p], Sig_inv [K,p,p] (+ column names, per-partition status).
    `to_frame()` gives the reference's stacked layout: K*p rows x (3+p) columns
    `par_id, coef, Sig_invMcoef, <names...>` (models.py:136-142)."""

    def __init__(self, coef, Sig_invMcoef, Sig_inv, names, status=None, n_iter=None, loglik=None,
                 num_partitions=None, sample_size=None, extra=None):
        self.coef, self.Sig_invMcoef, self.Sig_inv = coef, Sig_invMcoef, Sig_inv
        self.names = list(names)
        K = coef.shape[0]
        self.status = list(status) if status is not None else [0] * K
        self.n_iter = list(n_iter) if n_iter is not None else [0] * K
        self.loglik = list(loglik) if loglik is not None else [0.0] * K
        self.num_partitions = K if num_partitions is None else int(num_partitions)
        self.sample_size = sample_size
        self.extra = {} if extra is None else {k: list(v) for k, v in extra.items()}     # per-partition lists of a family's own

    @property
    def columns(self):
        return ["par_id", "coef", "Sig_invMcoef"] + self.names

    def block_frame(self, k):
        p = self.coef.shape[1]
        out_np = torch.cat([self.coef[k][:, None], self.Sig_invMcoef[k][:, None], self.Sig_inv[k]], 1).cpu().numpy()
        out = pd.DataFrame(out_np, columns=pd.Index(["coef", "Sig_invMcoef"] + self.names))
        out.insert(0, "par_id", np.arange(p))
        return out

    def to_frame(self):
        return pd.concat([self.block_frame(k) for k in range(self.coef.shape[0])], ignore_index=True)


def _partitions(n, partition_num, part_offsets):
    """The partitions of n rows as (first rows, row counts, common row step), the form the engine's fits take -- strided views,
    nothing is gathered: `part_offsets` (K+1 ints) gives contiguous row ranges, else partition_id = i % partition_num (models.py:33;
    None or 0: one partition) gives the rows k, k + K, ..."""
    if part_offsets is None:
        K = int(partition_num) if partition_num else 1
        return list(range(K)), [len(range(k, n, K)) for k in range(K)], K
    offs = [int(v) for v in part_offsets]
    return offs[:-1], [offs[k + 1] - offs[k] for k in range(len(offs) - 1)], 1


def _column_names(names, p, fit_intercept):
    """The result's column names: `names` (default x0 .. x{p-1}), `intercept` first when the fit carries one."""
    if names is None:
        names = ["x" + str(i) for i in range(p)]
    return (["intercept"] if fit_intercept else []) + list(names)


def _blocks(r, names, n, family=None):
    """MappedBlocks of an engine fit's result dict; with a log-link `family` (an engine.GLM_FAMILIES record) its own per-partition
    lists go to `extra`."""
    extra = None if family is None else {k: r[k] for k in family.fit_lists + (("df",) if family.df else ())}
    return MappedBlocks(r["coef"], r["Sig_invMcoef"], r["Sig_inv"], names, r["status"], r["n_iter"], r["loglik"], sample_size=n,
                        extra=extra)


def _require_dense_rows(who, X, note=""):
    """What opens every fit_*_partitions: the rows are on the GPU and fp64."""
    if not X.is_cuda:
        raise RuntimeError("%s runs on the GPU only (no CPU fallback)" % who)
    if X.dtype != torch.float64:
        raise TypeError("%s: X must be float64%s, got %s" % (who, note, X.dtype))


def _require_raw_rows(who, num, y):
    """What opens every fit_*_design: the response is on the GPU, the numeric columns (if any) are fp64."""
    if not torch.is_tensor(y) or not y.is_cuda:
        raise RuntimeError("%s runs on the GPU only (no CPU fallback)" % who)
    if num is not None and num.dtype != torch.float64:
        raise TypeError("%s: num must be float64, got %s" % (who, num.dtype))


def _fit_design(onehot_fit, dense_fit, num, codes, y, spec, partition_num, part_offsets, structured, names=None, family=None, **fit_args):
    """The body of the fit_*_design functions: the family's structured engine fit on the raw columns when the design qualifies,
    else its dense fit on the matrix the design kernel builds once; the same strided partitions either way.  `names`: the blocks'
    column names when they are not spec.names (the multinomial family's J class blocks); `family` as in _blocks."""
    n = y.numel()
    first, rows, step = _partitions(n, partition_num, part_offsets)
    plan = spec.onehot_plan() if structured else None
    if plan is not None:
        r = onehot_fit(plan, engine.row_major(num) if num is not None else None, engine.row_major(codes) if codes is not None else None,
                       y, first, rows, row_step=step, **fit_args)
    else:
        X, _ = spec.build(num, codes)
        r = dense_fit(X, y, first, rows, row_step=step, **fit_args)
    return _blocks(r, spec.names if names is None else names, n, family)


def _to_device(sample_df, name):
    """A frame's column as an fp64 device vector (None for no column)."""
    return None if name is None else torch.from_numpy(np.ascontiguousarray(sample_df[name].to_numpy(dtype=np.float64))).cuda()


def _zero_block(names):
    """The all-zero block of a chunk that is skipped (models.py:84-91)."""
    return pd.DataFrame(0, index=np.arange(len(names)), columns=["par_id", "coef", "Sig_invMcoef"] + names)


def _warn_missing_levels(missing, rows, names, fit_intercept, skip):
    """The reference's warning for a chunk that lacks expected dummy levels (models.py:80-91 / :187-194)."""
    shape = (rows, len(names) - (1 if fit_intercept else 0) - len(missing))
    warnings.warn("Dummies:" + str(set(missing)) + "missing in this data chunk " + str(shape)
                  + ("Skip modeling this part of data." if skip else ""))


def _first_block_frame(mb, who=None, not_pd="information matrix not positive definite (collinear design)", hint=""):
    """The frame of a one-partition map step, with the frame-level models' warnings: `who`'s soft failures by `status`, and the
    reference's NA warning (models.py:144-145)."""
    if who is not None and mb.status[0] == 1:
        warnings.warn("%s: Newton iterations did not converge (max_iter reached%s)" % (who, hint))
    elif who is not None and mb.status[0] == 2:
        warnings.warn("%s: %s" % (who, not_pd))
    out = mb.block_frame(0)
    if out.isna().values.any():
        warnings.warn("NAs appear in the final output")
    return out


def simulate_logistic(sample_size, p, partition_method, partition_num, seed=20260101, kind="uniform"):
    """models.py:6-40 with a seeded counter RNG on the GPU: features ~ U(-0.5,0.5) (:22), beta =
    ones on the first int(0.4p) coordinates (:12,18-19), label ~ Bernoulli(sigmoid(x.beta)) (:23,30),
    partition_id = i % partition_num (:33).  Returns the reference's frame: partition_id, label, x0.."""
    if partition_method != "systematic":
        raise Exception("No such partition method implemented!")      # models.py:35
    X, y = engine.synth(seed, 0, int(sample_size), int(p),
                        kind=engine.SYNTH_UNIFORM if kind == "uniform" else engine.SYNTH_GAUSSIAN)
    n = int(sample_size)
    pid = (np.arange(n) % partition_num).astype(np.float64)
    data_np = np.concatenate((pid[:, None], y.cpu().numpy()[:, None], X.cpu().numpy()), 1)
    return pd.DataFrame(data_np, columns=["partition_id"] + ["label"] + ["x" + str(x) for x in range(p)])


def _device_design(sample_df, Y_name, fit_intercept, dummy_info, dummy_factors_baseline, data_info, for_eval=False):
    """models.py:50-108,121-122 (and :159-206 for eval): the chunk's design matrix, built ON THE DEVICE.
    The host only does the column bookkeeping and turns categorical strings into level codes
    (design.DesignSpec); get_dummies / baseline drop / standardise / reindex / ones column are one
    dlsa_design_f64 launch.  Returns (X device tensor or None when the chunk must be skipped,
    names = [intercept,] usecols_x)."""
    spec = DesignSpec.from_reference(list(sample_df.columns), Y_name, fit_intercept, dummy_info,
                                     ([] if (for_eval and len(dummy_info) == 0) else dummy_factors_baseline), data_info)
    _, codes, unknown = spec.encode(sample_df, dummy_info, numeric=False)
    dev = torch.device("cuda")
    X, missing = spec.build(spec.numeric_to_device(sample_df, dev), torch.from_numpy(codes).to(dev))
    if missing or unknown:
        _warn_missing_levels(missing, len(sample_df), spec.names, fit_intercept, skip=not for_eval)
        if not for_eval:
            return None, spec.names
    return X, spec.names


def logistic_model(sample_df, Y_name, fit_intercept=False, dummy_info=[], dummy_factors_baseline=[],
                   data_info=[]):
    """Run the logistic model on one partition (a pandas frame), as the reference's GROUPED_MAP
    UDF does (models.py:42-147).  Returns the p x (3+p) frame `par_id, coef, Sig_invMcoef,
    [intercept,] <features>`; a chunk that lacks an expected dummy level returns the all-zero
    block with a warning (models.py:84-91)."""
    yd = _to_device(sample_df, Y_name)
    r = None
    if len(dummy_info) > 0:
        # dummy path: fit on the raw numerics + level codes when the design qualifies (structured passes, the dense
        # one-hot matrix is never built); the missing-level check of models.py:80-91 runs on the codes
        spec = DesignSpec.from_reference(list(sample_df.columns), Y_name, fit_intercept, dummy_info,
                                         dummy_factors_baseline, data_info)
        plan = spec.onehot_plan()
        if plan is not None:
            names = spec.names
            _, codes, unknown = spec.encode(sample_df, dummy_info, numeric=False)
            missing = spec.missing_levels(codes)
            if missing or unknown:
                _warn_missing_levels(missing, len(sample_df), names, fit_intercept, skip=True)
                return _zero_block(names)
            r = engine.onehot_irls_fit(plan, spec.numeric_to_device(sample_df), torch.from_numpy(codes).cuda(), yd, [0, len(sample_df)])
    if r is None:
        Xd, names = _device_design(sample_df, Y_name, fit_intercept, dummy_info, dummy_factors_baseline, data_info)
        if Xd is None:
            return _zero_block(names)
        r = engine.irls_fit(Xd, yd, [0, Xd.shape[0]])
    return _first_block_frame(_blocks(r, names, len(sample_df)), "logistic_model", "Hessian not positive definite (collinear or separable data)")


def fit_logistic_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, names=None,
                            tol=1e-13, max_iter=100, options=None, **option_fields):
    """Tensor fast path of the map step for MANY partitions of one device-resident shard.

    X [n, p] fp64 row-major on the GPU, y [n].  Either `part_offsets` (K+1 ints: partition k is the
    contiguous row range [off[k], off[k+1]) -- the layout `repartition(K, "partition_id")` gives,
    logistic_dlsa.py:295) or `partition_num` (systematic partition_id = i % K, models.py:33: partition k is
    the strided view X[k::K], nothing is gathered).  With fit_intercept the leading ones column of
    models.py:121-122 is implicit in the kernels (results have p + 1 columns, `intercept` first).
    `options` (an engine.IrlsOptions) or its fields as keyword arguments -- chains=, seeded=, fused=, predict=, subsample_div=, ... --
    set the IRLS driver's policy for this call (default: chosen from the shapes; same results to the parity tolerance either way).
    Returns MappedBlocks."""
    _require_dense_rows("fit_logistic_partitions", X, " (the logistic path is fp64 end to end; fit_linear_partitions takes fp32 rows)")
    y = y.to(torch.float64)                 # labels may arrive as integers / bools / fp32
    n, p = X.shape
    names = _column_names(names, p, fit_intercept)
    # No copy of the shard either way: partition_id = i % K is the strided view rows k, k + K, ... (row pitch ldx K), and the
    # intercept's ones column (models.py:121-122) is implicit in the kernels.  At config-3 scale (2.5e7 x 500 fp64 = 100 GB
    # of a 288 GB part) a gathered copy plus a [1 | X] copy would not fit.
    first, rows, step = _partitions(n, partition_num, part_offsets)
    with engine.irls_options(options, **option_fields):
        r = engine.irls_fit_ex(engine.row_major(X), y.contiguous(), first, rows, row_step=step, fit_intercept=fit_intercept,
                               tol=tol, max_iter=max_iter)
    return _blocks(r, names, n)


def fit_logistic_design(num, codes, y, spec, partition_num=None, part_offsets=None, structured=True, tol=1e-13,
                        max_iter=100, options=None, **option_fields):
    """Tensor fast path of the map step for a design given by its RAW columns: num [n, q] fp64 (columns in
    spec.numeric_cols order) and codes [n, f] int32 level codes (DesignSpec.encode), both on the GPU.
    With structured=True and a qualifying design (<= 8 dense columns, <= 8 factors; pair tables larger than LDS are cut into bands) the fit runs on
    the raw representation -- gather / histogram passes, the dense [n, p] matrix is never built (config 4: 76 B
    instead of 2080 B per row and pass); otherwise the matrix is built once by the design kernel and the dense
    kernels run.  Same MappedBlocks either way."""
    _require_raw_rows("fit_logistic_design", num, y)
    y = y.to(torch.float64)
    # partition_id = i % K (models.py:33) as strided views: nothing is gathered (the structured fit takes (first, rows, step); the
    # dense one builds the matrix once and hands the same views to dlsa_irls_fit_ex_f64)
    with engine.irls_options(options, **option_fields):       # (the IRLS driver's policy for this call: see fit_logistic_partitions)
        return _fit_design(engine.onehot_irls_fit_ex, engine.irls_fit_ex, num, codes, y.contiguous(), spec, partition_num, part_offsets,
                           structured, tol=tol, max_iter=max_iter)


def logistic_model_eval(sample_df, Y_name, par, fit_intercept=False, dummy_info=[], dummy_factors_baseline=[],
                        data_info=[]):
    """Log-likelihood of every estimator column of `par` on one partition (models.py:151-225)."""
    Xd, _ = _device_design(sample_df, Y_name, fit_intercept, dummy_info, dummy_factors_baseline, data_info,
                           for_eval=True)
    yd = _to_device(sample_df, Y_name)
    pard = torch.from_numpy(np.ascontiguousarray(np.asarray(par, dtype=np.float64))).cuda()
    ll = engine.loglik(Xd, yd, pard).cpu().numpy()
    return pd.DataFrame({par.columns[i]: [ll[i]] for i in range(par.shape[1])})


# ---------------------------------------------------------------------------------------------
# Linear-regression map step.  The reference claims linear DLSA (README.md:6) but ships
# only the logistic map; this sibling keeps the same block layout so dlsa_mapred / dlsa apply unchanged:
#   coef = OLS estimate, Sig_inv = X'X, Sig_invMcoef = X'y (= X'X coef).
# With these blocks the WLS combine of dlsa_mapred equals the global OLS estimate exactly.
# ---------------------------------------------------------------------------------------------
class _LinearBlock:
    """Sufficient statistics of one partition of a linear model, accumulated chunk by chunk ON THE DEVICE by library
    kernels only: H = [1 | X]'[1 | X] (fp64; the ones column of models.py:121-122 implicit), g = [1 | X]'y, y'y, n.
    fp64 rows: dlsa_gram_f64 (accumulate) straight into H's X-block; fp32 rows: dlsa_gram_f32_acc64 (fp32 MFMA passes,
    fp64 sum).  X'y, the column sums (the intercept's border), y'y and sum y: dlsa_xtv_stats_* -- one read of the chunk."""

    def __init__(self, p, fit_intercept, sig_out, smc_out, device):
        self.p, self.icpt = p, 1 if fit_intercept else 0
        self.sig, self.smc = sig_out, smc_out                      # [pp, pp] / [pp] views of the result block (fp64)
        self.HX = sig_out[self.icpt:, self.icpt:]                  # the X'X block, written in place (row pitch pp)
        self.g = torch.zeros((p,), dtype=torch.float64, device=device)
        self.colsum = torch.zeros((p,), dtype=torch.float64, device=device) if fit_intercept else None
        self.stats = torch.zeros((2,), dtype=torch.float64, device=device)
        self.rows = 0

    def add(self, Xc, yc):
        # (the X'y pass on a second stream next to the Gram of the same chunk was measured in round 4: 2.139 vs 2.141 s for config 5's
        # stream -- kernels on two streams do run side by side here, but take the sum of their times; bench/overlap_probe.py)
        first = self.rows == 0
        if Xc.dtype == torch.float32:
            engine.gram_acc64(Xc, None, out=self.HX, accumulate=not first)
        else:
            engine.gram(Xc, None, out=self.HX, accumulate=not first)
        engine.xtv_stats(Xc, yc, g=self.g, colsum=self.colsum, stats=self.stats, want_colsum=bool(self.icpt), accumulate=True)
        self.rows += Xc.shape[0]

    def finish(self):
        """Borders of the implicit ones column, X'y into the block; returns y'y (host float)."""
        st = self.stats.cpu().numpy()
        self.smc[self.icpt:] = self.g
        if self.icpt:
            self.sig[0, 0] = float(self.rows)
            self.sig[0, 1:] = self.colsum
            self.sig[1:, 0] = self.colsum
            self.smc[0] = float(st[1])
        return float(st[0])


def _linear_finish(blocks, coef, smc, sig, names, n):
    status, rss = [], []
    for k, blk in enumerate(blocks):
        if blk is None or blk.rows == 0:
            status.append(4); rss.append(0.0)
            continue
        yy = blk.finish()
        try:
            coef[k] = engine.spd_solve(sig[k], smc[k])
            status.append(0)
            rss.append(yy - float(np.dot(coef[k].cpu().numpy(), smc[k].cpu().numpy())))      # y'y - theta'X'y
        except Exception:
            status.append(2); rss.append(float("nan"))
            warnings.warn("linear_model: X'X not positive definite (collinear design)")
    return MappedBlocks(coef, smc, sig, names, status, [1] * len(blocks), rss, sample_size=n)


def fit_linear_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, names=None):
    """Tensor fast path: one Gram pass X'X + one X'y pass per partition, no copy of the shard -- partition_id = i % K
    (models.py:33) is the strided view X[k::K] (every kernel takes any row pitch), contiguous partitions are row ranges, and
    the intercept's ones column (models.py:121-122) stays implicit (its border comes from the X'y pass).  fp32 rows
    (config 5) run the fp32 MFMA Gram with fp64 slab sums; blocks are fp64 either way.  Returns MappedBlocks whose
    `loglik` slot carries the residual sum of squares of each partition."""
    if not X.is_cuda:
        raise RuntimeError("fit_linear_partitions runs on the GPU only (no CPU fallback)")
    if X.dtype not in (torch.float64, torch.float32):
        raise TypeError("fit_linear_partitions: X must be float64 or float32, got %s" % X.dtype)
    X = engine.row_major(X)
    y = y.to(X.dtype)
    n, p = X.shape
    if part_offsets is None:
        K = int(partition_num) if partition_num else 1
        views = [(X[k::K], y[k::K].contiguous() if K > 1 else y.contiguous()) for k in range(K)]
    else:
        offs = [int(v) for v in part_offsets]
        K = len(offs) - 1
        yc = y.contiguous()
        views = [(X[offs[k]:offs[k + 1]], yc[offs[k]:offs[k + 1]]) for k in range(K)]
    pp = p + (1 if fit_intercept else 0)
    names = _column_names(names, p, fit_intercept)
    coef = torch.zeros((K, pp), dtype=torch.float64, device=X.device)
    smc = torch.zeros((K, pp), dtype=torch.float64, device=X.device)
    sig = torch.zeros((K, pp, pp), dtype=torch.float64, device=X.device)
    blocks = []
    for k, (Xk, yk) in enumerate(views):
        if Xk.shape[0] == 0:
            blocks.append(None)
            continue
        blk = _LinearBlock(p, fit_intercept, sig[k], smc[k], X.device)
        blk.add(Xk, yk)
        blocks.append(blk)
    return _linear_finish(blocks, coef, smc, sig, names, n)


def fit_linear_streaming(n, p, partition_num=1, chunk_rows=1 << 22, seed=20260101, row0=0, kind="gaussian", sigma=1.0,
                         fit_intercept=False, dtype=torch.float32, names=None, device="cuda", on_chunk=None, overlap=False):
    """The linear map step for a shard that does NOT fit HBM (BASELINE config 5: 6.25e7 x 2000 fp32 = 500 GB per GPU, SURVEY
    8(d)): rows row0 .. row0 + n of the seeded stream are generated ON THE DEVICE chunk by chunk (dlsa_synth_*: a row is a
    pure function of (seed, i); y = X beta* + sigma N(0,1) by dlsa_synth_response_*), each chunk goes once through the Gram
    kernel (accumulating) and once through the X'y pass, and is overwritten by the next.  The K partitions are contiguous
    row ranges of the stream (the layout repartition(K, "partition_id") gives, logistic_dlsa.py:295); chunks never straddle
    a partition.  Peak memory = one chunk buffer + K blocks.  kind="gaussian32" (fp32 only) is the fp32-native stream: features and
    response in ONE launch (engine.synth_linear32), 8.5 ms per 2^22 x 2000 chunk where "gaussian" + synth_response take 41 -- config 5
    at its stated size 2.58 -> 2.11 s (97 -> 119 TF including generation).  overlap=True generates chunk i + 1 into a second buffer on
    a side stream while chunk i is consumed: the kernels do run side by side, but generator and Gram together take the SUM of their
    times (VALU work is not hidden under the fp32 matrix pipe on this chip, bench/overlap_probe.py: 120.1 + 41.2 -> 161.3 ms) for
    twice the chunk memory -- off by default.  Returns MappedBlocks (fp64 blocks)."""
    K = int(partition_num)
    n, p, chunk_rows = int(n), int(p), int(chunk_rows)
    if K < 1 or n < 0 or chunk_rows < 1:
        raise ValueError("fit_linear_streaming: need partition_num >= 1, n >= 0, chunk_rows >= 1")
    # kind "gaussian32": the fp32-native stream (engine.synth_linear32: features and response in ONE launch, a quarter of the
    # generator time of "gaussian" + synth_response at p = 2000) -- fp32 only
    native32 = isinstance(kind, str) and kind == "gaussian32"
    if native32 and dtype != torch.float32:
        raise ValueError("fit_linear_streaming: kind='gaussian32' is the fp32-native stream (dtype=torch.float32)")
    kind_id = 0 if native32 else ({"uniform": engine.SYNTH_UNIFORM, "gaussian": engine.SYNTH_GAUSSIAN}[kind] if isinstance(kind, str) else int(kind))
    pp = p + (1 if fit_intercept else 0)
    names = _column_names(names, p, fit_intercept)
    coef = torch.zeros((K, pp), dtype=torch.float64, device=device)
    smc = torch.zeros((K, pp), dtype=torch.float64, device=device)
    sig = torch.zeros((K, pp, pp), dtype=torch.float64, device=device)
    offs = [int(n * k / K) for k in range(K + 1)]
    rows_max = min(chunk_rows, max(1, max(offs[k + 1] - offs[k] for k in range(K))))
    chunks = [(k, r, min(rows_max, offs[k + 1] - r)) for k in range(K) for r in range(offs[k], offs[k + 1], rows_max)]
    # Two chunk buffers: chunk i + 1 is generated on a side stream while chunk i goes through the Gram and X'y kernels on the
    # caller's stream (generation is ~1/4 of a chunk's time at p = 2000: hidden instead of added).  HIP events order the hand-offs.
    nbuf = 2 if (overlap and len(chunks) > 1) else 1
    Xbuf = [engine.empty_rows(rows_max, p, dtype, device) for _ in range(nbuf)]
    ybuf = [torch.empty((rows_max,), dtype=dtype, device=device) for _ in range(nbuf)]
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream() if nbuf == 2 else main
    ready = [torch.cuda.Event() for _ in range(nbuf)]
    done = [torch.cuda.Event() for _ in range(nbuf)]

    def generate(i):
        k, r, m = chunks[i]
        b = i % nbuf
        with torch.cuda.stream(side):
            if i >= nbuf:
                side.wait_event(done[b])             # the kernels that read this buffer two chunks ago have finished
            if native32:
                engine.synth_linear32(seed, row0 + r, m, p, sigma=sigma, out=Xbuf[b][:m], out_y=ybuf[b][:m])
            else:
                engine.synth(seed, row0 + r, m, p, kind=kind_id, labels=False, dtype=dtype, out=Xbuf[b][:m])
                engine.synth_response(seed, row0 + r, Xbuf[b][:m], sigma=sigma, out=ybuf[b][:m])
            ready[b].record(side)

    blocks = [None] * K
    if nbuf == 2:
        side.wait_stream(main)
    if chunks:
        generate(0)
    for i, (k, r, m) in enumerate(chunks):
        b = i % nbuf
        if i + 1 < len(chunks) and nbuf == 2:
            generate(i + 1)
        main.wait_event(ready[b])
        if blocks[k] is None:
            blocks[k] = _LinearBlock(p, fit_intercept, sig[k], smc[k], device)
        blocks[k].add(Xbuf[b][:m], ybuf[b][:m])
        done[b].record(main)
        if nbuf == 1 and i + 1 < len(chunks):
            generate(i + 1)
        if on_chunk is not None:
            on_chunk(k, r, m)
    if nbuf == 2:
        main.wait_stream(side)
    return _linear_finish(blocks, coef, smc, sig, names, n)


def fit_linear_chunks(chunks, p, partition_num=1, fit_intercept=False, dtype=None, names=None, device="cuda", sample_size=None):
    """The linear map step for rows that live OUTSIDE HBM (host memory, files read chunk by chunk: `dlsa_amd.ingest`):
    `chunks` yields `(k, X, y)` -- rows of partition k, X [m, p] and y [m] as numpy arrays or torch tensors, on the host
    (pinned memory makes the copy asynchronous) or already on the device, any m >= 1, any order of k.  Two device chunk
    buffers: the host -> HBM copy of chunk i + 1 runs on a copy stream (SDMA engines, no CU) while chunk i goes through the
    Gram kernel (accumulating) and the X'y pass on the caller's stream, so a PCIe-bound source costs max(copy, compute) per
    chunk instead of their sum.  A host chunk may be reused by the producer as soon as the NEXT item is requested (the copy
    out of it has completed by then).  Every chunk of one call has the same dtype (fp32 -> fp32 MFMA Gram summed in fp64,
    fp64 -> fp64 Gram); blocks are fp64.  Peak device memory = two buffers of the largest chunk + K blocks.
    Returns MappedBlocks (`loglik` slot = residual sum of squares per partition), as fit_linear_partitions does."""
    K = int(partition_num)
    p = int(p)
    if K < 1 or p < 1:
        raise ValueError("fit_linear_chunks: need partition_num >= 1 and p >= 1")
    if not torch.cuda.is_available():
        raise RuntimeError("fit_linear_chunks runs on the GPU only (no CPU fallback)")
    pp = p + (1 if fit_intercept else 0)
    names = _column_names(names, p, fit_intercept)
    coef = torch.zeros((K, pp), dtype=torch.float64, device=device)
    smc = torch.zeros((K, pp), dtype=torch.float64, device=device)
    sig = torch.zeros((K, pp, pp), dtype=torch.float64, device=device)
    blocks = [None] * K
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    Xbuf, ybuf = [None, None], [None, None]
    ready = [torch.cuda.Event(), torch.cuda.Event()]
    done = [None, None]
    rows_seen = 0
    side.wait_stream(main)
    for i, item in enumerate(chunks):
        k, Xc, yc = item
        k = int(k)
        if not 0 <= k < K:
            raise ValueError("fit_linear_chunks: partition index %d outside 0..%d" % (k, K - 1))
        Xc = torch.from_numpy(Xc) if isinstance(Xc, np.ndarray) else Xc
        yc = torch.from_numpy(yc) if isinstance(yc, np.ndarray) else yc
        if Xc.dim() != 2 or Xc.shape[1] != p or yc.dim() != 1 or yc.shape[0] != Xc.shape[0]:
            raise ValueError("fit_linear_chunks: chunk %d has X %s, y %s (need [m, %d] and [m])" % (i, tuple(Xc.shape), tuple(yc.shape), p))
        m = int(Xc.shape[0])
        if m == 0:
            continue
        if dtype is None:
            dtype = Xc.dtype if Xc.dtype in (torch.float32, torch.float64) else torch.float64
        b = i & 1
        if Xc.is_cuda and Xc.dtype == dtype and Xc.stride(1) == 1 and yc.is_cuda:
            # rows already in HBM: no staging copy (the caller keeps them alive until the call returns)
            Xd, yd = Xc, yc if yc.dtype == dtype else yc.to(dtype)
        else:
            with torch.cuda.stream(side):
                if done[b] is not None:
                    side.wait_event(done[b])             # the kernels that read this buffer two chunks ago have finished
                if Xbuf[b] is None or Xbuf[b].shape[0] < m:
                    if done[b] is not None:
                        done[b].synchronize()            # (growing a buffer: its old storage must be idle before it is freed)
                    Xbuf[b] = engine.empty_rows(m, p, dtype, device)
                    ybuf[b] = torch.empty((m,), dtype=dtype, device=device)
                Xbuf[b][:m].copy_(Xc, non_blocking=True)
                ybuf[b][:m].copy_(yc, non_blocking=True)
                ready[b].record(side)
            main.wait_event(ready[b])
            Xd, yd = Xbuf[b][:m], ybuf[b][:m]
        if blocks[k] is None:
            blocks[k] = _LinearBlock(p, fit_intercept, sig[k], smc[k], device)
        blocks[k].add(Xd, yd)
        done[b] = torch.cuda.Event()
        done[b].record(main)
        rows_seen += m
        if not Xc.is_cuda:
            ready[b].synchronize()                       # the producer may overwrite its host chunk from here on
    main.wait_stream(side)
    return _linear_finish(blocks, coef, smc, sig, names, rows_seen if sample_size is None else int(sample_size))


def linear_model(sample_df, Y_name, fit_intercept=False, dummy_info=[], dummy_factors_baseline=[], data_info=[]):
    """Frame-level sibling of logistic_model for a linear response: same arguments, same
    p x (3+p) output frame `par_id, coef, Sig_invMcoef, [intercept,] <features>`."""
    Xd, names = _device_design(sample_df, Y_name, fit_intercept, dummy_info, dummy_factors_baseline, data_info)
    if Xd is None:
        return _zero_block(names)
    mb = fit_linear_partitions(Xd, _to_device(sample_df, Y_name), fit_intercept=False, names=names)      # the ones column is already in Xd
    return _first_block_frame(mb)


# ---------------------------------------------------------------------------------------------
# Cox proportional-hazards map step (Breslow ties by default, Efron's approximation on request): the third model family the DLSA method names.  The local objective of
# partition k is its own partial likelihood with risk sets inside the partition (a Cox model stratified by partition with a
# common beta); the block is coef = the partition's MLE, Sig_inv = the observed information there, Sig_invMcoef = Sig_inv coef,
# so dlsa_mapred / dlsa apply unchanged.  No intercept (the partial likelihood does not identify one).
# ---------------------------------------------------------------------------------------------
def simulate_cox(sample_size, p, partition_num, seed=20260101, censor_rate=0.3, tie_levels=None, strata=None):
    """Seeded survival rows: x as simulate_logistic's (U(-0.5, 0.5), the rows of engine.synth), hazard exp(x beta*) with beta* as
    in simulate_logistic (first int(0.4p) coefficients 1), event times T = E / exp(x beta*) with E ~ Exp(1), censoring times
    C ~ Exp(rate) with the rate that censors about `censor_rate` of the rows; time = min(T, C), event = T <= C.  tie_levels
    rounds the times onto that many quantile levels (heavy ties).  partition_id = i % partition_num.
    strata: an int S gives every row the stratum i // partition_num % S (every partition holds all S strata in equal shares)
    and multiplies the event times of stratum s by 2 ** (s - (S - 1) / 2): a baseline hazard of its own per stratum, the same
    beta*.  The column `stratum` then follows `event`.
    Returns the frame partition_id, time, event, [stratum,] x0 .. x{p-1}."""
    n, p = int(sample_size), int(p)
    if strata is not None and int(strata) < 1:
        raise ValueError("simulate_cox: strata must be a positive number of strata, got %r" % (strata,))
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    X = X.cpu().numpy()
    beta = np.zeros(p)
    beta[:int(0.4 * p)] = 1.0
    rng = np.random.default_rng(seed)
    T = rng.exponential(1.0, n) / np.exp(X @ beta)
    stratum = None
    if strata is not None:
        S = int(strata)
        stratum = np.arange(n) // int(partition_num) % S
        T = T * 2.0 ** (stratum - (S - 1) / 2.0)
    if censor_rate > 0:
        # E[P(C < T)] = rate / (rate + h) for a hazard h; one scalar rate from the median hazard is close enough for a simulator
        h = float(np.median(np.exp(X @ beta))) if n else 1.0
        rate = h * censor_rate / max(1e-12, 1.0 - censor_rate)
        C = rng.exponential(1.0 / rate, n)
    else:
        C = np.full(n, np.inf)
    time = np.minimum(T, C)
    event = (T <= C).astype(np.float64)
    if tie_levels:
        q = np.quantile(time, np.linspace(0, 1, int(tie_levels) + 1)[1:])
        time = q[np.minimum(np.searchsorted(q, time), len(q) - 1)]
    pid = (np.arange(n) % int(partition_num)).astype(np.float64)
    if stratum is not None:
        data = np.concatenate((pid[:, None], time[:, None], event[:, None], stratum.astype(np.float64)[:, None], X), 1)
        return pd.DataFrame(data, columns=["partition_id", "time", "event", "stratum"] + ["x" + str(i) for i in range(p)])
    data = np.concatenate((pid[:, None], time[:, None], event[:, None], X), 1)
    return pd.DataFrame(data, columns=["partition_id", "time", "event"] + ["x" + str(i) for i in range(p)])


def cox_order(time, part_id, strata=None):
    """The row permutation the Cox kernels read: one stable device sort keyed on (partition, -time), or with `strata` (an
    integer tensor of stratum codes per row) on (partition, stratum, -time).  Returns order int64.  part_id: int64 tensor of
    partition indices 0 .. K-1."""
    # stable sort by -time first, then a stable sort by partition keeps the time order inside every partition
    o1 = torch.sort(-time, stable=True).indices
    if strata is not None:
        o1 = o1[torch.sort(strata[o1], stable=True).indices]
    o2 = torch.sort(part_id[o1], stable=True).indices
    return o1[o2].contiguous()


def fit_cox_partitions(X, time, event, partition_num=None, part_offsets=None, names=None, tol=1e-13, max_iter=100, ties="breslow",
                       strata=None):
    """Cox map step for the partitions of one device-resident shard: X [n, p] fp64 row-major, time [n], event [n] (nonzero =
    event) on the GPU.  Partitions as fit_logistic_partitions: `part_offsets` (K+1 ints, contiguous row ranges) or
    `partition_num` (partition_id = i % K).  The rows are read through a permutation (one stable device sort keyed on
    (partition, -time)); nothing is copied.  ties: "breslow" (the default) or "efron" (the default of R's coxph, lifelines and
    scikit-survival), any letter case.  strata: None, or an integer tensor [n] of stratum codes on X's device: one common
    beta per partition and one baseline hazard per stratum (risk sets, tie groups and the cumulative hazard stop at stratum
    boundaries).  The codes are global: a stratum that spans partitions forms a risk set of its own in each of them.  With one
    event per stratum this is conditional logistic regression on matched sets.
    Returns MappedBlocks with `loglik` = log partial likelihood of that method per partition."""
    engine.cox_ties(ties)          # (a wrong name fails before any GPU work)
    engine.cox_strata(strata, X.shape[0])
    _require_dense_rows("fit_cox_partitions", X)
    X = engine.row_major(X)
    n, p = X.shape
    time = time.to(torch.float64).contiguous()
    event = event.to(torch.float64).contiguous()
    if part_offsets is None:
        K = int(partition_num) if partition_num else 1
        pid = torch.arange(n, device=X.device, dtype=torch.int64) % K
    else:
        offs = [int(v) for v in part_offsets]
        K = len(offs) - 1
        if offs[0] != 0 or offs[-1] != n:
            raise ValueError("fit_cox_partitions: part_offsets must run from 0 to n = %d" % n)
        pid = torch.repeat_interleave(torch.arange(K, device=X.device, dtype=torch.int64),
                                      torch.tensor([offs[k + 1] - offs[k] for k in range(K)], device=X.device))
    strata = engine.cox_strata_codes(strata, X.device)          # (once: cox_fit gets int32)
    order = cox_order(time, pid, strata)
    counts = torch.bincount(pid, minlength=K).cpu().tolist()
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + int(c))
    r = engine.cox_fit(X, time, event, order, offs, tol=tol, max_iter=max_iter, ties=ties, strata=strata)
    return _blocks(r, _column_names(names, p, False), n)


def cox_model(sample_df, time_name, event_name, dummy_info=[], dummy_factors_baseline=[], data_info=[], ties="breslow", strata=None):
    """Frame-level sibling of logistic_model / linear_model for survival data: one partition (a pandas frame) with a time
    and an event column.  Returns the p x (3+p) frame `par_id, coef, Sig_invMcoef, <features>`; a chunk that lacks an
    expected dummy level returns the all-zero block with a warning, as logistic_model does.  ties: as fit_cox_partitions.
    strata: a column name or a list of names; the distinct combinations of their values are the strata, and the columns are
    no features (KeyError for a name the frame lacks)."""
    engine.cox_ties(ties)
    codes = None
    if strata is not None:
        cols = [strata] if isinstance(strata, str) else list(strata)
        missing = [c for c in cols if c not in sample_df.columns]
        if missing or not cols:
            raise KeyError("cox_model: strata column(s) %r not in the frame" % (missing,))
        codes = sample_df.groupby(cols, sort=True, dropna=False).ngroup().to_numpy(dtype=np.int32)
        sample_df = sample_df.drop(columns=cols)
    features_df = sample_df.drop(columns=[event_name])
    Xd, names = _device_design(features_df, time_name, False, dummy_info, dummy_factors_baseline, data_info)
    if Xd is None:
        return _zero_block(names)
    sd = torch.from_numpy(np.ascontiguousarray(codes)).cuda() if codes is not None else None
    mb = fit_cox_partitions(Xd, _to_device(sample_df, time_name), _to_device(sample_df, event_name), names=names, ties=ties, strata=sd)
    return _first_block_frame(mb, "cox_model", hint=": monotone likelihood?")


# ---------------------------------------------------------------------------------------------
# Poisson regression map step (log link, optional offset / exposure): counts, event rates, traffic.  Partition k's local
# objective is its own log-likelihood sum y eta - mu - lgamma(y + 1) with eta = [1 | x]' beta + o; the block is coef = the
# partition's MLE, Sig_inv = the Fisher information [1 | X]' diag(mu) [1 | X] there, Sig_invMcoef = Sig_inv coef, so
# dlsa_mapred / dlsa apply unchanged.  The intercept is implicit, as in fit_logistic_partitions.
# ---------------------------------------------------------------------------------------------
def _simulate_glm(sample_size, p, partition_num, seed, base, coef_value, exposure, draw):
    """The body of the log-link simulators: simulate_poisson's rows and frame with y = draw(rng, mu), mu = base * exposure * exp(x beta*)."""
    n, p = int(sample_size), int(p)
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    X = X.cpu().numpy()
    beta = np.zeros(p)
    beta[:int(0.4 * p)] = float(coef_value)
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.5, 2.0, n) if exposure else np.ones(n)
    y = draw(rng, float(base) * e * np.exp(X @ beta))
    pid = (np.arange(n) % int(partition_num)).astype(np.float64)
    cols = [pid[:, None], y[:, None]] + ([e[:, None]] if exposure else []) + [X]
    return pd.DataFrame(np.concatenate(cols, 1),
                        columns=["partition_id", "y"] + (["exposure"] if exposure else []) + ["x" + str(i) for i in range(p)])


def simulate_poisson(sample_size, p, partition_num, seed=20260101, base_rate=1.0, coef_value=0.5, exposure=False):
    """Seeded count rows: x as simulate_logistic's (U(-0.5, 0.5), the rows of engine.synth), beta* = coef_value on the first int(0.4p)
    coefficients, y ~ Poisson(base_rate * exposure * exp(x beta*)) drawn with numpy; exposure (with exposure=True) ~ U(0.5, 2), else 1.
    partition_id = i % partition_num.  Returns the frame partition_id, y, [exposure,] x0 .. x{p-1}."""
    return _simulate_glm(sample_size, p, partition_num, seed, base_rate, coef_value, exposure,
                         lambda rng, mu: rng.poisson(mu).astype(np.float64))


def _poisson_offset(offset, exposure, n, device):
    if offset is not None and exposure is not None:
        raise ValueError("poisson: give an offset or an exposure, not both (offset = log exposure)")
    if exposure is not None:
        exposure = torch.as_tensor(exposure, dtype=torch.float64, device=device)
        if bool((exposure <= 0).any()):
            raise ValueError("poisson: exposure must be positive")
        offset = torch.log(exposure)
    if offset is None:
        return None
    offset = torch.as_tensor(offset, dtype=torch.float64, device=device).contiguous()
    if offset.numel() != n:
        raise ValueError("poisson: offset / exposure must have n = %d elements" % n)
    return offset


def _count_response(y):
    return "counts must be non-negative" if bool((y < 0).any()) else None


def _positive_response(y):
    return None if bool(((y > 0) & torch.isfinite(y)).all()) else "the response must be positive and finite"           # (NaN fails y > 0)


def _tweedie_response(y):
    if not bool(((y >= 0) & torch.isfinite(y)).all()):                # (NaN fails y >= 0)
        return "the response must be non-negative and finite"
    if y.numel() > 0 and not bool((y > 0).any()):
        return "no response is positive: the fit runs off to mu = 0"
    return None


def _binary_response(y):
    return None if bool(((y == 0) | (y == 1)).all()) else "the response must be 0 or 1"                                 # (NaN fails both)


# What a log-link family refuses in its response: y -> the message, or None for a response it takes.
_RESPONSE_REFUSED = {"poisson": _count_response, "negbin": _count_response, "gamma": _positive_response, "tweedie": _tweedie_response,
                     "probit": _binary_response, "cloglog": _binary_response}


def _alpha_not_zero(who, alpha, other):
    if alpha is not None and float(alpha) == 0.0:
        raise ValueError("%s: alpha = 0 is the Poisson model: use %s" % (who, other))


def _dispersion_or_none(who, dispersion, other):
    if dispersion is not None and not 0.0 < float(dispersion) < float("inf"):
        raise ValueError("%s: dispersion must be positive and finite (None estimates it)" % who)


# What fit_*_partitions / fit_*_design refuse in a family's scalar keyword before they look at the rows (the engine checks the rest):
# keyword -> check(who, value, who with the family's name replaced by its `other`).
_KEYWORD_REFUSED = {"alpha": _alpha_not_zero, "dispersion": _dispersion_or_none, "power": lambda who, power, other: engine.tweedie_power(who, power)}


def _glm_rows(fam, who, y, n, offset, exposure, device, scalars):
    """The response and the offset of a log-link fit of n rows as the engine takes them: (y fp64 contiguous, offset fp64 or None), on
    `device`; ValueError for a bad scalar keyword (in the C ABI's order), a wrong length, a response the family refuses or a bad offset /
    exposure, in this order."""
    for s in fam.scalars:
        _KEYWORD_REFUSED[s.name](who, scalars[s.name], who.replace(fam.name, fam.other) if fam.other else None)
    y = torch.as_tensor(y, device=device).to(torch.float64).contiguous()
    if y.numel() != n:
        raise ValueError("%s: y must have n = %d elements" % (who, n))
    refused = _RESPONSE_REFUSED[fam.name](y)
    if refused:
        raise ValueError("%s: %s" % (who, refused))
    return y, _poisson_offset(offset, exposure, n, device)


def _fit_glm_partitions(family, X, y, partition_num=None, part_offsets=None, fit_intercept=False, offset=None, exposure=None, names=None,
                        tol=1e-13, max_iter=100, **scalars):
    """The body of fit_<family>_partitions; `scalars`: the family's own keywords, as engine.<family>_fit_ex takes them."""
    fam, who = engine.GLM_FAMILIES[family], "fit_%s_partitions" % family
    _require_dense_rows(who, X)
    n, p = X.shape
    y, offset = _glm_rows(fam, who, y, n, offset, exposure, X.device, scalars)
    names = _column_names(names, p, fit_intercept)
    first, rows, step = _partitions(n, partition_num, part_offsets)
    r = getattr(engine, family + "_fit_ex")(engine.row_major(X), y, first, rows, row_step=step, offset=offset, fit_intercept=fit_intercept,
                                            tol=tol, max_iter=max_iter, **scalars)
    return _blocks(r, names, n, fam)


def _fit_glm_design(family, num, codes, y, spec, partition_num=None, part_offsets=None, offset=None, exposure=None, structured=True,
                    tol=1e-13, max_iter=100, **scalars):
    """The body of fit_<family>_design, on top of _fit_design; `scalars` as in _fit_glm_partitions."""
    fam, who = engine.GLM_FAMILIES[family], "fit_%s_design" % family
    _require_raw_rows(who, num, y)
    y, offset = _glm_rows(fam, who, y, y.numel(), offset, exposure, y.device, scalars)
    return _fit_design(getattr(engine, "onehot_%s_fit_ex" % family), getattr(engine, family + "_fit_ex"), num, codes, y, spec, partition_num,
                       part_offsets, structured, family=fam, offset=offset, tol=tol, max_iter=max_iter, **scalars)


def fit_poisson_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, offset=None, exposure=None, names=None,
                           tol=1e-13, max_iter=100):
    """Poisson map step for the partitions of one device-resident shard: X [n, p] fp64 row-major, y [n] counts on the GPU.
    Partitions as fit_logistic_partitions: `part_offsets` (K+1 ints, contiguous row ranges) or `partition_num` (partition_id = i % K,
    strided views: nothing is copied but the partition's counts and offsets, 8 bytes per row each).  With fit_intercept the ones column
    is implicit (results have p + 1 columns, `intercept` first).  `offset` [n] enters eta as is; `exposure` [n] is turned into
    offset = log(exposure).  Returns MappedBlocks with `loglik` = the full log-likelihood per partition."""
    return _fit_glm_partitions("poisson", X, y, partition_num, part_offsets, fit_intercept, offset, exposure, names, tol, max_iter)


def fit_poisson_design(num, codes, y, spec, partition_num=None, part_offsets=None, offset=None, exposure=None, structured=True,
                       tol=1e-13, max_iter=100):
    """Poisson map step for a design given by its RAW columns, the sibling of fit_logistic_design: num [n, q] fp64 (columns in
    spec.numeric_cols order), codes [n, f] int32 level codes (DesignSpec.encode) and counts y [n], all on the GPU.  With
    structured=True and a qualifying design (spec.onehot_plan(): <= 8 dense columns, <= 8 factors) the fit runs on the raw
    representation -- gather / histogram passes, the dense [n, p] matrix is never built; otherwise the matrix is built once by the
    design kernel and the dense Poisson fit runs on it.  An intercept is the spec's own constant column.  Partitions, `offset` and
    `exposure` as fit_poisson_partitions.  Same MappedBlocks either way (names = spec.names)."""
    return _fit_glm_design("poisson", num, codes, y, spec, partition_num, part_offsets, offset, exposure, structured, tol, max_iter)


def _count_raw_frame(sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info, dummy_factors_baseline, data_info):
    """The raw representation of one chunk for the structured count paths: (spec, plan or None when the design does not qualify,
    codes host array, unknown, y, offset column, exposure column).  The intercept is the plan's constant column."""
    frame = sample_df.drop(columns=[c for c in (offset_name, exposure_name) if c is not None])
    spec = DesignSpec.from_reference(list(frame.columns), Y_name, fit_intercept, dummy_info, dummy_factors_baseline, data_info)
    plan = spec.onehot_plan()
    if plan is None:
        return spec, None, None, False, None, None, None
    _, codes, unknown = spec.encode(frame, dummy_info, numeric=False)
    return spec, plan, codes, unknown, _to_device(sample_df, Y_name), _to_device(sample_df, offset_name), _to_device(sample_df, exposure_name)


def _count_frame(sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info, dummy_factors_baseline, data_info,
                 for_eval=False):
    """(X device design WITHOUT the ones column -- the kernels carry the intercept -- or None, names, y, offset, exposure) of one chunk."""
    frame = sample_df.drop(columns=[c for c in (offset_name, exposure_name) if c is not None])
    Xd, names = _device_design(frame, Y_name, False, dummy_info, dummy_factors_baseline, data_info, for_eval=for_eval)
    return (Xd, _column_names(names, len(names), fit_intercept), _to_device(sample_df, Y_name), _to_device(sample_df, offset_name),
            _to_device(sample_df, exposure_name))


def _count_model(family, structured, *chunk, **scalars):
    """The body of the log-link families' <family>_model: `chunk` is (sample_df, Y_name, fit_intercept, offset_name, exposure_name,
    dummy_info, dummy_factors_baseline, data_info), `scalars` the family's own keywords.  Returns (the block's frame, the MappedBlocks or
    None for the all-zero block of a skipped chunk)."""
    sample_df, fit_intercept, dummy_info = chunk[0], chunk[2], chunk[5]
    mb = None
    if structured and len(dummy_info) > 0:
        spec, plan, codes, unknown, yd, od, ed = _count_raw_frame(*chunk)
        if plan is not None:
            names = spec.names
            missing = spec.missing_levels(codes)
            if missing or unknown:
                _warn_missing_levels(missing, len(sample_df), names, fit_intercept, skip=True)
                return _zero_block(names), None
            mb = _fit_glm_design(family, spec.numeric_to_device(sample_df), torch.from_numpy(codes).cuda(), yd, spec, offset=od, exposure=ed,
                                 **scalars)
    if mb is None:
        Xd, names, yd, od, ed = _count_frame(*chunk)
        if Xd is None:
            return _zero_block(names), None
        mb = _fit_glm_partitions(family, Xd, yd, fit_intercept=fit_intercept, offset=od, exposure=ed,
                                 names=names[1:] if fit_intercept else names, **scalars)
    return _first_block_frame(mb, family + "_model"), mb


def _loglik_frame(par, run):
    """One row, a column per estimator column of `par`: the log-likelihood run(beta)[2] of one pass at that column."""
    pard = np.asarray(par, dtype=np.float64)
    out = {}
    for i in range(pard.shape[1]):
        b = torch.from_numpy(np.ascontiguousarray(pard[:, i])).cuda()
        out[par.columns[i]] = [float(run(b)[2].item())]
    return pd.DataFrame(out)


def _count_model_eval(family, par, structured, *chunk, **scalars):
    """The body of the log-link families' <family>_model_eval, `chunk` and `scalars` as in _count_model: the log-likelihood of every
    column of `par` by one pass without the information per column -- engine.<family>_pass or, on the raw representation,
    engine.onehot_<family>_pass."""
    sample_df, fit_intercept, dummy_info = chunk[0], chunk[2], chunk[5]
    run = None
    if structured and len(dummy_info) > 0:
        spec, plan, codes, unknown, yd, od, ed = _count_raw_frame(*chunk)
        if plan is not None:
            missing = spec.missing_levels(codes)
            if missing or unknown:
                _warn_missing_levels(missing, len(sample_df), spec.names, fit_intercept, skip=False)
            od = _poisson_offset(od, ed, yd.numel(), yd.device)
            num, cd = spec.numeric_to_device(sample_df), torch.from_numpy(codes).cuda()

            def run(b):
                return getattr(engine, "onehot_%s_pass" % family)(plan, num, cd, yd, b, offset=od, want_H=False, **scalars)
    if run is None:
        Xd, _, yd, od, ed = _count_frame(*chunk, for_eval=True)
        od = _poisson_offset(od, ed, yd.numel(), yd.device)
        X = engine.row_major(Xd)

        def run(b):
            return getattr(engine, family + "_pass")(X, yd, b, offset=od, fit_intercept=fit_intercept, want_H=False, **scalars)
    return _loglik_frame(par, run)


def poisson_model(sample_df, Y_name, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                  dummy_factors_baseline=[], data_info=[], structured=False):
    """Frame-level sibling of logistic_model / cox_model for count data: one partition (a pandas frame) with the count column
    Y_name and optionally an offset or an exposure column.  Returns the p x (3+p) frame `par_id, coef, Sig_invMcoef,
    [intercept,] <features>`; a chunk that lacks an expected dummy level returns the all-zero block with a warning.
    structured=True with a dummy_info and a qualifying design fits on the raw numerics + level codes (fit_poisson_design; the
    dense one-hot matrix is never built, the missing-level check runs on the codes); the default is the dense path."""
    return _count_model("poisson", structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                        dummy_factors_baseline, data_info)[0]


def poisson_model_eval(sample_df, Y_name, par, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                       dummy_factors_baseline=[], data_info=[], structured=False):
    """Log-likelihood (sum y eta - mu - lgamma(y + 1)) of every estimator column of `par` on one partition, shaped like
    logistic_model_eval's output: one row, a column per estimator.  structured=True with a dummy_info and a qualifying design
    evaluates on the raw numerics + level codes (one structured pass per estimator column); the default is the dense path."""
    return _count_model_eval("poisson", par, structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                             dummy_factors_baseline, data_info)


# ---------------------------------------------------------------------------------------------
# Probit and complementary log-log map steps for a 0/1 response, the two binary links beside the logit: P(y = 1) = Phi(eta) and
# P(y = 1) = 1 - exp(-e^eta) with eta = [1 | x]' beta + o.  The block is coef = the partition's MLE, Sig_inv = the OBSERVED information
# there (not the Fisher information R's glm weights by; the two agree in expectation), Sig_invMcoef = Sig_inv coef, so dlsa_mapred /
# dlsa / lars_lsa apply unchanged.  Offsets and exposure as in the Poisson step: under the cloglog link offset = log(exposure) is the
# model of "any event within the exposure", the grouped-time twin of the Cox step.  Dense rows only so far.
# ---------------------------------------------------------------------------------------------
BINARY_LINKS = ("probit", "cloglog")


def simulate_binary(sample_size, p, partition_num, link, seed=20260101, intercept=-0.5, coef_value=0.5, exposure=False):
    """Seeded 0/1 rows under `link` ("probit" or "cloglog"): x and beta* as simulate_poisson's, eta = intercept + log(exposure) + x beta*,
    y ~ Bernoulli(Phi(eta)) respectively Bernoulli(1 - exp(-e^eta)) drawn with numpy; exposure (with exposure=True) ~ U(0.5, 2), else 1.
    partition_id = i % partition_num.  Returns the frame partition_id, y, [exposure,] x0 .. x{p-1}."""
    if link not in BINARY_LINKS:
        raise ValueError("simulate_binary: link must be one of %s, got %r" % (", ".join(BINARY_LINKS), link))

    def draw(rng, mu):
        eta = np.log(mu)
        prob = -np.expm1(-mu) if link == "cloglog" else torch.special.ndtr(torch.from_numpy(eta)).numpy()
        return (rng.uniform(size=len(mu)) < prob).astype(np.float64)
    return _simulate_glm(sample_size, p, partition_num, seed, np.exp(float(intercept)), coef_value, exposure, draw)


def fit_probit_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, offset=None, exposure=None, names=None,
                          tol=1e-13, max_iter=100):
    """Probit map step for the partitions of one device-resident shard; arguments as fit_poisson_partitions, y in {0, 1} (anything else
    is refused).  A partition with an intercept and a single response value returns the all-zero block (status EMPTY).  Returns
    MappedBlocks with `loglik` = the log-likelihood per partition."""
    return _fit_glm_partitions("probit", X, y, partition_num, part_offsets, fit_intercept, offset, exposure, names, tol, max_iter)


def fit_cloglog_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, offset=None, exposure=None, names=None,
                           tol=1e-13, max_iter=100):
    """Complementary log-log map step for the partitions of one device-resident shard; arguments and results as fit_probit_partitions.
    `exposure` [n] (interval length, effort) is turned into offset = log(exposure)."""
    return _fit_glm_partitions("cloglog", X, y, partition_num, part_offsets, fit_intercept, offset, exposure, names, tol, max_iter)


def probit_model(sample_df, Y_name, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                 dummy_factors_baseline=[], data_info=[]):
    """Frame-level sibling of poisson_model for a 0/1 response under the probit link: one partition (a pandas frame) with the response
    column Y_name and optionally an offset or an exposure column.  Returns the p x (3+p) frame `par_id, coef, Sig_invMcoef, [intercept,]
    <features>`; a chunk that lacks an expected dummy level returns the all-zero block with a warning."""
    return _count_model("probit", False, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                        dummy_factors_baseline, data_info)[0]


def probit_model_eval(sample_df, Y_name, par, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                      dummy_factors_baseline=[], data_info=[]):
    """Probit log-likelihood of every estimator column of `par` on one partition, shaped like poisson_model_eval's output: one row, a
    column per estimator (one pass without the information per column)."""
    return _count_model_eval("probit", par, False, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                             dummy_factors_baseline, data_info)


def cloglog_model(sample_df, Y_name, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                  dummy_factors_baseline=[], data_info=[]):
    """probit_model under the complementary log-log link; exposure_name names the column of interval lengths or efforts."""
    return _count_model("cloglog", False, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                        dummy_factors_baseline, data_info)[0]


def cloglog_model_eval(sample_df, Y_name, par, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                       dummy_factors_baseline=[], data_info=[]):
    """probit_model_eval under the complementary log-log link."""
    return _count_model_eval("cloglog", par, False, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                             dummy_factors_baseline, data_info)


# ---------------------------------------------------------------------------------------------
# Negative-binomial (NB2) map step for overdispersed counts: Var y = mu + alpha mu^2.  On such data a Poisson block has the right
# coef and a Sig_inv too large by the dispersion factor, which the combine's weights and the AIC / BIC choice inherit.  beta and
# alpha are information-orthogonal, so the block stays [coef | Sig_inv coef | Sig_inv] over the regression coefficients with
# Sig_inv = [1 | X]' diag(mu / (1 + alpha mu)) [1 | X], and dlsa_mapred / dlsa apply unchanged.
# ---------------------------------------------------------------------------------------------
def simulate_negbin(sample_size, p, partition_num, alpha, seed=20260101, base_rate=1.0, coef_value=0.5, exposure=False):
    """simulate_poisson's rows and frame with overdispersed counts: y ~ Poisson(mu * G), G ~ Gamma(shape 1 / alpha, scale alpha)
    (mean 1), so y ~ NB2(mu, alpha) with mu = base_rate * exposure * exp(x beta*)."""
    alpha = float(alpha)
    if not alpha > 0:
        raise ValueError("simulate_negbin: alpha must be positive (alpha = 0 is simulate_poisson)")
    return _simulate_glm(sample_size, p, partition_num, seed, base_rate, coef_value, exposure,
                         lambda rng, mu: rng.poisson(mu * rng.gamma(1.0 / alpha, alpha, len(mu))).astype(np.float64))


def fit_negbin_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, offset=None, exposure=None, alpha=None,
                          names=None, tol=1e-13, max_iter=100):
    """Negative-binomial map step for the partitions of one device-resident shard; arguments as fit_poisson_partitions.  alpha=None
    estimates every partition's own dispersion (a partition that is not overdispersed gets alpha = 0 and exactly its Poisson block);
    alpha > 0 fits every partition at that common dispersion (e.g. combine_dispersion of a first map step); alpha = 0 is refused:
    that is fit_poisson_partitions.  Returns MappedBlocks with `loglik` = the full log-likelihood per partition and
    `extra` = {"alpha", "alpha_info" (the information about log alpha), "pearson"} per partition."""
    return _fit_glm_partitions("negbin", X, y, partition_num, part_offsets, fit_intercept, offset, exposure, names, tol, max_iter, alpha=alpha)


def fit_negbin_design(num, codes, y, spec, partition_num=None, part_offsets=None, offset=None, exposure=None, alpha=None,
                      structured=True, tol=1e-13, max_iter=100):
    """Negative-binomial map step for a design given by its RAW columns, the sibling of fit_poisson_design: num [n, q] fp64, codes
    [n, f] int32 level codes and counts y [n], all on the GPU.  With structured=True and a qualifying design (spec.onehot_plan())
    the fit runs on the raw representation -- the dense [n, p] matrix is never built; otherwise the matrix is built once by the
    design kernel and the dense NB2 fit runs on it.  An intercept is the spec's own constant column.  Partitions, `offset` and
    `exposure` as fit_poisson_partitions, alpha as fit_negbin_partitions (alpha = 0 is refused: that is fit_poisson_design).  Same
    MappedBlocks either way (names = spec.names, `extra` = {"alpha", "alpha_info", "pearson"} per partition)."""
    return _fit_glm_design("negbin", num, codes, y, spec, partition_num, part_offsets, offset, exposure, structured, tol, max_iter, alpha=alpha)


def combine_dispersion(mb):
    """The common dispersion of a negative-binomial map step: the information-weighted mean of log alpha_k over the partitions with
    status OK and alpha_k > 0 (weights alpha_info), returned as alpha -- the one-round combine of the dispersion, to be passed as
    `alpha=` to a second map step.  0.0 when no partition is overdispersed."""
    al, info = mb.extra["alpha"], mb.extra["alpha_info"]
    use = [k for k in range(len(al)) if mb.status[k] == 0 and al[k] > 0 and info[k] > 0]
    if not use:
        return 0.0
    wsum = sum(info[k] for k in use)
    return float(np.exp(sum(info[k] * np.log(al[k]) for k in use) / wsum))


def negbin_model(sample_df, Y_name, fit_intercept=False, offset_name=None, exposure_name=None, alpha=None, dummy_info=[],
                 dummy_factors_baseline=[], data_info=[], structured=False):
    """Frame-level sibling of poisson_model for overdispersed counts: one partition (a pandas frame) with the count column Y_name and
    optionally an offset or an exposure column; alpha as fit_negbin_partitions.  Returns the p x (3+p) frame `par_id, coef,
    Sig_invMcoef, [intercept,] <features>` with the dispersion in `out.attrs["alpha"]`; a chunk that lacks an expected dummy level
    returns the all-zero block with a warning.  structured=True with a dummy_info and a qualifying design fits on the raw numerics +
    level codes (fit_negbin_design; the dense one-hot matrix is never built, the missing-level check runs on the codes); the
    default is the dense path."""
    out, mb = _count_model("negbin", structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                           dummy_factors_baseline, data_info, alpha=alpha)
    out.attrs["alpha"] = mb.extra["alpha"][0] if mb is not None else 0.0         # (a skipped chunk's all-zero block: 0)
    return out


def negbin_model_eval(sample_df, Y_name, par, alpha, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                      dummy_factors_baseline=[], data_info=[], structured=False):
    """Negative-binomial log-likelihood at dispersion alpha > 0 of every estimator column of `par` on one partition, shaped like
    poisson_model_eval's output: one row, a column per estimator (one pass without the information per column).  structured=True
    with a dummy_info and a qualifying design evaluates on the raw numerics + level codes (one structured pass per estimator
    column); the default is the dense path."""
    return _count_model_eval("negbin", par, structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                             dummy_factors_baseline, data_info, alpha=alpha)


# ---------------------------------------------------------------------------------------------
# Gamma regression map step (log link) for positive, right-skewed continuous responses: claim severity, cost, duration, delay --
# the severity half of the frequency / severity pair whose frequency half is the Poisson / NB2 step above.  Var y = phi mu^2.  beta^
# does not depend on the dispersion phi, the information does: Sig_inv = [1 | X]' diag(y / mu) [1 | X] / phi.  So every partition
# estimates its own phi (Pearson: P / (n - p)) for its block, the combine's weights and the AIC / BIC choice then carry the right
# scale, and dlsa_mapred / dlsa apply unchanged.
# ---------------------------------------------------------------------------------------------
def simulate_gamma(sample_size, p, partition_num, shape, seed=20260101, base_mean=1.0, coef_value=0.5, exposure=False):
    """simulate_poisson's rows and frame with a positive continuous response: y ~ Gamma(shape, scale mu / shape) (mean mu, dispersion
    1 / shape) with mu = base_mean * exposure * exp(x beta*)."""
    shape = float(shape)
    if not shape > 0:
        raise ValueError("simulate_gamma: shape must be positive")
    return _simulate_glm(sample_size, p, partition_num, seed, base_mean, coef_value, exposure, lambda rng, mu: rng.gamma(shape, mu / shape))


def fit_gamma_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, offset=None, exposure=None, dispersion=None,
                         names=None, tol=1e-13, max_iter=100):
    """Gamma (log link) map step for the partitions of one device-resident shard; arguments as fit_poisson_partitions, y > 0.
    dispersion=None estimates every partition's own dispersion (Pearson) for its block; dispersion > 0 gives every block that common
    dispersion (e.g. combine_gamma_dispersion of a first map step).  Returns MappedBlocks with `loglik` = the full log-likelihood per
    partition at the dispersion used and `extra` = {"dispersion", "pearson", "deviance", "df"} per partition."""
    return _fit_glm_partitions("gamma", X, y, partition_num, part_offsets, fit_intercept, offset, exposure, names, tol, max_iter,
                               dispersion=dispersion)


def fit_gamma_design(num, codes, y, spec, partition_num=None, part_offsets=None, offset=None, exposure=None, dispersion=None,
                     structured=True, tol=1e-13, max_iter=100):
    """Gamma map step for a design given by its RAW columns, the sibling of fit_poisson_design: num [n, q] fp64, codes [n, f] int32
    level codes and responses y [n] > 0, all on the GPU.  With structured=True and a qualifying design (spec.onehot_plan()) the fit
    runs on the raw representation -- the dense [n, p] matrix is never built; otherwise the matrix is built once by the design kernel
    and the dense Gamma fit runs on it.  An intercept is the spec's own constant column.  Partitions, `offset` and `exposure` as
    fit_poisson_partitions, dispersion as fit_gamma_partitions.  Same MappedBlocks either way (names = spec.names)."""
    return _fit_glm_design("gamma", num, codes, y, spec, partition_num, part_offsets, offset, exposure, structured, tol, max_iter,
                           dispersion=dispersion)


def combine_gamma_dispersion(mb):
    """The common dispersion of a Gamma map step: the pooled Pearson estimate sum_k P_k / sum_k (n_k - p) over the partitions with
    status OK -- the exact one-round combine of the dispersion, to be passed as `dispersion=` to a second map step.  NaN when no
    partition qualifies."""
    return _pooled_pearson_dispersion(mb)


def _pooled_pearson_dispersion(mb):
    """sum_k P_k / sum_k df_k over the partitions with status OK and df_k > 0 (NaN without one), from a map step whose `extra` holds
    `pearson` and `df`: the Gamma and the Tweedie fits'."""
    P, df = mb.extra["pearson"], mb.extra["df"]
    use = [k for k in range(len(P)) if mb.status[k] == 0 and df[k] > 0]
    if not use:
        return float("nan")
    return float(sum(P[k] for k in use) / sum(df[k] for k in use))


def gamma_model(sample_df, Y_name, fit_intercept=False, offset_name=None, exposure_name=None, dispersion=None, dummy_info=[],
                dummy_factors_baseline=[], data_info=[], structured=False):
    """Frame-level sibling of poisson_model for a positive continuous response: one partition (a pandas frame) with the response
    column Y_name and optionally an offset or an exposure column; dispersion as fit_gamma_partitions.  Returns the p x (3+p) frame
    `par_id, coef, Sig_invMcoef, [intercept,] <features>` with the dispersion used in `out.attrs["dispersion"]`; a chunk that lacks an
    expected dummy level returns the all-zero block with a warning.  structured=True with a dummy_info and a qualifying design fits
    on the raw numerics + level codes (fit_gamma_design); the default is the dense path."""
    out, mb = _count_model("gamma", structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                           dummy_factors_baseline, data_info, dispersion=dispersion)
    out.attrs["dispersion"] = mb.extra["dispersion"][0] if mb is not None else 0.0      # (a skipped chunk's all-zero block: 0)
    return out


def gamma_model_eval(sample_df, Y_name, par, dispersion, fit_intercept=False, offset_name=None, exposure_name=None, dummy_info=[],
                     dummy_factors_baseline=[], data_info=[], structured=False):
    """Gamma log-likelihood at dispersion > 0 of every estimator column of `par` on one partition, shaped like poisson_model_eval's
    output: one row, a column per estimator (one pass without the information per column).  structured=True with a dummy_info and a
    qualifying design evaluates on the raw numerics + level codes; the default is the dense path."""
    return _count_model_eval("gamma", par, structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                             dummy_factors_baseline, data_info, dispersion=dispersion)


# ---------------------------------------------------------------------------------------------
# Tweedie (compound Poisson-Gamma) map step, log link, variance power 1 < xi < 2: a response that is exactly zero for many rows and
# positive, right-skewed for the rest -- pure premium, cost per policy, rainfall, spend per visitor: the frequency / severity pair
# above as one model.  Var y = phi mu^xi.  xi is given by the caller.  beta^ does not depend on phi, the information does: Sig_inv =
# [1 | X]' diag((xi - 1) y mu^(1 - xi) + (2 - xi) mu^(2 - xi)) [1 | X] / phi, so every partition estimates its own phi (Pearson) for its
# block, as the Gamma step does, and dlsa_mapred / dlsa apply unchanged.  `loglik` is the quasi-log-likelihood (the part of the log
# density that depends on beta): the series factor of the Tweedie density is out of scope, and with it a full likelihood, AIC
# across xi and a profile estimate of xi.
# ---------------------------------------------------------------------------------------------
def simulate_tweedie(sample_size, p, partition_num, power, dispersion, seed=20260101, base_mean=1.0, coef_value=0.5, exposure=False):
    """simulate_poisson's rows and frame with a compound Poisson-Gamma response of mean mu = base_mean * exposure * exp(x beta*) and
    variance dispersion * mu^power: N ~ Poisson(mu^(2 - power) / (dispersion (2 - power))), y = the sum of N Gamma draws = Gamma(shape
    N (2 - power) / (power - 1), scale dispersion (power - 1) mu^(power - 1)), y = 0 at N = 0."""
    xi, phi = engine.tweedie_power("simulate_tweedie", power), float(dispersion)
    if not 0.0 < phi < float("inf"):
        raise ValueError("simulate_tweedie: dispersion must be positive and finite")
    return _simulate_glm(sample_size, p, partition_num, seed, base_mean, coef_value, exposure, lambda rng, mu: _tweedie_draw(rng, mu, xi, phi))


def _tweedie_draw(rng, mu, power, dispersion):
    """Compound Poisson-Gamma draws with mean mu (an array) and variance dispersion * mu^power, 1 < power < 2."""
    N = rng.poisson(mu ** (2.0 - power) / (dispersion * (2.0 - power)))
    draws = rng.gamma(np.maximum(N, 1) * ((2.0 - power) / (power - 1.0)), dispersion * (power - 1.0) * mu ** (power - 1.0))
    return np.where(N > 0, draws, 0.0)


def fit_tweedie_partitions(X, y, partition_num=None, part_offsets=None, fit_intercept=False, offset=None, exposure=None, power=1.5,
                           dispersion=None, names=None, tol=1e-13, max_iter=100):
    """Tweedie (log link, Var y = dispersion * mu^power, 1 < power < 2 given) map step for the partitions of one device-resident
    shard; arguments as fit_poisson_partitions, y >= 0 with at least one positive response in every partition.  dispersion as
    fit_gamma_partitions (None: every partition's own Pearson estimate; > 0: that common one, e.g. combine_tweedie_dispersion of a
    first map step).  Returns MappedBlocks with `loglik` = the quasi-log-likelihood per partition at the dispersion used (the density's
    series factor is not computed) and `extra` = {"dispersion", "pearson", "deviance", "df"} per partition."""
    return _fit_glm_partitions("tweedie", X, y, partition_num, part_offsets, fit_intercept, offset, exposure, names, tol, max_iter,
                               power=power, dispersion=dispersion)


def fit_tweedie_design(num, codes, y, spec, partition_num=None, part_offsets=None, offset=None, exposure=None, power=1.5,
                       dispersion=None, structured=True, tol=1e-13, max_iter=100):
    """Tweedie map step for a design given by its RAW columns, the sibling of fit_gamma_design: num [n, q] fp64, codes [n, f] int32
    level codes and responses y [n] >= 0, all on the GPU.  With structured=True and a qualifying design (spec.onehot_plan()) the fit
    runs on the raw representation -- the dense [n, p] matrix is never built; otherwise the matrix is built once by the design kernel
    and the dense Tweedie fit runs on it.  An intercept is the spec's own constant column.  Partitions, `offset` and `exposure` as
    fit_poisson_partitions, power and dispersion as fit_tweedie_partitions.  Same MappedBlocks either way (names = spec.names)."""
    return _fit_glm_design("tweedie", num, codes, y, spec, partition_num, part_offsets, offset, exposure, structured, tol, max_iter,
                           power=power, dispersion=dispersion)


def combine_tweedie_dispersion(mb):
    """The common dispersion of a Tweedie map step: the pooled Pearson estimate sum_k P_k / sum_k (n_k - p) over the partitions with
    status OK, as combine_gamma_dispersion -- to be passed as `dispersion=` to a second map step.  NaN when no partition qualifies."""
    return _pooled_pearson_dispersion(mb)


def tweedie_model(sample_df, Y_name, fit_intercept=False, offset_name=None, exposure_name=None, power=1.5, dispersion=None,
                  dummy_info=[], dummy_factors_baseline=[], data_info=[], structured=False):
    """Frame-level sibling of gamma_model for a non-negative response with exact zeros: one partition (a pandas frame) with the
    response column Y_name and optionally an offset or an exposure column; power and dispersion as fit_tweedie_partitions.  Returns
    the p x (3+p) frame `par_id, coef, Sig_invMcoef, [intercept,] <features>` with the dispersion used in `out.attrs["dispersion"]`
    and the power in `out.attrs["power"]`; a chunk that lacks an expected dummy level returns the all-zero block with a warning.
    structured=True with a dummy_info and a qualifying design fits on the raw numerics + level codes (fit_tweedie_design); the
    default is the dense path."""
    out, mb = _count_model("tweedie", structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                           dummy_factors_baseline, data_info, power=power, dispersion=dispersion)
    out.attrs["dispersion"] = mb.extra["dispersion"][0] if mb is not None else 0.0      # (a skipped chunk's all-zero block: 0)
    out.attrs["power"] = float(power)
    return out


def tweedie_model_eval(sample_df, Y_name, par, power, dispersion, fit_intercept=False, offset_name=None, exposure_name=None,
                       dummy_info=[], dummy_factors_baseline=[], data_info=[], structured=False):
    """Tweedie quasi-log-likelihood at (power, dispersion > 0) of every estimator column of `par` on one partition, shaped like
    poisson_model_eval's output: one row, a column per estimator (one pass without the information per column).  The values compare
    estimators at this (power, dispersion) only.  structured=True with a dummy_info and a qualifying design evaluates on the raw
    numerics + level codes; the default is the dense path."""
    return _count_model_eval("tweedie", par, structured, sample_df, Y_name, fit_intercept, offset_name, exposure_name, dummy_info,
                             dummy_factors_baseline, data_info, power=power, dispersion=dispersion)


# ---------------------------------------------------------------------------------------------
# Multinomial logistic (softmax) map step for a response with C unordered classes (delay cause, product chosen, diagnosis group).
# Class 0 is the reference class; the parameter is class-major, theta = [beta_1 | ... | beta_J] with J = C - 1, so a partition's block
# is [coef | Sig_inv coef | Sig_inv] over J * pe coefficients named "<name>:<j>", and dlsa_mapred applies unchanged.  dlsa() knows
# one unpenalised intercept at position 0 through fit_intercept=True; multinomial blocks with intercepts go through
# dlsa(..., unpenalized="intercepts") (intercept_columns below), those without through dlsa(..., fit_intercept=False).
# ---------------------------------------------------------------------------------------------
def simulate_multinomial(sample_size, p, partition_num, classes, seed=20260101, coef_value=1.0):
    """Seeded rows with a class response: x as simulate_logistic's (U(-0.5, 0.5), the rows of engine.synth), beta*_j = +-coef_value
    (the sign alternating with the class j = 1 .. classes - 1) on the first int(0.4p) coefficients, y ~ softmax(0, x beta*_1, ...)
    drawn with numpy as class codes 0 .. classes - 1.  partition_id = i % partition_num.  Returns the frame partition_id, y,
    x0 .. x{p-1}."""
    n, p, C = int(sample_size), int(p), int(classes)
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    X = X.cpu().numpy()
    B = np.zeros((p, C))
    for j in range(1, C):
        B[:int(0.4 * p), j] = float(coef_value) * (1.0 if j % 2 else -1.0)
    eta = X @ B
    pr = np.exp(eta - eta.max(1, keepdims=True))
    cdf = np.cumsum(pr / pr.sum(1, keepdims=True), 1)
    rng = np.random.default_rng(seed)
    y = np.minimum((rng.random(n)[:, None] > cdf).sum(1), C - 1).astype(np.float64)
    pid = (np.arange(n) % int(partition_num)).astype(np.float64)
    return pd.DataFrame(np.concatenate([pid[:, None], y[:, None], X], 1), columns=["partition_id", "y"] + ["x" + str(i) for i in range(p)])


def intercept_columns(names):
    """Indices of the intercept columns among `names`: "intercept" (one-response families) and "intercept:<j>" (class j of a
    multinomial block) -- what dlsa(..., unpenalized="intercepts") keeps out of the penalty."""
    out = []
    for i, nm in enumerate(names):
        head, sep, tail = str(nm).partition(":")
        if head == "intercept" and (not sep or tail.isdigit()):
            out.append(i)
    return out


def multinomial_column_names(names, classes):
    """The J * pe column names of a multinomial block: "<name>:<j>" for j = 1 .. classes - 1, class-major (`names` = one class
    block's names, `intercept` first when the fit carries one)."""
    return ["%s:%d" % (nm, j) for j in range(1, int(classes)) for nm in names]


def fit_multinomial_partitions(X, y, classes, partition_num=None, part_offsets=None, fit_intercept=False, names=None, tol=1e-13,
                               max_iter=100):
    """Multinomial logistic map step for the partitions of one device-resident shard: X [n, p] fp64 row-major, y [n] class codes
    0 .. classes - 1 on the GPU (class 0 is the reference).  Partitions and the implicit intercept as fit_poisson_partitions.  Every
    partition with rows must hold every class.  Returns MappedBlocks over the (classes - 1) * pe coefficients "<name>:<j>",
    "intercept:<j>" first in each class block, with `loglik` = the log-likelihood per partition."""
    _require_dense_rows("fit_multinomial_partitions", X)
    n, p = X.shape
    y = torch.as_tensor(y, device=X.device).to(torch.float64).contiguous()
    if y.numel() != n:
        raise ValueError("fit_multinomial_partitions: y must have n = %d elements" % n)
    classes = engine.multinomial_classes("fit_multinomial_partitions", classes, p + (1 if fit_intercept else 0))
    names = multinomial_column_names(_column_names(names, p, fit_intercept), classes)
    first, rows, step = _partitions(n, partition_num, part_offsets)
    r = engine.multinomial_fit_ex(engine.row_major(X), y, first, rows, row_step=step, classes=classes, fit_intercept=fit_intercept,
                                  tol=tol, max_iter=max_iter)
    return _blocks(r, names, n)


def fit_multinomial_design(num, codes, y, spec, classes, partition_num=None, part_offsets=None, structured=True, tol=1e-13,
                           max_iter=100):
    """Multinomial logistic map step for a design given by its RAW columns, the sibling of fit_poisson_design: num [n, q] fp64, codes
    [n, f] int32 level codes (DesignSpec.encode) and the class codes y [n] (0 .. classes - 1, class 0 the reference), all on the
    GPU.  With structured=True and a qualifying design (spec.onehot_plan()) the fit runs on the raw representation -- the dense
    [n, p] matrix is never built; otherwise the matrix is built once by the design kernel and the dense multinomial fit runs on it
    without an implicit intercept.  An intercept is the spec's own constant column, one column of every class block.  Partitions as
    fit_poisson_partitions; every partition with rows must hold every class.  Same MappedBlocks either way over the
    (classes - 1) * p coefficients multinomial_column_names(spec.names, classes)."""
    _require_raw_rows("fit_multinomial_design", num, y)
    y = y.to(torch.float64).contiguous()
    classes = engine.multinomial_classes("fit_multinomial_design", classes, len(spec.names))
    return _fit_design(engine.onehot_multinomial_fit_ex, engine.multinomial_fit_ex, num, codes, y, spec, partition_num, part_offsets,
                       structured, names=multinomial_column_names(spec.names, classes), classes=classes, tol=tol, max_iter=max_iter)


def _multinomial_codes_frame(who, sample_df, Y_name, classes):
    """(the chunk with its response column Y_name turned from the labels `classes` -- reference first -- into class codes, C)."""
    labels = list(classes)
    if len(set(labels)) != len(labels):
        raise ValueError("%s: classes must be distinct labels, reference first" % who)
    codes = sample_df[Y_name].map({lab: float(i) for i, lab in enumerate(labels)})
    if codes.isna().any():
        raise ValueError("%s: column %r holds values that are not among classes=%r" % (who, Y_name, labels))
    return sample_df.assign(**{Y_name: codes.astype(np.float64)}), len(labels)


def _multinomial_frame(who, sample_df, Y_name, classes, fit_intercept, dummy_info, dummy_factors_baseline, data_info, for_eval=False):
    """(X device design without the ones column or None, the J * pe names, the class codes on the device, C) of one chunk whose
    response column holds the labels `classes` (reference first)."""
    frame, C = _multinomial_codes_frame(who, sample_df, Y_name, classes)
    Xd, names = _device_design(frame, Y_name, False, dummy_info, dummy_factors_baseline, data_info, for_eval=for_eval)
    return Xd, _column_names(names, len(names), fit_intercept), _to_device(frame, Y_name), C


def multinomial_model(sample_df, Y_name, classes, fit_intercept=False, dummy_info=[], dummy_factors_baseline=[], data_info=[],
                      tol=1e-13, max_iter=100, structured=False):
    """Frame-level sibling of logistic_model for a response with more than two unordered classes: one partition (a pandas frame)
    whose column Y_name holds the labels listed in `classes`, the reference class first.  `classes` is required: a partition cannot
    discover the classes it lacks.  Returns the stacked (J pe) x (3 + J pe) frame `par_id, coef, Sig_invMcoef, <name>:<j> ...`; a
    chunk that lacks an expected dummy level returns the all-zero block with a warning.
    structured=True with a dummy_info and a qualifying design fits on the raw numerics + level codes (fit_multinomial_design; the
    dense one-hot matrix is never built, the missing-level check runs on the codes); the default is the dense path."""
    if structured and len(dummy_info) > 0:
        frame, C = _multinomial_codes_frame("multinomial_model", sample_df, Y_name, classes)
        spec, plan, codes, unknown, yd, _, _ = _count_raw_frame(frame, Y_name, fit_intercept, None, None, dummy_info,
                                                                dummy_factors_baseline, data_info)
        if plan is not None:
            missing = spec.missing_levels(codes)
            if missing or unknown:
                _warn_missing_levels(missing, len(sample_df), spec.names, fit_intercept, skip=True)
                return _zero_block(multinomial_column_names(spec.names, C))
            mb = fit_multinomial_design(spec.numeric_to_device(frame), torch.from_numpy(codes).cuda(), yd, spec, C, tol=tol,
                                        max_iter=max_iter)
            return _first_block_frame(mb, "multinomial_model")
    Xd, names, yd, C = _multinomial_frame("multinomial_model", sample_df, Y_name, classes, fit_intercept, dummy_info,
                                          dummy_factors_baseline, data_info)
    if Xd is None:
        return _zero_block(multinomial_column_names(names, C))
    mb = fit_multinomial_partitions(Xd, yd, C, fit_intercept=fit_intercept, names=names[1:] if fit_intercept else names, tol=tol,
                                    max_iter=max_iter)
    return _first_block_frame(mb, "multinomial_model")


def multinomial_model_eval(sample_df, Y_name, par, classes, fit_intercept=False, dummy_info=[], dummy_factors_baseline=[], data_info=[],
                           structured=False):
    """Log-likelihood (sum log p_y) of every estimator column of `par` (J * pe rows, class-major) on one partition, shaped like
    logistic_model_eval's output: one row, a column per estimator (one pass without the information per column).  structured=True
    with a dummy_info and a qualifying design runs the passes on the raw numerics + level codes."""
    run = None
    if structured and len(dummy_info) > 0:
        frame, C = _multinomial_codes_frame("multinomial_model_eval", sample_df, Y_name, classes)
        spec, plan, codes, unknown, yd, _, _ = _count_raw_frame(frame, Y_name, fit_intercept, None, None, dummy_info,
                                                                dummy_factors_baseline, data_info)
        if plan is not None:
            missing = spec.missing_levels(codes)
            if missing or unknown:
                _warn_missing_levels(missing, len(sample_df), spec.names, fit_intercept, skip=False)
            num, cd = spec.numeric_to_device(frame), torch.from_numpy(codes).cuda()

            def run(b):
                return engine.onehot_multinomial_pass(plan, num, cd, yd, b, C, want_H=False)
    if run is None:
        Xd, _, yd, C = _multinomial_frame("multinomial_model_eval", sample_df, Y_name, classes, fit_intercept, dummy_info,
                                          dummy_factors_baseline, data_info, for_eval=True)
        X = engine.row_major(Xd)

        def run(b):
            return engine.multinomial_pass(X, yd, b, C, fit_intercept=fit_intercept, want_H=False)
    return _loglik_frame(par, run)


# ---------------------------------------------------------------------------------------------
# Ordinal (proportional-odds) map step for a response with C ORDERED classes (delay bucket, credit grade, severity score):
# logit P(y <= j) = alpha_{j+1} - x'beta.  A partition's block is [coef | Sig_inv coef | Sig_inv] over the J + p coefficients
# ["intercept:1" .. "intercept:J"] + names, the J = C - 1 cutpoints first, so dlsa_mapred applies unchanged and
# dlsa(..., unpenalized="intercepts") keeps the cutpoints out of the penalty (intercept_columns above).
# ---------------------------------------------------------------------------------------------
def ordinal_column_names(names, classes):
    """The J + p column names of an ordinal block: the cutpoints "intercept:1" .. "intercept:J" (J = classes - 1), then `names`."""
    return ["intercept:%d" % j for j in range(1, int(classes))] + list(names)


def simulate_ordinal(sample_size, p, partition_num, classes, seed=20260101, coef_value=1.0):
    """Seeded rows with an ordered class response: x as simulate_logistic's (U(-0.5, 0.5), the rows of engine.synth), beta* =
    coef_value on the first int(0.4p) coefficients, the cutpoints alpha*_j = logit(j / classes) (equal class shares at eta = 0),
    y = the number of cutpoints below eta + a logistic draw (numpy), class codes 0 .. classes - 1.  partition_id = i %
    partition_num.  Returns the frame partition_id, y, x0 .. x{p-1}."""
    n, p, C = int(sample_size), int(p), int(classes)
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    X = X.cpu().numpy()
    beta = np.zeros(p)
    beta[:int(0.4 * p)] = float(coef_value)
    share = np.arange(1, C) / C
    alpha = np.log(share / (1.0 - share))
    rng = np.random.default_rng(seed)
    latent = X @ beta + rng.logistic(size=n)
    y = (latent[:, None] > alpha[None, :]).sum(1).astype(np.float64)
    pid = (np.arange(n) % int(partition_num)).astype(np.float64)
    return pd.DataFrame(np.concatenate([pid[:, None], y[:, None], X], 1), columns=["partition_id", "y"] + ["x" + str(i) for i in range(p)])


def fit_ordinal_partitions(X, y, classes, partition_num=None, part_offsets=None, names=None, tol=1e-13, max_iter=100):
    """Ordinal (proportional-odds) map step for the partitions of one device-resident shard: X [n, p] fp64 row-major WITHOUT a
    constant column (the cutpoints are the intercepts), y [n] class codes 0 .. classes - 1 on the GPU.  Partitions as
    fit_poisson_partitions.  Every partition with rows must hold every class.  Returns MappedBlocks over the (classes - 1) + p
    coefficients ordinal_column_names(names, classes), with `loglik` = the log-likelihood per partition."""
    _require_dense_rows("fit_ordinal_partitions", X)
    n, p = X.shape
    y = torch.as_tensor(y, device=X.device).to(torch.float64).contiguous()
    if y.numel() != n:
        raise ValueError("fit_ordinal_partitions: y must have n = %d elements" % n)
    classes = engine.ordinal_classes("fit_ordinal_partitions", classes, p)
    names = ordinal_column_names(_column_names(names, p, False), classes)
    first, rows, step = _partitions(n, partition_num, part_offsets)
    r = engine.ordinal_fit_ex(engine.row_major(X), y, first, rows, row_step=step, classes=classes, tol=tol, max_iter=max_iter)
    return _blocks(r, names, n)


def fit_ordinal_design(num, codes, y, spec, classes, partition_num=None, part_offsets=None, structured=True, tol=1e-13, max_iter=100):
    """Ordinal (proportional-odds) map step for a design given by its RAW columns, the sibling of fit_multinomial_design: num [n, q]
    fp64, codes [n, f] int32 level codes (DesignSpec.encode) and the class codes y [n] (0 .. classes - 1, lowest first), all on the
    GPU.  The spec must have NO constant column (ValueError otherwise): the cutpoints are the intercepts.  With structured=True and a
    qualifying design (spec.onehot_plan()) the fit runs on the raw representation -- the dense [n, p] matrix is never built;
    otherwise the matrix is built once by the design kernel and the dense ordinal fit runs on it.  Partitions as
    fit_poisson_partitions; every partition with rows must hold every class.  Same MappedBlocks either way over the (classes - 1) + p
    coefficients ordinal_column_names(spec.names, classes)."""
    _require_raw_rows("fit_ordinal_design", num, y)
    if any(int(k) == 0 for k in spec.kind):
        raise ValueError("fit_ordinal_design: the design has a constant column; the cutpoints are the intercepts of an ordinal "
                         "model, so build the spec with fit_intercept=False")
    y = y.to(torch.float64).contiguous()
    classes = engine.ordinal_classes("fit_ordinal_design", classes, len(spec.names))
    return _fit_design(engine.onehot_ordinal_fit_ex, engine.ordinal_fit_ex, num, codes, y, spec, partition_num, part_offsets,
                       structured, names=ordinal_column_names(spec.names, classes), classes=classes, tol=tol, max_iter=max_iter)


def _ordinal_frame(who, sample_df, Y_name, classes, dummy_info, dummy_factors_baseline, data_info, for_eval=False):
    """(X device design without a ones column or None, its p names, the class codes on the device, C) of one chunk whose response
    column holds the labels `classes`, lowest first."""
    frame, C = _multinomial_codes_frame(who, sample_df, Y_name, classes)
    Xd, names = _device_design(frame, Y_name, False, dummy_info, dummy_factors_baseline, data_info, for_eval=for_eval)
    return Xd, list(names), _to_device(frame, Y_name), C


def ordinal_model(sample_df, Y_name, classes, dummy_info=[], dummy_factors_baseline=[], data_info=[], tol=1e-13, max_iter=100,
                  structured=False):
    """Frame-level sibling of multinomial_model for an ORDERED response: one partition (a pandas frame) whose column Y_name holds the
    labels listed in `classes`, lowest first.  `classes` is required: a partition cannot discover the classes it lacks.  There is no
    fit_intercept: the J cutpoints are the intercepts.  Returns the stacked (J + p) x (3 + J + p) frame `par_id, coef, Sig_invMcoef,
    intercept:1 .. intercept:J, <name> ...`; a chunk that lacks an expected dummy level returns the all-zero block with a warning.
    structured=True with a dummy_info and a qualifying design fits on the raw numerics + level codes (fit_ordinal_design; the dense
    one-hot matrix is never built, the missing-level check runs on the codes); the default is the dense path (the design matrix is
    built by the design kernel)."""
    if structured and len(dummy_info) > 0:
        frame, C = _multinomial_codes_frame("ordinal_model", sample_df, Y_name, classes)
        spec, plan, codes, unknown, yd, _, _ = _count_raw_frame(frame, Y_name, False, None, None, dummy_info, dummy_factors_baseline,
                                                                data_info)
        if plan is not None:
            missing = spec.missing_levels(codes)
            if missing or unknown:
                _warn_missing_levels(missing, len(sample_df), spec.names, False, skip=True)
                return _zero_block(ordinal_column_names(spec.names, C))
            mb = fit_ordinal_design(spec.numeric_to_device(frame), torch.from_numpy(codes).cuda(), yd, spec, C, tol=tol, max_iter=max_iter)
            return _first_block_frame(mb, "ordinal_model")
    Xd, names, yd, C = _ordinal_frame("ordinal_model", sample_df, Y_name, classes, dummy_info, dummy_factors_baseline, data_info)
    if Xd is None:
        return _zero_block(ordinal_column_names(names, C))
    mb = fit_ordinal_partitions(Xd, yd, C, names=names, tol=tol, max_iter=max_iter)
    return _first_block_frame(mb, "ordinal_model")


def ordinal_model_eval(sample_df, Y_name, par, classes, dummy_info=[], dummy_factors_baseline=[], data_info=[], structured=False):
    """Log-likelihood (sum log P(y)) of every estimator column of `par` (J + p rows, cutpoints first) on one partition, shaped like
    logistic_model_eval's output: one row, a column per estimator (one pass without the information per column).  structured=True
    with a dummy_info and a qualifying design runs the passes on the raw numerics + level codes."""
    run = None
    if structured and len(dummy_info) > 0:
        frame, C = _multinomial_codes_frame("ordinal_model_eval", sample_df, Y_name, classes)
        spec, plan, codes, unknown, yd, _, _ = _count_raw_frame(frame, Y_name, False, None, None, dummy_info, dummy_factors_baseline,
                                                                data_info)
        if plan is not None:
            missing = spec.missing_levels(codes)
            if missing or unknown:
                _warn_missing_levels(missing, len(sample_df), spec.names, False, skip=False)
            num, cd = spec.numeric_to_device(frame), torch.from_numpy(codes).cuda()

            def run(b):
                return engine.onehot_ordinal_pass(plan, num, cd, yd, b, C, want_H=False)
    if run is None:
        Xd, _, yd, C = _ordinal_frame("ordinal_model_eval", sample_df, Y_name, classes, dummy_info, dummy_factors_baseline, data_info,
                                      for_eval=True)
        X = engine.row_major(Xd)

        def run(b):
            return engine.ordinal_pass(X, yd, b, C, want_H=False)
    return _loglik_frame(par, run)
