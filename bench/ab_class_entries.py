#!/usr/bin/env python3
"""A/B of the eight multinomial / ordinal entries (dense and structured one-hot; pass and fit) across two builds of the library, bit
for bit, in the manner of ab_dispersion_entries.py.  One process, one build:

    python bench/ab_class_entries.py --out FILE.npz          every output array, status, n_iter, return code and refusal text
    python bench/ab_class_entries.py --compare A.npz B.npz   per-array byte comparison; exit status 1 on any mismatch

Run --out once in a checkout of each build, then --compare.  The kernels accumulate in a fixed order, so the bar is equality.
The C ABI is called directly with dlsa_amd.engine's marshalling helpers; outputs are pre-filled, so what an entry leaves unwritten
compares too.  The dense Poisson and NB2 entries ride along (through the wrappers): their row pass shares the skeleton of the
class families' (csrc/row_pass.h); Gamma and Tweedie are ab_dispersion_entries.py's."""
import argparse
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ab_dispersion_entries import main_compare  # noqa: E402

FILL = -7.0
ROWS = (700, 0, 300)          # an empty partition, several row batches per wave, a ragged last batch
N = 2100                      # rows of the shard: partitions of ROWS at row_step 1 (first 0, 700, 700) and 3 (first 0, 1, 2)
WIDTHS = (5, 130)             # one column chunk on the scalar loads, two on the 16-byte ones
CLASSES = (2, 4, 8)
MAX_ITER = 12                 # (a fit that has not converged by then compares all the same)


def main_out(path):
    import torch
    from dlsa_amd import _lib, engine
    lib = _lib.load()
    res = {}
    ptr, stream = engine._ptr, engine._stream

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def new(*shape):
        return torch.full(shape, FILL, dtype=torch.float64, device="cuda")

    def keep(tag, rc, **arrays):
        res[tag + "/rc"] = np.array(rc)
        res[tag + "/error"] = np.array(_lib.last_error() if rc else "")
        for k, v in arrays.items():
            if v is not None:
                res[tag + "/" + k] = v.cpu().numpy() if hasattr(v, "cpu") else np.array(list(v))

    def entry(fam, rows, what):
        return getattr(lib, "dlsa_%s%s_%s" % ("onehot_" if rows[0] == "onehot" else "", fam, what))

    def shape_of(fam, rows):
        """(the arguments that name the rows, the shape arguments next to `classes`, what a structured workspace query starts with, pe)"""
        if rows[0] == "dense":
            X, icpt = rows[1], rows[2] if fam == "multinomial" else 0
            p = X.shape[1]
            return (ptr(X), X.stride(0)), (p, icpt) if fam == "multinomial" else (p,), (), p + icpt
        plan, num, codes = rows[1:4]
        return (plan._h, *engine._oh_args(plan, num, codes)), (), (plan._h,), plan.p

    def coefficients(fam, pe, C):
        return (C - 1) * pe if fam == "multinomial" else C - 1 + pe

    def run_pass(tag, fam, rows, y, theta, C, n, null=None, pad=0, short=0):
        """rows: ("dense", X, icpt) or ("onehot", plan, num, codes)"""
        head, shape, qhead, pe = shape_of(fam, rows)
        d = coefficients(fam, pe, C)
        ld = (n + 31) // 32 * 32
        out = {"H": new(d, d + pad), "g": new(d), "loglik": new(1), "rows": new(C - 1, ld) if fam == "multinomial" else new(n)}
        if null:
            out[null] = None
        need = entry(fam, rows, "workspace_bytes")(*qhead, n, *shape, C, 1)
        ws = engine._workspace(need, y.device)
        tail = (ptr(out["rows"]), ld) if fam == "multinomial" else (ptr(out["rows"]),)
        rc = entry(fam, rows, "pass_f64")(*head, ptr(y), ptr(theta), C, n, *shape, ptr(out["H"]), d + pad, ptr(out["g"]), ptr(out["loglik"]),
                                          *tail, ptr(ws), need - short, stream())
        torch.cuda.synchronize()
        keep(tag, rc, ws_bytes=[need], **out)

    def run_fit(tag, fam, rows, y, C, step, part_rows=ROWS, short=0):
        head, shape, qhead, pe = shape_of(fam, rows)
        first = (0, 1, 2) if step == 3 else tuple(int(v) for v in np.concatenate([[0], np.cumsum(part_rows)[:-1]]))
        K, step, max_rows, c_first, c_rows = engine._strided_partitions(tag, first, part_rows, step, N)
        out = engine._FitOut(K, coefficients(fam, pe, C), y.device)
        for t in (out.coef, out.smc, out.sig):
            t.fill_(FILL)
        need = entry(fam, rows, "workspace_bytes")(*qhead, max_rows, *shape, C, step)
        ws = engine._workspace(need, y.device)
        rc = entry(fam, rows, "fit_f64")(*head, ptr(y), c_first, c_rows, step, K, *shape, C, 1e-13, MAX_ITER, *out.args, ptr(ws), need - short,
                                         stream())
        torch.cuda.synchronize()
        keep(tag, rc, ws_bytes=[need], coef=out.coef, Sig_inv=out.sig, Sig_invMcoef=out.smc, **out.host)

    def theta_of(fam, pe, C):
        if fam == "multinomial":
            return dev(np.linspace(-0.3, 0.4, (C - 1) * pe))
        return dev(np.concatenate([np.linspace(-1.0, 1.2, C - 1), np.linspace(-0.3, 0.4, pe)]))

    def both(tag, fam, rows, y, C, pe, nulls):
        """the fits at both row steps, the pass on the first 700 rows, and (nulls) each nullable output left out in turn"""
        for step in (1, 3):
            run_fit("fit/%s/step%d" % (tag, step), fam, rows, y, C, step)
        front = rows[:1] + tuple(v[:700] if hasattr(v, "stride") else v for v in rows[1:])
        theta = theta_of(fam, pe, C)
        run_pass("pass/%s" % tag, fam, front, y[:700], theta, C, 700)
        run_pass("pass/%s/ldh_pad3" % tag, fam, front, y[:700], theta, C, 700, pad=3)
        for null in nulls:
            run_pass("pass/%s/null_%s" % (tag, null), fam, front, y[:700], theta, C, 700, null=null)

    rng = np.random.default_rng(21)
    y_of = {C: dev(rng.integers(0, C, N).astype(np.float64)) for C in CLASSES}
    X_of = {p: dev(rng.uniform(-0.5, 0.5, (N, p))) for p in WIDTHS}

    # ---- dense ----------------------------------------------------------------------------------------------------------
    for p, C in itertools.product(WIDTHS, CLASSES):
        nulls = ("H", "g", "loglik", "rows") if p == WIDTHS[0] else ()
        for icpt in (0, 1):
            both("multinomial/p%d/C%d/icpt%d" % (p, C, icpt), "multinomial", ("dense", X_of[p], icpt), y_of[C], C, p + icpt, nulls)
        both("ordinal/p%d/C%d" % (p, C), "ordinal", ("dense", X_of[p], 0), y_of[C], C, p, nulls)
        for m, s in itertools.product((0, 1, 7, 700, 100000), (1, 3)):
            res["query/multinomial/p%d/C%d/rows%d/step%d" % (p, C, m, s)] = np.array(lib.dlsa_multinomial_workspace_bytes(m, p, 1, C, s))
            res["query/ordinal/p%d/C%d/rows%d/step%d" % (p, C, m, s)] = np.array(lib.dlsa_ordinal_workspace_bytes(m, p, C, s))

    # ---- structured one-hot: 2 numerics and two factors; a small plan (p = 5) and a wide one (p = 130), each with the constant
    # column (the multinomial family's intercept) and without it (either family) ------------------------------------------------
    plans = {}
    for levels, const in itertools.product(((2, 2), (60, 69)), (True, False)):
        kind, src = ([0] if const else []) + [1, 1], ([0] if const else []) + [0, 1]
        shift, scale = [0.0] * const + [0.2, -0.1], [1.0] * const + [1.5, 0.8]
        d, nlev = len(kind), sum(levels)
        # (with the constant column the first level of each factor is its baseline; without it the first factor keeps all its levels)
        level_col, col = [], d
        for t, nl in enumerate(levels):
            for lv in range(nl):
                drop = lv == 0 and (const or t > 0)
                level_col.append(-1 if drop else col)
                col += 0 if drop else 1
        arr = lambda v, t: np.asarray(v, dtype=t)
        plan = engine.OnehotPlan(col, arr(kind, np.int32), arr(src, np.int32), arr(shift, np.float64), arr(scale, np.float64), list(range(d)),
                                 list(levels), level_col)
        num = dev(rng.normal(size=(N, 2)) * 0.3)
        codes = dev(np.stack([rng.integers(0, nl, N) for nl in levels], 1).astype(np.int32))
        plans[(nlev, const)] = ("onehot", plan, num, codes)
        for C in CLASSES:
            fams = ("multinomial",) if const else ("multinomial", "ordinal")
            for fam in fams:
                tag = "onehot_%s/levels%d/const%d/C%d" % (fam, nlev, const, C)
                both(tag, fam, plans[(nlev, const)], y_of[C], C, plan.p, ("H", "g", "loglik", "rows") if nlev == 4 else ())
                for m, s in itertools.product((0, 1, 255, 256, 257, 700, 100000), (1, 3)):
                    res["query/%s/rows%d/step%d" % (tag, m, s)] = np.array(entry(fam, ("onehot",), "workspace_bytes")(plan._h, m, C, s))

    # ---- refusals and NaNs ----------------------------------------------------------------------------------------------
    C, p = 4, WIDTHS[0]
    ybad = y_of[C].clone()
    ybad[5] = 1.5
    ylack = torch.where((torch.arange(N, device="cuda") >= 700) & (y_of[C] == 2.0), 0.0, y_of[C])      # partition 2 lacks class 2
    for fam, rep in itertools.product(("multinomial", "ordinal"), ("dense", "onehot")):
        rows = ("dense", X_of[p], 1) if rep == "dense" else plans[(4, False)]
        pe = shape_of(fam, rows)[3]
        tag = "refusal/%s/%s" % (rep, fam)
        run_fit(tag + "/bad_class_code", fam, rows, ybad, C, 1)
        run_fit(tag + "/missing_class", fam, rows, ylack, C, 1)
        run_fit(tag + "/ws_short_fit", fam, rows, y_of[C], C, 1, short=1)
        run_pass(tag + "/ws_short_pass", fam, rows, y_of[C], theta_of(fam, pe, C), C, N, short=1)
        run_pass(tag + "/bad_class_code_pass", fam, rows, ybad, theta_of(fam, pe, C), C, N)          # loglik = NaN, nothing refused
        if fam == "ordinal":
            theta = theta_of(fam, pe, C)
            theta[1] = theta[0]                                                                      # two equal cutpoints: loglik = NaN
            run_pass(tag + "/unordered_cutpoints", fam, rows, y_of[C], theta, C, N)

    # ---- the dense count models on the same skeleton --------------------------------------------------------------------
    off = dev(np.log(rng.uniform(0.5, 2.0, N)))
    for p, icpt in itertools.product(WIDTHS, (False, True)):
        X, o = X_of[p], off if icpt else None
        yc = dev(rng.poisson(np.exp(X.cpu().numpy() @ np.linspace(-0.6, 0.6, p) + 0.3)).astype(np.float64))
        beta = dev(np.linspace(-0.3, 0.4, p + icpt))
        first = (0, 700, 700)
        for step, fr in ((1, first), (3, (0, 1, 2))):
            for fam, fit, kw in (("poisson", engine.poisson_fit_ex, {}), ("negbin", engine.negbin_fit_ex, {}),
                                 ("negbin_fixed", engine.negbin_fit_ex, {"alpha": 0.5})):
                r = fit(X, yc, fr, ROWS, row_step=step, offset=o, fit_intercept=icpt, max_iter=MAX_ITER, **kw)
                for k, v in r.items():
                    res["count/%s_fit/p%d/icpt%d/step%d/%s" % (fam, p, icpt, step, k)] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        for fam, outs in (("poisson", engine.poisson_pass(X[:700], yc[:700], beta, offset=None if o is None else o[:700], fit_intercept=icpt,
                                                           want_w=True)),
                          ("negbin", engine.negbin_pass(X[:700], yc[:700], beta, 0.5, offset=None if o is None else o[:700],
                                                        fit_intercept=icpt, want_w=True, want_theta=True))):
            torch.cuda.synchronize()
            for i, v in enumerate(outs):
                res["count/%s_pass/p%d/icpt%d/out%d" % (fam, p, icpt, i)] = v.cpu().numpy()
    np.savez(path, **res)
    print("ab_class_entries: %d arrays of %d entry calls -> %s" % (len(res), sum(k.endswith("/rc") for k in res), path))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(main_compare(*args.compare))
    main_out(args.out)
