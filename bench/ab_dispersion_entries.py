#!/usr/bin/env python3
"""A/B of the eight Gamma / Tweedie entries (dense and structured one-hot; pass and fit) across two builds of the library, bit for
bit.  One process, one build:

    python bench/ab_dispersion_entries.py --out FILE.npz          every output array, status, n_iter, return code and refusal text
    python bench/ab_dispersion_entries.py --compare A.npz B.npz   per-array byte comparison; exit status 1 on any mismatch

Run --out once in a checkout of each build, then --compare.  The kernels accumulate in a fixed order, so the bar is equality.
The C ABI is called with dlsa_amd.engine's own marshalling helpers, directly where the wrappers cannot express a case (a null g or
loglik, a pitch ldh > pe, a workspace one byte short).  Outputs are pre-filled, so what an entry leaves unwritten compares too."""
import argparse
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FILL = -7.0
ROWS = (700, 0, 300)          # an empty partition, more than one 256-row block, a ragged last block
N = 2100                      # rows of the shard: partitions of ROWS at row_step 1 (first 0, 700, 700) and 3 (first 0, 1, 2)
P = 5
POWERS = (1.2, 1.5, 1.9)


def main_out(path):
    import torch
    from dlsa_amd import _lib, engine
    lib = _lib.load()
    res = {}

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

    def scalars(fam, power, dispersion):
        return ((power,) if fam == "tweedie" else ()) + (dispersion,)

    def run_pass(tag, fam, rows, n, pe, dispersion, power, null=None, pad=0, short=0):
        """rows: ("dense", X, icpt) or ("onehot", plan, num, codes); the arguments of the two ABIs differ only in how the rows are named"""
        y, o, beta = rows[-3:]
        H, g, ll, w, st = new(pe, pe + pad), new(pe), new(1), new(n), new(2)
        out = {"H": H, "g": g, "loglik": ll, "w": w, "stats": st}
        if null:
            out[null] = None
        if rows[0] == "dense":
            X, icpt = rows[1:3]
            need = getattr(lib, "dlsa_%s_workspace_bytes" % fam)(n, X.shape[1], icpt, 1)
            head, shape, name = (engine._ptr(X), X.stride(0)), (n, X.shape[1], icpt), "dlsa_%s_pass_f64" % fam
        else:
            plan, num, codes = rows[1:4]
            need = getattr(lib, "dlsa_onehot_%s_workspace_bytes" % fam)(plan._h, n, 1)
            head, shape, name = (plan._h, *engine._oh_args(plan, num, codes)), (n,), "dlsa_onehot_%s_pass_f64" % fam
        ws = engine._workspace(need, y.device)
        rc = getattr(lib, name)(*head, engine._ptr(y), engine._ptr(o), engine._ptr(beta), *scalars(fam, power, dispersion), *shape,
                                engine._ptr(out["H"]), pe + pad, *[engine._ptr(out[k]) for k in ("g", "loglik", "w", "stats")],
                                engine._ptr(ws), need - short, engine._stream())
        torch.cuda.synchronize()
        keep(tag, rc, ws_bytes=[need], **out)

    def run_fit(tag, fam, rows, n, pe, step, dispersion, power, part_rows=ROWS, short=0):
        y, o = rows[-2:]
        first = (0, 1, 2) if step == 3 else tuple(int(v) for v in np.concatenate([[0], np.cumsum(part_rows)[:-1]]))
        K, step, max_rows, c_first, c_rows = engine._strided_partitions(tag, first, part_rows, step, n)
        out = engine._FitOut(K, pe, y.device, engine.GLM_FAMILIES[fam])
        for t in (out.coef, out.smc, out.sig):
            t.fill_(FILL)
        if rows[0] == "dense":
            X, icpt = rows[1:3]
            need = getattr(lib, "dlsa_%s_workspace_bytes" % fam)(max_rows, X.shape[1], icpt, step)
            head, shape, name = (engine._ptr(X), X.stride(0)), (X.shape[1], icpt), "dlsa_%s_fit_f64" % fam
        else:
            plan, num, codes = rows[1:4]
            need = getattr(lib, "dlsa_onehot_%s_workspace_bytes" % fam)(plan._h, max_rows, step)
            head, shape, name = (plan._h, *engine._oh_args(plan, num, codes)), (), "dlsa_onehot_%s_fit_f64" % fam
        ws = engine._workspace(need, y.device)
        rc = getattr(lib, name)(*head, engine._ptr(y), engine._ptr(o), c_first, c_rows, step, K, *shape, *scalars(fam, power, dispersion),
                                1e-13, 100, *out.args, engine._ptr(ws), need - short, engine._stream())
        torch.cuda.synchronize()
        keep(tag, rc, ws_bytes=[need], coef=out.coef, Sig_inv=out.sig, Sig_invMcoef=out.smc, **out.host)

    rng = np.random.default_rng(20)
    X = rng.uniform(-0.5, 0.5, (N, P))
    off = np.log(rng.uniform(0.5, 2.0, N))
    mu = np.exp(X @ np.linspace(-0.6, 0.6, P) + 0.3)
    y_of = {"gamma": rng.gamma(2.0, mu / 2.0), "tweedie": np.where(rng.random(N) < 0.4, 0.0, rng.gamma(2.0, mu))}
    fams = [("gamma", None)] + [("tweedie", xi) for xi in POWERS]
    Xd, offd = dev(X), dev(off)

    # ---- dense ----------------------------------------------------------------------------------------------------------
    for (fam, xi), icpt, o in itertools.product(fams, (0, 1), (None, offd)):
        tag = "%s%s/icpt%d/off%d" % (fam, "" if xi is None else xi, icpt, o is not None)
        yd, pe = dev(y_of[fam]), P + icpt
        for step, disp in itertools.product((1, 3), (0.0, 0.7)):
            run_fit("fit/%s/step%d/disp%s" % (tag, step, disp), fam, ("dense", Xd, icpt, yd, o), N, pe, step, disp, xi)
        beta = dev(np.linspace(-0.3, 0.4, pe))
        rows = ("dense", Xd[:700], icpt, yd[:700], None if o is None else o[:700], beta)
        for disp in (1.0, 2.5):
            run_pass("pass/%s/disp%s" % (tag, disp), fam, rows, 700, pe, disp, xi)
        for null in ("H", "g", "loglik", "stats"):
            run_pass("pass/%s/null_%s" % (tag, null), fam, rows, 700, pe, 2.5, xi, null=null)
        run_pass("pass/%s/ldh_pad3" % tag, fam, rows, 700, pe, 2.5, xi, pad=3)

    # ---- structured one-hot: 2 numerics, factors of 3 and 4 levels, with and without the constant column -----------------------
    plans = {}
    for const in (True, False):
        kind, src, shift, scale = ([0] if const else []) + [1, 1], ([0] if const else []) + [0, 1], [0.0] * const + [0.2, -0.1], [1.0] * const + [1.5, 0.8]
        d = len(kind)
        # (without the constant column the first factor keeps all its levels: the design stays of full rank)
        level_col = [-1 if const else d + 5, d, d + 1, -1, d + 2, d + 3, d + 4]
        p = d + (5 if const else 6)
        arr = lambda v, t: np.asarray(v, dtype=t)
        plan = engine.OnehotPlan(p, arr(kind, np.int32), arr(src, np.int32), arr(shift, np.float64), arr(scale, np.float64), list(range(d)),
                                 [3, 4], level_col)
        plans[const] = (plan, p)
        for fam, m, s in itertools.product(("gamma", "tweedie"), (0, 1, 255, 256, 257, 700, 100000), (1, 3)):
            res["query/onehot_%s/const%d/rows%d/step%d" % (fam, const, m, s)] = np.array(
                getattr(lib, "dlsa_onehot_%s_workspace_bytes" % fam)(plan._h, m, s))
    num = rng.normal(size=(N, 2)) * 0.3
    codes = np.stack([rng.integers(0, 3, N), rng.integers(0, 4, N)], 1).astype(np.int32)
    numd, codesd = dev(num), dev(codes)
    for (fam, xi), const, o in itertools.product(fams, (True, False), (None, offd)):
        plan, p = plans[const]
        tag = "onehot_%s%s/const%d/off%d" % (fam, "" if xi is None else xi, const, o is not None)
        yd = dev(y_of[fam])
        for step, disp in itertools.product((1, 3), (0.0, 0.7)):
            run_fit("fit/%s/step%d/disp%s" % (tag, step, disp), fam, ("onehot", plan, numd, codesd, yd, o), N, p, step, disp, xi)
        beta = dev(np.linspace(-0.3, 0.4, p))
        rows = ("onehot", plan, numd[:700], codesd[:700], yd[:700], None if o is None else o[:700], beta)
        for disp in (1.0, 2.5):
            run_pass("pass/%s/disp%s" % (tag, disp), fam, rows, 700, p, disp, xi)
        for null in ("H", "g", "loglik", "stats"):
            run_pass("pass/%s/null_%s" % (tag, null), fam, rows, 700, p, 2.5, xi, null=null)
        run_pass("pass/%s/ldh_pad3" % tag, fam, rows, 700, p, 2.5, xi, pad=3)

    # ---- refusals (dense with the intercept, structured with the constant column) -------------------------------------------
    plan, p = plans[True]
    for fam, xi in (("gamma", None), ("tweedie", 1.5)):
        y = y_of[fam].copy()
        bad = {"few_rows": (y, (700, 4, 300)), "all_zero_or_y0": (np.where(np.arange(N) >= 700, 0.0, y), (700, 300))}
        ybad = y.copy()
        ybad[5] = 0.0 if fam == "gamma" else -1.0
        bad["bad_row"] = (ybad, ROWS)
        for (what, (yy, part_rows)), rep in itertools.product(bad.items(), ("dense", "onehot")):
            rows = ("dense", Xd, 1, dev(yy), offd) if rep == "dense" else ("onehot", plan, numd, codesd, dev(yy), offd)
            run_fit("refusal/%s/%s/%s" % (rep, fam, what), fam, rows, N, P + 1 if rep == "dense" else p, 1, 0.0, xi, part_rows=part_rows)
        yd = dev(y)
        for rep in ("dense", "onehot"):
            pe = P + 1 if rep == "dense" else p
            rows = ("dense", Xd, 1) if rep == "dense" else ("onehot", plan, numd, codesd)
            run_fit("refusal/%s/%s/ws_short_fit" % (rep, fam), fam, rows + (yd, offd), N, pe, 1, 0.0, xi, short=1)
            run_pass("refusal/%s/%s/ws_short_pass" % (rep, fam), fam, rows + (yd, offd, dev(np.zeros(pe))), N, pe, 1.0, xi, short=1)
    np.savez(path, **res)
    print("ab_dispersion_entries: %d arrays of %d entry calls -> %s" % (len(res), sum(k.endswith("/rc") for k in res), path))


def main_compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    keys = sorted(set(a.files) | set(b.files))
    bad = [k for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
           or a[k].tobytes() != b[k].tobytes()]
    calls = [k for k in keys if k.endswith("/rc")]
    refused = [k for k in calls if k in a.files and int(a[k]) != 0]
    print("cases (entry calls) %d, of them with a non-zero return code %d; workspace queries %d; arrays compared %d; mismatches = %d" % (
        len(calls), len(refused), sum(k.startswith("query/") for k in keys), len(keys), len(bad)))
    for k in bad:
        print("MISMATCH", k)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(main_compare(*args.compare))
    main_out(args.out)
