"""Timing of the ordinal (proportional-odds) map step (csrc/ordinal.hip) next to the unchanged Poisson pass on the same rows, the
sibling of bench/multinomial_bench.py.  Every pair is timed alternating in one call, five rounds of `reps` calls each; each side
reports its median and its run-to-run spread (fastest .. slowest of the rounds).  Prints one JSON line per case:
  pass      the ordinal pass alone (g, loglik; no H, no w) next to engine.poisson_pass (g, loglik; no H, no w) on the same rows, with
            the algorithmic bandwidth of one read of the rows (8 p + 8 bytes per row): one read of X and one dot product per row on
            either side, so the ratio should track 1;
  pass_mn3  the multinomial pass with C = 3 (two dot products per row) next to the same Poisson pass: the ratio the ordinal one is
            held against;
  eval      one ordinal evaluation with H (pass with the in-pass borders, or the masked X'v route where C NC > 16, + ONE Gram +
            the assembly) next to the Poisson evaluation with H on the same rows (its pass + one Gram): hessian_ms = eval - pass;
  fit       a whole fit of the first shape (one partition): time, evaluations, time per evaluation.
Shapes: 1e6 x {50, 130, 500}; --classes C (default 4).
With --structured (a leg of its own) the structured one-hot path (csrc/onehot_ordinal.hip) on bench/surrogates.airline_shaped rows
without their constant column (7 numerics, 5 factors, p = 259; the cutpoints are the intercepts), at C = 4 and C = 8:
  oh_pass   the structured ordinal pass (g, loglik) next to the unchanged structured Poisson pass (g, loglik) on the same rows
            (its plan keeps the constant column), with the byte floor n (8q + 4f + 8) of either;
  oh_eval   one structured evaluation with H (pass + ONE structured Gram + the assembly) next to the dense ordinal evaluation on
            the matrix the design kernel builds from the same rows, and next to the structured multinomial evaluation at the same C;
  oh_fit    the structured fit of one 1e6-row partition: time, evaluations, time per evaluation;
  oh_masked (--masked) one evaluation on the masked border route: 1e6 rows, one 500-level factor + 1 numeric, C = 8."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlsa_amd  # noqa: E402
from dlsa_amd import engine  # noqa: E402
from gamma_bench import alternating, sides, timed  # noqa: E402


def data(n, p, C, seed=321):
    """simulate_ordinal's model on engine.synth rows, drawn on the device: class codes y, a Poisson response of the same linear
    predictor for the yardstick, a 3-class response for the multinomial yardstick, and theta* = [alpha | beta]"""
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: int(0.4 * p)] = 0.5
    share = torch.arange(1, C, dtype=torch.float64, device="cuda") / C
    alpha = torch.log(share / (1.0 - share))
    g = torch.Generator(device="cuda").manual_seed(9)
    eta = X @ beta
    u = torch.rand(n, dtype=torch.float64, device="cuda", generator=g).clamp_(1e-300, 1.0 - 1e-16)
    latent = eta + torch.log(u / (1.0 - u))
    y = (latent[:, None] > alpha[None, :]).sum(1).to(torch.float64)
    yp = torch.poisson(torch.exp(eta), generator=g)
    y3 = torch.randint(0, 3, (n,), device="cuda", generator=g).to(torch.float64)
    return X, y, yp, y3, torch.cat([alpha, beta])


def pass_case(n, p, C, reps):
    X, y, yp, _, theta = data(n, p, C)
    th, beta = (0.5 * theta).contiguous(), (0.5 * theta[C - 1:]).contiguous()
    to, tp = alternating(lambda: engine.ordinal_pass(X, y, th, C, want_H=False), lambda: engine.poisson_pass(X, yp, beta, want_H=False), reps)
    gb = n * (8.0 * p + 8.0)
    return {"case": "pass", "n": n, "p": p, "classes": C, **sides("ordinal", to, "poisson", tp),
            "ordinal_TBps": round(gb / (to[0] * 1e-3) / 1e12, 3), "poisson_TBps": round(gb / (tp[0] * 1e-3) / 1e12, 3)}


def pass_mn3_case(n, p, C, reps):
    X, _, yp, y3, theta = data(n, p, C)
    beta = (0.5 * theta[C - 1:]).contiguous()
    th3 = torch.cat([beta, -beta]).contiguous()
    tm, tp = alternating(lambda: engine.multinomial_pass(X, y3, th3, 3, want_H=False), lambda: engine.poisson_pass(X, yp, beta, want_H=False), reps)
    return {"case": "pass_mn3", "n": n, "p": p, **sides("multinomial3", tm, "poisson", tp)}


def eval_case(n, p, C, reps):
    X, y, yp, _, theta = data(n, p, C)
    th, beta = (0.5 * theta).contiguous(), (0.5 * theta[C - 1:]).contiguous()
    te, tq = alternating(lambda: engine.ordinal_pass(X, y, th, C), lambda: engine.poisson_pass(X, yp, beta), reps)
    t0 = sorted(timed(lambda: engine.ordinal_pass(X, y, th, C, want_H=False), reps) for _ in range(5))[2]
    nc = 1
    while nc * 128 < p:
        nc *= 2
    return {"case": "eval", "n": n, "p": p, "classes": C, "borders": "in the pass" if C * nc <= 16 else "masked X'v per cutpoint",
            **sides("ordinal_eval", te, "poisson_eval", tq), "hessian_ms": round(te[0] - t0, 4), "dimension": C - 1 + p}


def fit_case(n, p, C, reps):
    X, y, _, _, _ = data(n, p, C)
    last = {}

    def fit():
        last["m"] = dlsa_amd.fit_ordinal_partitions(X, y, C)
    ts = sorted(timed(fit, reps) for _ in range(3))
    mb = last["m"]
    return {"case": "fit", "n": n, "p": p, "classes": C, "fit_ms": round(ts[1], 3), "fit_spread_ms": [round(ts[0], 3), round(ts[-1], 3)],
            "evaluations": mb.n_iter, "ms_per_evaluation": round(ts[1] / mb.n_iter[0], 3), "status_ok": mb.status == [0]}


def airline_ordinal(n, C, dense):
    """surrogates.airline_shaped's rows with a C-class ordered response drawn from the structured representation at the surrogate's
    beta and equal-share cutpoints: d["cls"], d["theta"] = [alpha | beta without the constant], d["plan0"] the plan WITHOUT the
    constant column (p = 259), d["X0"] (dense=True) the built matrix without it, d["cnt"] a Poisson response for the yardstick."""
    import surrogates                            # bench/surrogates.py: test / bench data, not product code
    d = surrogates.airline_shaped(n, dense=dense)
    num, codes, levels, p = d["num"], d["codes"], d["levels"], d["p"]
    q = num.shape[1]
    b = d["beta"]
    eta = ((num - 1.5) / 3.0) @ b[1:1 + q]
    pos = 1 + q
    level_col = []
    for fi, L in enumerate(levels):
        tab = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), b[pos:pos + L - 1]])
        eta = eta + tab[codes[:, fi].long()]
        level_col += [-1] + list(range(pos - 1, pos - 1 + L - 1))
        pos += L - 1
    g = torch.Generator(device="cuda").manual_seed(13)
    share = torch.arange(1, C, dtype=torch.float64, device="cuda") / C
    alpha = torch.log(share / (1.0 - share))
    u = torch.rand(n, dtype=torch.float64, device="cuda", generator=g).clamp_(1e-300, 1.0 - 1e-16)
    d["cls"] = ((eta + torch.log(u / (1.0 - u)))[:, None] > alpha[None, :]).sum(1).to(torch.float64)
    d["cnt"] = torch.poisson(torch.exp(b[0] + eta), generator=g)
    d["theta"] = torch.cat([alpha, b[1:]]).contiguous()
    d["plan0"] = engine.OnehotPlan(p - 1, [1] * q, list(range(q)), [1.5] * q, [3.0] * q, list(range(q)), list(levels), level_col)
    if dense:
        d["X0"] = d["X"][:, 1:].contiguous()
    return d


def oh_pass_case(n, C, reps):
    d = airline_ordinal(n, C, dense=False)
    num, codes = d["num"], d["codes"]
    th, beta = (0.5 * d["theta"]).contiguous(), (0.5 * d["beta"]).contiguous()
    to, tp = alternating(lambda: engine.onehot_ordinal_pass(d["plan0"], num, codes, d["cls"], th, C, want_H=False),
                         lambda: engine.onehot_poisson_pass(d["plan"], num, codes, d["cnt"], beta, want_H=False), reps)
    floor = n * (8.0 * num.shape[1] + 4.0 * codes.shape[1] + 8.0)
    return {"case": "oh_pass", "n": n, "p": d["p"] - 1, "classes": C, **sides("ordinal", to, "poisson", tp), "floor_bytes": int(floor),
            "ordinal_TBps": round(floor / (to[0] * 1e-3) / 1e12, 3), "poisson_TBps": round(floor / (tp[0] * 1e-3) / 1e12, 3)}


def oh_eval_case(n, C, reps):
    d = airline_ordinal(n, C, dense=True)
    num, codes, y = d["num"], d["codes"], d["cls"]
    th = (0.5 * d["theta"]).contiguous()
    J, p = C - 1, d["p"]
    g = torch.Generator(device="cuda").manual_seed(14)
    thm = (torch.randn(J * p, dtype=torch.float64, device="cuda", generator=g) * 0.15).contiguous()
    ts, td = alternating(lambda: engine.onehot_ordinal_pass(d["plan0"], num, codes, y, th, C), lambda: engine.ordinal_pass(d["X0"], y, th, C), reps)
    tm = sorted(timed(lambda: engine.onehot_multinomial_pass(d["plan"], num, codes, y, thm, C), reps) for _ in range(5))
    t0 = sorted(timed(lambda: engine.onehot_ordinal_pass(d["plan0"], num, codes, y, th, C, want_H=False), reps) for _ in range(5))[2]
    return {"case": "oh_eval", "n": n, "p": p - 1, "classes": C, "dimension": J + p - 1, **sides("structured_eval", ts, "dense_eval", td),
            "multinomial_eval_ms": round(tm[2], 4), "multinomial_eval_spread_ms": [round(tm[0], 4), round(tm[-1], 4)],
            "ratio_to_multinomial": round(ts[0] / tm[2], 3), "multinomial_dimension": J * p, "hessian_ms": round(ts[0] - t0, 4)}


def oh_fit_case(n, C):
    d = airline_ordinal(n, C, dense=False)
    last = {}

    def fit():
        last["r"] = engine.onehot_ordinal_fit_ex(d["plan0"], d["num"], d["codes"], d["cls"], [0], [n], classes=C)
    ts = sorted(timed(fit, 1) for _ in range(3))
    r = last["r"]
    return {"case": "oh_fit", "n": n, "p": d["p"] - 1, "classes": C, "fit_ms": round(ts[1], 3), "fit_spread_ms": [round(ts[0], 3), round(ts[-1], 3)],
            "evaluations": r["n_iter"], "ms_per_evaluation": round(ts[1] / max(1, r["n_iter"][0]), 3), "status_ok": r["status"] == [0]}


def oh_masked_case(n, C, reps):
    """the masked border route: one numeric + one 500-level factor with uniform levels, baseline dropped (p = 500): C = 8 leaves the
    32 KiB budget, the J border vectors take one structured X'v each"""
    L = 500
    g = torch.Generator(device="cuda").manual_seed(15)
    num = torch.randn((n, 1), dtype=torch.float64, device="cuda", generator=g)
    codes = torch.randint(0, L, (n, 1), device="cuda", generator=g).int()
    plan = engine.OnehotPlan(L, [1], [0], [0.0], [1.0], [0], [L], [-1] + list(range(1, L)))
    beta = torch.randn(L, dtype=torch.float64, device="cuda", generator=g) * 0.15
    share = torch.arange(1, C, dtype=torch.float64, device="cuda") / C
    th = torch.cat([torch.log(share / (1.0 - share)), beta]).contiguous()
    y = torch.randint(0, C, (n,), device="cuda", generator=g).to(torch.float64)
    te = sorted(timed(lambda: engine.onehot_ordinal_pass(plan, num, codes, y, th, C), reps) for _ in range(5))
    t0 = sorted(timed(lambda: engine.onehot_ordinal_pass(plan, num, codes, y, th, C, want_H=False), reps) for _ in range(5))
    return {"case": "oh_masked", "n": n, "p": L, "classes": C, "eval_ms": round(te[2], 4), "eval_spread_ms": [round(te[0], 4), round(te[-1], 4)],
            "pass_ms": round(t0[2], 4)}


def structured_main(a):
    n = 1_000_000
    if a.masked:
        print(json.dumps(oh_masked_case(n, 8, max(1, a.reps // 2))), flush=True)
        return
    for C in (4, 8):
        for fn in (lambda: oh_pass_case(n, C, a.reps * 4), lambda: oh_eval_case(n, C, max(1, a.reps // 2)), lambda: oh_fit_case(n, C)):
            print(json.dumps(fn()), flush=True)
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--small", action="store_true", help="1e6 x 50 only (a quick check)")
    ap.add_argument("--structured", action="store_true", help="the structured one-hot leg only (airline-shaped rows, C = 4 and C = 8)")
    ap.add_argument("--masked", action="store_true", help="with --structured: the masked border route only (p = 500, C = 8)")
    a = ap.parse_args()
    if a.structured:
        return structured_main(a)
    C = a.classes
    shapes = [(1_000_000, 50)] if a.small else [(1_000_000, 50), (1_000_000, 130), (1_000_000, 500)]
    for n, p in shapes:
        for fn in (lambda: pass_case(n, p, C, a.reps), lambda: pass_mn3_case(n, p, C, a.reps), lambda: eval_case(n, p, C, max(1, a.reps // 2))):
            print(json.dumps(fn()), flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(fit_case(shapes[0][0], shapes[0][1], C, 1)), flush=True)


if __name__ == "__main__":
    main()
