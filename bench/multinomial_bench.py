"""Timing of the multinomial logistic map step (csrc/multinomial.hip) next to the unchanged Poisson pass on the same rows.  Every
pair is timed alternating in one call, five rounds of `reps` calls each; each side reports its median and its run-to-run spread
(fastest .. slowest of the rounds).  Prints one JSON line per case:
  pass      the multinomial pass alone (g, loglik; no H, no P) next to engine.poisson_pass (g, loglik; no H, no w) on the same rows,
            with the algorithmic bandwidth of one read of the rows (8 p + 8 bytes per row) and the byte-derived floor of the ratio,
            (8 p + 8 + 8 J [P stored]) / (8 p + 8) -- 1.0 here, since P is not stored;
  pass_prob the same with P stored (what an evaluation with H runs) next to the Poisson pass that stores its weights;
  eval      one evaluation with H (pass + J (J + 1) / 2 weight kernels, Grams and border passes + the mirror), and the Cholesky solve of
            the (J pe)^2 system on its own: hessian_ms = eval_ms - the pass with P;
  fit       a whole fit of the first shape with an intercept (one partition): time, evaluations, time per evaluation.
Run under rocprofv3 --kernel-trace --stats for the per-kernel split (weight kernel / Grams / border passes)."""
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
    """simulate_multinomial's model on engine.synth rows, drawn on the device: class codes y, a Poisson response of a comparable
    linear predictor for the yardstick, and theta* (class-major, no intercept)"""
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    B = torch.zeros((C - 1, p), dtype=torch.float64, device="cuda")
    for j in range(1, C):
        B[j - 1, : int(0.4 * p)] = 0.5 if j % 2 else -0.5
    g = torch.Generator(device="cuda").manual_seed(9)
    eta = torch.cat([torch.zeros((n, 1), dtype=torch.float64, device="cuda"), X @ B.t()], 1)
    cdf = torch.cumsum(torch.softmax(eta, 1), 1)
    u = torch.rand((n, 1), dtype=torch.float64, device="cuda", generator=g)
    y = (u > cdf).sum(1).clamp_max(C - 1).to(torch.float64)
    yp = torch.poisson(torch.exp(eta[:, 1]), generator=g)
    return X, y, yp, B


def pass_case(n, p, C, reps, prob):
    X, y, yp, B = data(n, p, C)
    theta, beta = (0.5 * B).reshape(-1).contiguous(), (0.5 * B[0]).contiguous()
    tm, tp = alternating(lambda: engine.multinomial_pass(X, y, theta, C, want_H=False, want_prob=prob),
                         lambda: engine.poisson_pass(X, yp, beta, want_H=False, want_w=prob), reps)
    gb = n * (8.0 * p + 8.0)
    J = C - 1
    return {"case": "pass_prob" if prob else "pass", "n": n, "p": p, "classes": C, **sides("multinomial", tm, "poisson", tp),
            "byte_floor_ratio": round((8.0 * p + 8 + (8 * J if prob else 0)) / (8.0 * p + 8 + (8 if prob else 0)), 4),
            "multinomial_TBps": round(gb / (tm[0] * 1e-3) / 1e12, 3), "poisson_TBps": round(gb / (tp[0] * 1e-3) / 1e12, 3)}


def eval_case(n, p, C, reps):
    X, y, _, B = data(n, p, C)
    theta = (0.5 * B).reshape(-1).contiguous()
    H, g = engine.multinomial_pass(X, y, theta, C)[:2]
    te, tq = alternating(lambda: engine.multinomial_pass(X, y, theta, C), lambda: engine.multinomial_pass(X, y, theta, C, want_H=False, want_prob=True), reps)
    ts = sorted(timed(lambda: engine.spd_solve(H, g), reps * 4) for _ in range(5))
    J = C - 1
    return {"case": "eval", "n": n, "p": p, "classes": C, "grams": J * (J + 1) // 2, **sides("eval", te, "pass_with_P", tq),
            "hessian_ms": round(te[0] - tq[0], 4), "solve_ms": round(ts[2], 4), "dimension": J * p}


def fit_case(n, p, C, reps):
    X, y, _, _ = data(n, p, C)
    last = {}

    def fit():
        last["m"] = dlsa_amd.fit_multinomial_partitions(X, y, C, fit_intercept=True)
    ts = sorted(timed(fit, reps) for _ in range(3))
    mb = last["m"]
    return {"case": "fit", "n": n, "p": p, "classes": C, "fit_ms": round(ts[1], 3), "fit_spread_ms": [round(ts[0], 3), round(ts[-1], 3)],
            "evaluations": mb.n_iter, "ms_per_evaluation": round(ts[1] / mb.n_iter[0], 3), "status_ok": mb.status == [0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, nargs="*", default=[3, 8])
    ap.add_argument("--small", action="store_true", help="1e6 x 100 only (a quick check)")
    ap.add_argument("--fit-only", action="store_true", help="one fit of the first shape per class count (the run to put under rocprofv3)")
    a = ap.parse_args()
    shapes = [(1_000_000, 100)] if a.small else [(10_000_000, 100), (2_000_000, 500)]
    if a.fit_only:
        for C in a.classes:
            print(json.dumps(fit_case(shapes[0][0], shapes[0][1], C, 1)), flush=True)
        return
    for C in a.classes:
        for n, p in shapes:
            if (C - 1) * (p + 1) > 2048:
                print(json.dumps({"case": "skipped", "n": n, "p": p, "classes": C, "why": "(classes - 1) * (p + 1) > 2048"}), flush=True)
                continue
            for fn in (lambda: pass_case(n, p, C, a.reps, False), lambda: pass_case(n, p, C, a.reps, True),
                       lambda: eval_case(n, p, C, max(1, a.reps // 2))):
                print(json.dumps(fn()), flush=True)
                torch.cuda.empty_cache()
        print(json.dumps(fit_case(shapes[0][0], shapes[0][1], C, 1)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
