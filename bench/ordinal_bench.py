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
Shapes: 1e6 x {50, 130, 500}; --classes C (default 4)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--small", action="store_true", help="1e6 x 50 only (a quick check)")
    a = ap.parse_args()
    C = a.classes
    shapes = [(1_000_000, 50)] if a.small else [(1_000_000, 50), (1_000_000, 130), (1_000_000, 500)]
    for n, p in shapes:
        for fn in (lambda: pass_case(n, p, C, a.reps), lambda: pass_mn3_case(n, p, C, a.reps), lambda: eval_case(n, p, C, max(1, a.reps // 2))):
            print(json.dumps(fn()), flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(fit_case(shapes[0][0], shapes[0][1], C, 1)), flush=True)


if __name__ == "__main__":
    main()
