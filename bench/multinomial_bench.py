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
Run under rocprofv3 --kernel-trace --stats for the per-kernel split (weight kernel / Grams / border passes).
With --structured (a leg of its own) the structured one-hot path (csrc/onehot_multinomial.hip) on bench/surrogates.airline_shaped
rows (7 numerics, 5 factors, p = 260 with the intercept):
  oh_pass / oh_pass_prob  the structured multinomial pass (g, loglik; and with P stored) next to the unchanged structured Poisson pass
            (g, loglik; and with its weights stored) on the same rows, with the byte-derived floor of the ratio,
            (8q + 4f + 8 + 8 J [P stored]) / (8q + 4f + 8 + 8 [w stored]);
  oh_eval   one structured evaluation (pass + J (J + 1) / 2 weight kernels and structured Grams + the mirror) next to the dense
            multinomial evaluation on the matrix the design kernel builds from the same rows (its constant column a column);
  oh_fit    the structured fit of 1e6-row partitions next to the dense fit of the same partitions on the built matrix.
--structured --fit-only runs one structured fit per class count (the run to put under rocprofv3)."""
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


def airline_multinomial(n, C, dense=True):
    """surrogates.airline_shaped's rows with a C-class response drawn from the structured representation at B = 0.15 N(0, 1)
    (d["cls"], d["B"] [J, p]) and a Poisson response at d["beta"] for the yardstick (d["cnt"])"""
    import surrogates                            # bench/surrogates.py: test / bench data, not product code
    d = surrogates.airline_shaped(n, dense=dense)
    num, codes, levels, p = d["num"], d["codes"], d["levels"], d["p"]
    q = num.shape[1]
    g = torch.Generator(device="cuda").manual_seed(13)
    B = torch.randn((C - 1, p), dtype=torch.float64, device="cuda", generator=g) * 0.15

    def linear(b):
        eta = b[0] + ((num - 1.5) / 3.0) @ b[1:1 + q]
        pos = 1 + q
        for fi, L in enumerate(levels):
            tab = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), b[pos:pos + L - 1]])
            eta = eta + tab[codes[:, fi].long()]
            pos += L - 1
        return eta
    eta = torch.stack([torch.zeros(n, dtype=torch.float64, device="cuda")] + [linear(B[j]) for j in range(C - 1)], 1)
    cdf = torch.cumsum(torch.softmax(eta, 1), 1)
    u = torch.rand((n, 1), dtype=torch.float64, device="cuda", generator=g)
    d["cls"] = (u > cdf).sum(1).clamp_max(C - 1).to(torch.float64)
    d["cnt"] = torch.poisson(torch.exp(linear(d["beta"])), generator=g)
    d["B"] = B
    return d


def oh_pass_case(n, C, reps, prob):
    d = airline_multinomial(n, C, dense=False)
    plan, num, codes, y, yp = d["plan"], d["num"], d["codes"], d["cls"], d["cnt"]
    theta, beta = (0.5 * d["B"]).reshape(-1).contiguous(), (0.5 * d["beta"]).contiguous()
    tm, tp = alternating(lambda: engine.onehot_multinomial_pass(plan, num, codes, y, theta, C, want_H=False, want_prob=prob),
                         lambda: engine.onehot_poisson_pass(plan, num, codes, yp, beta, want_H=False, want_w=prob), reps)
    row = 8.0 * num.shape[1] + 4.0 * codes.shape[1] + 8.0
    J = C - 1
    return {"case": "oh_pass_prob" if prob else "oh_pass", "n": n, "p": d["p"], "classes": C, **sides("multinomial", tm, "poisson", tp),
            "byte_floor_ratio": round((row + (8 * J if prob else 0)) / (row + (8 if prob else 0)), 4),
            "multinomial_TBps": round(n * row / (tm[0] * 1e-3) / 1e12, 3), "poisson_TBps": round(n * row / (tp[0] * 1e-3) / 1e12, 3)}


def oh_eval_case(n, C, reps):
    d = airline_multinomial(n, C)
    plan, num, codes, y, X = d["plan"], d["num"], d["codes"], d["cls"], d["X"]
    theta = (0.5 * d["B"]).reshape(-1).contiguous()
    ts, td = alternating(lambda: engine.onehot_multinomial_pass(plan, num, codes, y, theta, C),
                         lambda: engine.multinomial_pass(X, y, theta, C), reps)
    J = C - 1
    return {"case": "oh_eval", "n": n, "p": d["p"], "classes": C, "grams": J * (J + 1) // 2, "dimension": J * d["p"],
            **sides("structured_eval", ts, "dense_eval", td)}


def oh_fit_case(n, K, C, reps, dense=True):
    d = airline_multinomial(n, C, dense=dense)
    plan, num, codes, y = d["plan"], d["num"], d["codes"], d["cls"]
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    last = {}

    def structured():
        last["s"] = engine.onehot_multinomial_fit_ex(plan, num, codes, y, first, rows, row_step=K, classes=C)

    def dense_fit():
        last["d"] = engine.multinomial_fit_ex(d["X"], y, first, rows, row_step=K, classes=C)
    if not dense:
        ts = sorted(timed(structured, reps) for _ in range(3))
        rs = last["s"]
        return {"case": "oh_fit_only", "n": n, "p": d["p"], "classes": C, "partitions": K, "fit_ms": round(ts[1], 3),
                "evaluations": rs["n_iter"][:4], "status_ok": all(s == 0 for s in rs["status"])}
    ts, td = alternating(structured, dense_fit, reps, rounds=3)
    rs, rd = last["s"], last["d"]
    per = (ts[0] / sum(rs["n_iter"])) / (td[0] / sum(rd["n_iter"]))
    return {"case": "oh_fit", "n": n, "p": d["p"], "classes": C, "partitions": K, **sides("structured_fit", ts, "dense_fit", td),
            "structured_evaluations": rs["n_iter"][:4], "dense_evaluations": rd["n_iter"][:4], "ratio_per_evaluation": round(per, 3),
            "structured_ms_per_evaluation": round(ts[0] / sum(rs["n_iter"]), 3),
            "status_ok": all(s == 0 for s in rs["status"]) and all(s == 0 for s in rd["status"])}


def structured_main(a):
    n = 1_000_000
    for C in a.classes:
        if a.fit_only:
            print(json.dumps(oh_fit_case(n, 1, C, 1, dense=False)), flush=True)
            continue
        for fn in (lambda: oh_pass_case(n, C, a.reps * 4, False), lambda: oh_pass_case(n, C, a.reps * 4, True),
                   lambda: oh_eval_case(n, C, max(1, a.reps // 2)), lambda: oh_fit_case(n, 1, C, 1)):
            print(json.dumps(fn()), flush=True)
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, nargs="*", default=[3, 8])
    ap.add_argument("--small", action="store_true", help="1e6 x 100 only (a quick check)")
    ap.add_argument("--fit-only", action="store_true", help="one fit of the first shape per class count (the run to put under rocprofv3)")
    ap.add_argument("--structured", action="store_true", help="the structured one-hot leg only (airline-shaped rows, C = 3 and C = 8)")
    a = ap.parse_args()
    if a.structured:
        return structured_main(a)
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
