"""Timing of the Gamma map step (csrc/gamma.hip) next to the Poisson one on the same rows.  Every pair is timed alternating in one
call, `rounds` rounds of `reps` calls each; each side reports its median and its run-to-run spread (min .. max of the rounds).
Prints one JSON line per case:
  pass      the Gamma pass alone (r, g, loglik) next to engine.poisson_pass on the same rows, with the algorithmic bandwidth of one
            read of the rows (8 p bytes per row);
  iter      one Newton evaluation + solve (dlsa_gamma_pass_f64 with H + the Cholesky solve) next to the Poisson one;
  fit       a whole fit of 1e7 x 100 with an intercept and offsets (one partition, estimated dispersion) next to the Poisson fit.
With --structured (a leg of its own) the structured one-hot path (csrc/onehot_gamma.hip) on bench/surrogates.airline_shaped rows
with Gamma responses (shape 2, exposure ~ U(0.5, 2)):
  oh_pass   the structured Gamma pass next to the structured Poisson pass (bytes per row 8q + 4f + 32 against 8q + 4f + 24);
  oh_newton a structured Newton evaluation (pass + H) next to the Poisson one -- the same ordered Gram on both sides;
  oh_fit    the structured fit of 1e6-row partitions next to the dense Gamma fit of the same partitions (matrix built once), with
            the peak device memory of both.
Run under rocprofv3 --kernel-trace --stats for the per-kernel split."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlsa_amd  # noqa: E402
from dlsa_amd import engine  # noqa: E402
from poisson_bench import airline_poisson, timed  # noqa: E402


def alternating(fa, fb, reps, rounds=5):
    """fa and fb timed in turns in the same call: ((median, min, max) ms of fa, the same of fb) over `rounds` rounds of `reps` calls"""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    ta.sort(); tb.sort()
    return (ta[len(ta) // 2], ta[0], ta[-1]), (tb[len(tb) // 2], tb[0], tb[-1])


def sides(name_a, a, name_b, b):
    out = {}
    for name, (med, lo, hi) in ((name_a, a), (name_b, b)):
        out.update({name + "_ms": round(med, 4), name + "_spread_ms": [round(lo, 4), round(hi, 4)]})
    out["ratio"] = round(a[0] / b[0], 3)
    return out


def gamma2(mu, g):
    """y ~ Gamma(shape 2, mean mu): mu / 2 times the sum of two unit exponentials"""
    u = torch.rand((2, mu.numel()), dtype=torch.float64, device=mu.device, generator=g).clamp_min_(1e-300)
    return mu * (-0.5) * torch.log(u).sum(0)


def data(n, p, seed=321, intercept=0.2):
    """poisson_bench.data's rows with both responses: Gamma (shape 2) and Poisson of the same mean"""
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: int(0.4 * p)] = 0.5
    g = torch.Generator(device="cuda").manual_seed(9)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    mu = torch.exp(X @ beta + intercept + o)
    yp = torch.poisson(mu, generator=g)
    return X, gamma2(mu, g), yp, o, beta


def pass_case(n, p, reps):
    X, yg, yp, o, beta = data(n, p)
    b = beta * 0.5
    tg, tp = alternating(lambda: engine.gamma_pass(X, yg, b, offset=o, want_H=False, want_w=True),
                         lambda: engine.poisson_pass(X, yp, b, offset=o, want_H=False, want_w=True), reps)
    gb = 8.0 * n * p
    return {"case": "pass", "n": n, "p": p, **sides("gamma", tg, "poisson", tp),
            "gamma_TBps": round(gb / (tg[0] * 1e-3) / 1e12, 3), "poisson_TBps": round(gb / (tp[0] * 1e-3) / 1e12, 3)}


def iter_case(n, p, reps):
    X, yg, yp, o, beta = data(n, p)
    b = beta * 0.5

    def gamma():
        H, g = engine.gamma_pass(X, yg, b, offset=o)[:2]
        engine.spd_solve(H, g)

    def poisson():
        H, g = engine.poisson_pass(X, yp, b, offset=o)[:2]
        engine.spd_solve(H, g)
    tg, tp = alternating(gamma, poisson, reps)
    return {"case": "iter", "n": n, "p": p, **sides("gamma_newton_iter", tg, "poisson_newton_iter", tp)}


def wall(fn, reps):
    r = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3 / reps


def fit_case(n, p, reps):
    X, yg, yp, o, _ = data(n, p)
    mg, t_g = wall(lambda: dlsa_amd.fit_gamma_partitions(X, yg, fit_intercept=True, offset=o), reps)
    mp, t_p = wall(lambda: dlsa_amd.fit_poisson_partitions(X, yp, fit_intercept=True, offset=o), reps)
    return {"case": "fit", "n": n, "p": p, "gamma_fit_ms": round(t_g, 2), "gamma_iters": mg.n_iter, "poisson_fit_ms": round(t_p, 2),
            "poisson_iters": mp.n_iter, "status_ok": mg.status == [0] and mp.status == [0], "dispersion": round(mg.extra["dispersion"][0], 5)}


def airline_gamma(n):
    """poisson_bench.airline_poisson's rows with a Gamma response of the same mean (shape 2) in d["resp"]"""
    d = airline_poisson(n)
    num, codes, beta = d["num"], d["codes"], d["beta"]
    q = num.shape[1]
    eta = beta[0] + ((num - 1.5) / 3.0) @ beta[1:1 + q]
    pos = 1 + q
    for fi, L in enumerate(d["levels"]):
        tab = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), beta[pos:pos + L - 1]])
        eta = eta + tab[codes[:, fi].long()]
        pos += L - 1
    mu = torch.exp(eta + d["offset"])
    d["resp"] = gamma2(mu, torch.Generator(device="cuda").manual_seed(10))
    return d


def oh_pass_case(n, reps):
    d = airline_gamma(n)
    plan, num, codes, yg, yp, o = d["plan"], d["num"], d["codes"], d["resp"], d["counts"], d["offset"]
    b = d["beta"] * 0.5
    q, f = num.shape[1], codes.shape[1]
    tg, tp = alternating(lambda: engine.onehot_gamma_pass(plan, num, codes, yg, b, offset=o, want_H=False, want_w=True),
                         lambda: engine.onehot_poisson_pass(plan, num, codes, yp, b, offset=o, want_H=False, want_w=True), reps)
    return {"case": "oh_pass", "n": n, "p": d["p"], **sides("gamma", tg, "poisson", tp),
            "bytes_ratio": round((8 * q + 4 * f + 32) / (8 * q + 4 * f + 24), 3)}


def oh_newton_case(n, reps):
    d = airline_gamma(n)
    plan, num, codes, yg, yp, o = d["plan"], d["num"], d["codes"], d["resp"], d["counts"], d["offset"]
    b = d["beta"] * 0.5
    tg, tp = alternating(lambda: engine.onehot_gamma_pass(plan, num, codes, yg, b, offset=o),
                         lambda: engine.onehot_poisson_pass(plan, num, codes, yp, b, offset=o), reps)
    return {"case": "oh_newton", "n": n, "p": d["p"], **sides("gamma_eval", tg, "poisson_eval", tp)}


def oh_fit_case(n, K, reps):
    d = airline_gamma(n)
    plan, num, codes, y, o = d["plan"], d["num"], d["codes"], d["resp"], d["offset"]
    del d["y"], d["counts"]
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    raw = num.numel() * 8 + codes.numel() * 4 + y.numel() * 8 + o.numel() * 8

    def fresh():
        torch.cuda.synchronize()
        engine.release_workspace()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    fresh()
    structured = lambda: engine.onehot_gamma_fit_ex(plan, num, codes, y, first, rows, row_step=K, offset=o)   # noqa: E731
    rs, t_s = wall(structured, reps)
    peak_s = torch.cuda.max_memory_allocated()
    fresh()
    X, _ = engine.design(num, codes, *d["spec"])
    rd, t_d = wall(lambda: engine.gamma_fit_ex(X, y, first, rows, row_step=K, offset=o), reps)
    peak_d = torch.cuda.max_memory_allocated()
    gap = float((rs["coef"] - rd["coef"]).abs().max() / rd["coef"].abs().max())
    return {"case": "oh_fit", "n": n, "p": d["p"], "partitions": K, "structured_fit_ms": round(t_s, 2), "dense_fit_ms": round(t_d, 2),
            "ratio": round(t_s / t_d, 3), "iters_structured": rs["n_iter"][:4], "iters_dense": rd["n_iter"][:4],
            "status_ok": all(s == 0 for s in rs["status"]) and all(s == 0 for s in rd["status"]), "coef_rel_gap": gap,
            "dispersion": [round(v, 5) for v in rs["dispersion"][:4]], "raw_GB": round(raw / 1e9, 3),
            "structured_peak_GB": round(peak_s / 1e9, 3), "dense_peak_GB": round(peak_d / 1e9, 3)}


def structured_main(a):
    n = 1_000_000 if a.small else 4_000_000
    print(json.dumps(oh_pass_case(1_000_000, a.reps * 4)), flush=True)
    torch.cuda.empty_cache()
    print(json.dumps(oh_newton_case(1_000_000, a.reps * 2)), flush=True)
    torch.cuda.empty_cache()
    print(json.dumps(oh_fit_case(n, n // 1_000_000, max(1, a.reps // 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1e6 x 100 only (a quick check)")
    ap.add_argument("--structured", action="store_true", help="the structured one-hot leg only (airline-shaped rows)")
    a = ap.parse_args()
    if a.structured:
        return structured_main(a)
    shapes = [(1_000_000, 100)] if a.small else [(10_000_000, 100), (2_000_000, 500)]
    for n, p in shapes:
        print(json.dumps(pass_case(n, p, a.reps)), flush=True)
        torch.cuda.empty_cache()
        print(json.dumps(iter_case(n, p, a.reps)), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(fit_case(shapes[0][0], shapes[0][1], max(1, a.reps // 2))), flush=True)


if __name__ == "__main__":
    main()
