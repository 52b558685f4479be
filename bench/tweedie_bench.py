"""Timing of the Tweedie map step (csrc/tweedie.hip) next to the Gamma one -- the GammaRow instantiation of the same row-pass kernel
in the same build -- on the same rows.  Every pair is timed alternating in one call, five rounds of `reps` calls each; each side
reports its median and its run-to-run spread (fastest .. slowest of the rounds).  Prints one JSON line per case:
  pass      the Tweedie pass alone (w, g, loglik) next to engine.gamma_pass on the same rows, with the algorithmic bandwidth of one
            read of the rows (8 p bytes per row);
  iter      one Newton evaluation + solve (dlsa_tweedie_pass_f64 with H + the Cholesky solve) next to the Gamma one;
  fit       a whole fit of 1e7 x 100 with an intercept and offsets (one partition, estimated dispersion) next to the Gamma fit.
With --structured (a leg of its own) the structured one-hot path (csrc/onehot_tweedie.hip) on bench/surrogates.airline_shaped rows
with compound Poisson-Gamma responses (power 1.5, dispersion 1, exposure ~ U(0.5, 2)):
  oh_pass   the structured Tweedie pass next to the structured Gamma pass (the same bytes per row: 8q + 4f + 32);
  oh_newton a structured Newton evaluation (pass + H) next to the Gamma one -- the same ordered Gram on both sides;
  oh_fit    the structured Tweedie fit of 1e6-row partitions next to the structured Gamma fit of the same partitions.
Run under rocprofv3 --kernel-trace --stats for the per-kernel split."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlsa_amd  # noqa: E402
from dlsa_amd import engine  # noqa: E402
from gamma_bench import airline_gamma, alternating, gamma2, sides  # noqa: E402

POWER = 1.5


def compound(mu, power, dispersion, g):
    """compound Poisson-Gamma draws of mean mu and variance dispersion * mu^power on the device: N ~ Poisson(mu^(2 - xi) / (phi (2 - xi))),
    y ~ Gamma(shape N (2 - xi) / (xi - 1), scale phi (xi - 1) mu^(xi - 1)), 0 at N = 0"""
    N = torch.poisson(mu ** (2.0 - power) / (dispersion * (2.0 - power)), generator=g)
    shape = N.clamp_min(1.0) * ((2.0 - power) / (power - 1.0))
    draws = torch._standard_gamma(shape, generator=g) * (dispersion * (power - 1.0)) * mu ** (power - 1.0)
    return torch.where(N > 0, draws, torch.zeros_like(draws))


def data(n, p, seed=321, intercept=0.2):
    """gamma_bench.data's rows with both responses: Tweedie (power 1.5, dispersion 1: about a tenth of the rows zero) and Gamma (shape
    2) of the same mean"""
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: int(0.4 * p)] = 0.5
    g = torch.Generator(device="cuda").manual_seed(9)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    mu = torch.exp(X @ beta + intercept + o)
    return X, compound(mu, POWER, 1.0, g), gamma2(mu, g), o, beta


def pass_case(n, p, reps):
    X, yt, yg, o, beta = data(n, p)
    b = beta * 0.5
    tt, tg = alternating(lambda: engine.tweedie_pass(X, yt, b, POWER, offset=o, want_H=False, want_w=True),
                         lambda: engine.gamma_pass(X, yg, b, offset=o, want_H=False, want_w=True), reps)
    gb = 8.0 * n * p
    return {"case": "pass", "n": n, "p": p, "zero_share": round(float((yt == 0).double().mean()), 4), **sides("tweedie", tt, "gamma", tg),
            "tweedie_TBps": round(gb / (tt[0] * 1e-3) / 1e12, 3), "gamma_TBps": round(gb / (tg[0] * 1e-3) / 1e12, 3)}


def iter_case(n, p, reps):
    X, yt, yg, o, beta = data(n, p)
    b = beta * 0.5

    def tweedie():
        H, g = engine.tweedie_pass(X, yt, b, POWER, offset=o)[:2]
        engine.spd_solve(H, g)

    def gamma():
        H, g = engine.gamma_pass(X, yg, b, offset=o)[:2]
        engine.spd_solve(H, g)
    tt, tg = alternating(tweedie, gamma, reps)
    return {"case": "iter", "n": n, "p": p, **sides("tweedie_newton_iter", tt, "gamma_newton_iter", tg)}


def fit_case(n, p, reps):
    X, yt, yg, o, _ = data(n, p)
    last = {}

    def tweedie():
        last["t"] = dlsa_amd.fit_tweedie_partitions(X, yt, fit_intercept=True, offset=o, power=POWER)

    def gamma():
        last["g"] = dlsa_amd.fit_gamma_partitions(X, yg, fit_intercept=True, offset=o)
    tt, tg = alternating(tweedie, gamma, reps)
    mt, mg = last["t"], last["g"]
    per = (tt[0] / mt.n_iter[0]) / (tg[0] / mg.n_iter[0])
    return {"case": "fit", "n": n, "p": p, **sides("tweedie_fit", tt, "gamma_fit", tg), "tweedie_iters": mt.n_iter, "gamma_iters": mg.n_iter,
            "ratio_per_evaluation": round(per, 3), "status_ok": mt.status == [0] and mg.status == [0],
            "dispersion": round(mt.extra["dispersion"][0], 5)}


def airline_tweedie(n):
    """gamma_bench.airline_gamma's rows with a Tweedie response of the same mean in d["tw"] (d["resp"] stays the Gamma one)"""
    d = airline_gamma(n)
    num, codes, beta = d["num"], d["codes"], d["beta"]
    q = num.shape[1]
    eta = beta[0] + ((num - 1.5) / 3.0) @ beta[1:1 + q]
    pos = 1 + q
    for fi, L in enumerate(d["levels"]):
        tab = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), beta[pos:pos + L - 1]])
        eta = eta + tab[codes[:, fi].long()]
        pos += L - 1
    d["tw"] = compound(torch.exp(eta + d["offset"]), POWER, 1.0, torch.Generator(device="cuda").manual_seed(11))
    return d


def oh_pass_case(n, reps):
    d = airline_tweedie(n)
    plan, num, codes, yt, yg, o = d["plan"], d["num"], d["codes"], d["tw"], d["resp"], d["offset"]
    b = d["beta"] * 0.5
    tt, tg = alternating(lambda: engine.onehot_tweedie_pass(plan, num, codes, yt, b, POWER, offset=o, want_H=False, want_w=True),
                         lambda: engine.onehot_gamma_pass(plan, num, codes, yg, b, offset=o, want_H=False, want_w=True), reps)
    return {"case": "oh_pass", "n": n, "p": d["p"], "zero_share": round(float((yt == 0).double().mean()), 4), **sides("tweedie", tt, "gamma", tg)}


def oh_newton_case(n, reps):
    d = airline_tweedie(n)
    plan, num, codes, yt, yg, o = d["plan"], d["num"], d["codes"], d["tw"], d["resp"], d["offset"]
    b = d["beta"] * 0.5
    tt, tg = alternating(lambda: engine.onehot_tweedie_pass(plan, num, codes, yt, b, POWER, offset=o),
                         lambda: engine.onehot_gamma_pass(plan, num, codes, yg, b, offset=o), reps)
    return {"case": "oh_newton", "n": n, "p": d["p"], **sides("tweedie_eval", tt, "gamma_eval", tg)}


def oh_fit_case(n, K, reps):
    d = airline_tweedie(n)
    plan, num, codes, yt, yg, o = d["plan"], d["num"], d["codes"], d["tw"], d["resp"], d["offset"]
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    last = {}

    def tweedie():
        last["t"] = engine.onehot_tweedie_fit_ex(plan, num, codes, yt, first, rows, row_step=K, offset=o, power=POWER)

    def gamma():
        last["g"] = engine.onehot_gamma_fit_ex(plan, num, codes, yg, first, rows, row_step=K, offset=o)
    tt, tg = alternating(tweedie, gamma, reps)
    rt, rg = last["t"], last["g"]
    per = (tt[0] / sum(rt["n_iter"])) / (tg[0] / sum(rg["n_iter"]))
    return {"case": "oh_fit", "n": n, "p": d["p"], "partitions": K, **sides("tweedie_fit", tt, "gamma_fit", tg),
            "tweedie_iters": rt["n_iter"][:4], "gamma_iters": rg["n_iter"][:4], "ratio_per_evaluation": round(per, 3),
            "status_ok": all(s == 0 for s in rt["status"]) and all(s == 0 for s in rg["status"]),
            "dispersion": [round(v, 5) for v in rt["dispersion"][:4]]}


def structured_main(a):
    print(json.dumps(oh_pass_case(1_000_000, a.reps * 4)), flush=True)
    torch.cuda.empty_cache()
    print(json.dumps(oh_newton_case(1_000_000, a.reps * 2)), flush=True)
    torch.cuda.empty_cache()
    print(json.dumps(oh_fit_case(1_000_000, 1, max(1, a.reps // 2))), flush=True)


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
