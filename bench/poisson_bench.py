"""Timing of the Poisson map step (csrc/poisson.hip).  Prints one JSON line per case:
  pass      the Poisson pass alone (w, g, loglik) next to engine.logit_pass on the same rows in the same run, with the algorithmic
            bandwidth of one read of the rows (8 p bytes per row);
  iter      one Newton iteration (dlsa_poisson_pass_f64 with H + the Cholesky solve) next to its parts run one after another
            (the pass without H, the weighted dlsa_gram_f64, the solve);
  fit       a whole fit of 1e7 x 100 with an intercept and offsets (one partition);
  strided   2.5e7 x 500 as 25 strided partitions (partition_id = i % 25) with an intercept, and the peak device memory.
Run under rocprofv3 --kernel-trace --stats for the per-kernel split."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlsa_amd  # noqa: E402
from dlsa_amd import engine  # noqa: E402


def timed(fn, reps):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def data(n, p, seed=321, intercept=0.2, offset=True):
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: int(0.4 * p)] = 0.5
    g = torch.Generator(device="cuda").manual_seed(9)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5) if offset else None
    eta = X @ beta + intercept + (o if offset else 0.0)
    y = torch.poisson(torch.exp(eta), generator=g)
    yl = (torch.rand(n, dtype=torch.float64, device="cuda", generator=g) < torch.sigmoid(eta)).to(torch.float64)
    return X, y, o, yl, beta


def pass_case(n, p, reps):
    X, y, o, yl, beta = data(n, p)
    b = beta * 0.5
    t_pois = timed(lambda: engine.poisson_pass(X, y, b, want_H=False, want_w=True), reps)
    t_pois_off = timed(lambda: engine.poisson_pass(X, y, b, offset=o, want_H=False, want_w=True), reps)
    t_logit = timed(lambda: engine.logit_pass(X, yl, b), reps)
    gb = 8.0 * n * p
    return {"case": "pass", "n": n, "p": p, "poisson_ms": round(t_pois, 3), "poisson_offset_ms": round(t_pois_off, 3),
            "logit_ms": round(t_logit, 3), "ratio_vs_logit": round(t_pois / t_logit, 3),
            "poisson_TBps": round(gb / (t_pois * 1e-3) / 1e12, 3), "logit_TBps": round(gb / (t_logit * 1e-3) / 1e12, 3)}


def iter_case(n, p, reps):
    X, y, o, _, beta = data(n, p)
    b = beta * 0.5

    def fused():
        H, g, _, _ = engine.poisson_pass(X, y, b, offset=o)
        engine.spd_solve(H, g)

    def parts():
        _, g, _, w = engine.poisson_pass(X, y, b, offset=o, want_H=False, want_w=True)
        H = engine.gram(X, w)
        engine.spd_solve(H, g)
    t_it, t_parts = timed(fused, reps), timed(parts, reps)
    return {"case": "iter", "n": n, "p": p, "newton_iter_ms": round(t_it, 3), "pass_gram_solve_ms": round(t_parts, 3),
            "ratio": round(t_it / t_parts, 3)}


def fit_case(n, p, K, reps, strided):
    X, y, o, _, _ = data(n, p, offset=not strided)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()

    def run():
        return dlsa_amd.fit_poisson_partitions(X, y, partition_num=K, fit_intercept=True, offset=o)
    mb = run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        mb = run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    return {"case": "strided" if strided else "fit", "n": n, "p": p, "partitions": K, "fit_ms": round(ms, 2),
            "iters": mb.n_iter[:4], "status_ok": all(s == 0 for s in mb.status),
            "peak_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2), "data_GB": round(base / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1e6 x 100 only (a quick check)")
    ap.add_argument("--no-strided", action="store_true", help="skip the 2.5e7 x 500 case (100 GB of rows)")
    a = ap.parse_args()
    shapes = [(1_000_000, 100)] if a.small else [(10_000_000, 100), (2_000_000, 500)]
    for n, p in shapes:
        print(json.dumps(pass_case(n, p, a.reps)), flush=True)
        torch.cuda.empty_cache()
        print(json.dumps(iter_case(n, p, a.reps)), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(fit_case(shapes[0][0], shapes[0][1], 1, max(1, a.reps // 2), False)), flush=True)
    torch.cuda.empty_cache()
    if not a.small and not a.no_strided:
        engine.release_workspace()
        torch.cuda.empty_cache()
        print(json.dumps(fit_case(25_000_000, 500, 25, 1, True)), flush=True)


if __name__ == "__main__":
    main()
