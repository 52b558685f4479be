"""Timing of the Poisson map step (csrc/poisson.hip).  Prints one JSON line per case:
  pass      the Poisson pass alone (w, g, loglik) next to engine.logit_pass on the same rows in the same run, with the algorithmic
            bandwidth of one read of the rows (8 p bytes per row);
  iter      one Newton iteration (dlsa_poisson_pass_f64 with H + the Cholesky solve) next to its parts run one after another
            (the pass without H, the weighted dlsa_gram_f64, the solve);
  fit       a whole fit of 1e7 x 100 with an intercept and offsets (one partition);
  strided   2.5e7 x 500 as 25 strided partitions (partition_id = i % 25) with an intercept, and the peak device memory.
With --structured (a leg of its own; the plain run stays as it is) the structured one-hot path (csrc/onehot_poisson.hip) on
bench/surrogates.airline_shaped rows with Poisson counts (exposure ~ U(0.5, 2)), every pair timed in one call and alternating:
  oh_pass   the structured Poisson pass next to engine.onehot_logit_pass on the same rows (bytes per row 8q + 4f + 24 against
            8q + 4f + 16; target: time ratio <= bytes ratio x 1.15);
  oh_newton a structured Newton evaluation (pass + H) next to onehot_logit_pass + onehot_gram with caller weights -- the same
            ordered Gram on both sides (target <= 1.1);
  oh_fit    the structured fit of 1e6-row partitions next to the dense Poisson fit of the same partitions (matrix built once, build
            time reported separately), with the peak device memory of both (peak statistics reset after the data are generated).
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


def alternating(fa, fb, reps, rounds=5):
    """fa and fb timed in turns in the same call: (median ms of fa, median ms of fb) over `rounds` rounds of `reps` calls each"""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    ta.sort(); tb.sort()
    return ta[len(ta) // 2], tb[len(tb) // 2]


def airline_poisson(n, seed=7):
    """airline_shaped rows with counts y ~ Poisson(exposure * exp(eta)) from its beta, exposure ~ U(0.5, 2); the logistic labels stay
    in d["y"] for the logit pass"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import surrogates
    d = surrogates.airline_shaped(n, seed=seed, dense=False)
    num, codes, beta = d["num"], d["codes"], d["beta"]
    q = num.shape[1]
    g = torch.Generator(device="cuda").manual_seed(9)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    eta = beta[0] + ((num - 1.5) / 3.0) @ beta[1:1 + q]
    pos = 1 + q
    for fi, L in enumerate(d["levels"]):
        tab = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), beta[pos:pos + L - 1]])
        eta = eta + tab[codes[:, fi].long()]
        pos += L - 1
    d["counts"] = torch.poisson(torch.exp(eta + o), generator=g)
    d["offset"] = o
    return d


def oh_pass_case(n, reps):
    d = airline_poisson(n)
    plan, num, codes, y, yl, o = d["plan"], d["num"], d["codes"], d["counts"], d["y"], d["offset"]
    b = d["beta"] * 0.5
    q, f = num.shape[1], codes.shape[1]
    t_pois, t_logit = alternating(lambda: engine.onehot_poisson_pass(plan, num, codes, y, b, offset=o, want_H=False, want_w=True),
                                  lambda: engine.onehot_logit_pass(plan, num, codes, yl, b), reps)
    t_noff, _ = alternating(lambda: engine.onehot_poisson_pass(plan, num, codes, y, b, want_H=False, want_w=True),
                            lambda: engine.onehot_logit_pass(plan, num, codes, yl, b), reps, rounds=3)
    bp, bl = 8 * q + 4 * f + 24, 8 * q + 4 * f + 16
    return {"case": "oh_pass", "n": n, "p": d["p"], "poisson_offset_ms": round(t_pois, 4), "poisson_ms": round(t_noff, 4),
            "logit_ms": round(t_logit, 4), "ratio_vs_logit": round(t_pois / t_logit, 3), "bytes_ratio": round(bp / bl, 3),
            "target_ratio": round(bp / bl * 1.15, 3), "target_met": bool(t_pois / t_logit <= bp / bl * 1.15),
            "poisson_TBps": round(bp * n / (t_pois * 1e-3) / 1e12, 3), "logit_TBps": round(bl * n / (t_logit * 1e-3) / 1e12, 3)}


def oh_newton_case(n, reps):
    d = airline_poisson(n)
    plan, num, codes, y, yl, o = d["plan"], d["num"], d["codes"], d["counts"], d["y"], d["offset"]
    b = d["beta"] * 0.5

    def pois():
        engine.onehot_poisson_pass(plan, num, codes, y, b, offset=o)

    def logit():
        w, _, _ = engine.onehot_logit_pass(plan, num, codes, yl, b)
        engine.onehot_gram(plan, num, codes, w)              # caller weights: the ordered floating-point Gram
    t_pois, t_logit = alternating(pois, logit, reps)
    return {"case": "oh_newton", "n": n, "p": d["p"], "poisson_eval_ms": round(t_pois, 4), "logit_pass_plus_gram_ms": round(t_logit, 4),
            "ratio": round(t_pois / t_logit, 3), "target_ratio": 1.1, "target_met": bool(t_pois / t_logit <= 1.1)}


def oh_fit_case(n, K, reps):
    d = airline_poisson(n)
    plan, num, codes, y, o = d["plan"], d["num"], d["codes"], d["counts"], d["offset"]
    del d["y"]
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    raw = num.numel() * 8 + codes.numel() * 4 + y.numel() * 8 + o.numel() * 8

    def peak_of(fn):
        torch.cuda.synchronize()
        engine.release_workspace()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        r = fn()
        torch.cuda.synchronize()
        return r, torch.cuda.max_memory_allocated()

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3 / reps
    structured = lambda: engine.onehot_poisson_fit_ex(plan, num, codes, y, first, rows, row_step=K, offset=o)
    rs, peak_s = peak_of(structured)
    rs, t_s = wall(structured)
    torch.cuda.synchronize()
    engine.release_workspace()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    X, _ = engine.design(num, codes, *d["spec"])
    torch.cuda.synchronize()
    t_build = (time.perf_counter() - t0) * 1e3
    dense = lambda: engine.poisson_fit_ex(X, y, first, rows, row_step=K, offset=o)
    rd = dense()
    torch.cuda.synchronize()
    peak_d = torch.cuda.max_memory_allocated()
    rd, t_d = wall(dense)
    gap = float((rs["coef"] - rd["coef"]).abs().max() / rd["coef"].abs().max())
    return {"case": "oh_fit", "n": n, "p": d["p"], "partitions": K, "structured_fit_ms": round(t_s, 2), "dense_fit_ms": round(t_d, 2),
            "dense_build_ms": round(t_build, 2), "ratio": round(t_s / t_d, 3), "not_slower": bool(t_s <= t_d),
            "iters_structured": rs["n_iter"][:4], "iters_dense": rd["n_iter"][:4],
            "status_ok": all(s == 0 for s in rs["status"]) and all(s == 0 for s in rd["status"]), "coef_rel_gap": gap,
            "raw_GB": round(raw / 1e9, 3), "structured_peak_GB": round(peak_s / 1e9, 3), "dense_peak_GB": round(peak_d / 1e9, 3),
            "structured_peak_below_raw_plus_1GB": bool(peak_s < raw + 1e9)}


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
    ap.add_argument("--no-strided", action="store_true", help="skip the 2.5e7 x 500 case (100 GB of rows)")
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
    print(json.dumps(fit_case(shapes[0][0], shapes[0][1], 1, max(1, a.reps // 2), False)), flush=True)
    torch.cuda.empty_cache()
    if not a.small and not a.no_strided:
        engine.release_workspace()
        torch.cuda.empty_cache()
        print(json.dumps(fit_case(25_000_000, 500, 25, 1, True)), flush=True)


if __name__ == "__main__":
    main()
