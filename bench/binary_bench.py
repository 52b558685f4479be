"""Timing of the probit and cloglog map steps (csrc/binary.hip).  Prints one JSON line per case:
  pass      the link's pass alone (w, g, loglik) next to engine.poisson_pass on the SAME rows in the same run, every pair timed in
            turns, with the algorithmic bandwidth of one read of the rows (8 p bytes per row).  The Poisson pass is timed on the 0/1
            response (its time does not depend on the counts' values);
  fit       a whole fit of the rows with an intercept and offsets (one partition) next to the Poisson fit of the same rows.
--link probit | cloglog | both.  The expectation this bench is there to confirm or refute: at p >= 64 the pass is bound by the row
stream like the Poisson pass, at narrow p the transcendentals of the row terms show.  Run under rocprofv3 --kernel-trace --stats for
the per-kernel split."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlsa_amd  # noqa: E402
from dlsa_amd import engine  # noqa: E402

LINKS = ("probit", "cloglog")


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


def alternating(fa, fb, reps, rounds=5):
    """fa and fb timed in turns in the same call: (median ms of fa, median ms of fb) over `rounds` rounds of `reps` calls each"""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    ta.sort(); tb.sort()
    return ta[len(ta) // 2], tb[len(tb) // 2]


def data(link, n, p, seed=321, intercept=-0.5):
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: max(1, int(0.4 * p))] = 0.5
    g = torch.Generator(device="cuda").manual_seed(9)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    eta = X @ beta + intercept + o
    prob = -torch.expm1(-torch.exp(eta)) if link == "cloglog" else torch.special.ndtr(eta)
    y = (torch.rand(n, dtype=torch.float64, device="cuda", generator=g) < prob).to(torch.float64)
    return X, y, o, beta


def pass_case(link, n, p, reps):
    X, y, o, beta = data(link, n, p)
    b = beta * 0.5
    run = getattr(engine, link + "_pass")
    t_link, t_pois = alternating(lambda: run(X, y, b, offset=o, want_H=False, want_w=True),
                                 lambda: engine.poisson_pass(X, y, b, offset=o, want_H=False, want_w=True), reps)
    gb = 8.0 * n * p
    return {"case": "pass", "link": link, "n": n, "p": p, link + "_ms": round(t_link, 4), "poisson_ms": round(t_pois, 4),
            "ratio_vs_poisson": round(t_link / t_pois, 3), link + "_TBps": round(gb / (t_link * 1e-3) / 1e12, 3),
            "poisson_TBps": round(gb / (t_pois * 1e-3) / 1e12, 3), "response_share": round(float(y.mean()), 3)}


def fit_case(link, n, p, reps):
    X, y, o, _ = data(link, n, p)
    fit = getattr(dlsa_amd, "fit_%s_partitions" % link)

    def wall(fn):
        mb = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            mb = fn()
        torch.cuda.synchronize()
        return mb, (time.perf_counter() - t0) * 1e3 / reps
    mb, ms = wall(lambda: fit(X, y, fit_intercept=True, offset=o))
    mp, ms_p = wall(lambda: dlsa_amd.fit_poisson_partitions(X, y, fit_intercept=True, offset=o))
    return {"case": "fit", "link": link, "n": n, "p": p, "fit_ms": round(ms, 2), "iters": mb.n_iter, "status_ok": all(s == 0 for s in mb.status),
            "poisson_fit_ms": round(ms_p, 2), "poisson_iters": mp.n_iter, "ms_per_iter": round(ms / max(1, mb.n_iter[0]), 2),
            "poisson_ms_per_iter": round(ms_p / max(1, mp.n_iter[0]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--link", choices=LINKS + ("both",), default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1e6 rows only (a quick check)")
    a = ap.parse_args()
    n = 1_000_000 if a.small else 4_000_000
    for link in (LINKS if a.link == "both" else (a.link,)):
        for p in (4, 16, 64, 128, 500):
            rows = n if p <= 128 else n // 4
            print(json.dumps(pass_case(link, rows, p, a.reps)), flush=True)
            torch.cuda.empty_cache()
        print(json.dumps(fit_case(link, n, 100, max(1, a.reps // 2))), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
