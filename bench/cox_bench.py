"""Timing of the Cox map step (csrc/cox.hip): one Newton iteration (dlsa_cox_pass_f64 + the Cholesky solve) and the scan pass
alone, at 1e7 x 100 and 2e6 x 500, on rows stored in time order and on shuffled rows.  Prints one JSON line per case with the
algorithmic bandwidth of the row passes against the traffic model:
  eta pass + scan pass: 2 reads of the rows (8 p bytes each) + the Gram's read of the rows (8 p) + A written and read
  (8 p per event row).  Run under rocprofv3 --kernel-trace --stats for the per-kernel split.
--ties efron times Efron's approximation (ties="efron"), --tie-levels N rounds the times onto N quantile levels first (1 = all
rows tied); with either, the JSON line also names the method, the levels and the number of A rows (Breslow: the groups with
events; Efron: one more for every group of two events or more), and the model counts those rows.
--strata S gives every row a random stratum code out of S (one baseline hazard per stratum, tie groups cut at the strata);
--matched M makes sets of M consecutive rows with one event each, the row that leaves first (conditional logistic regression
on 1:M-1 matched sets: n / M strata).  With either, `order` is sorted on (stratum, -time), "sorted" stores the rows in that
order, and the JSON line names the stratum count; the model adds the flag byte that each of the three walks reads per position
(3n) and the flag kernel's gathers (12n: order twice and two codes per position), which the pass entry timed here runs on every
call while the fit runs them once per partition."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dlsa_amd import engine  # noqa: E402


def a_rows(t, ev, ties, strata=None):
    """rows of A: tie groups with events, and under Efron once more those with two events or more (groups cut at the strata)"""
    lv, inv = torch.unique(t, return_inverse=True)
    if strata is not None:
        _, sinv = torch.unique(strata, return_inverse=True)
        _, inv = torch.unique(sinv * lv.numel() + inv, return_inverse=True)
    d = torch.bincount(inv, weights=ev)
    return int((d > 0).sum().item()) + (int((d > 1).sum().item()) if ties == "efron" else 0)


def case(n, p, shuffled, reps, ties="breslow", tie_levels=None, strata=None, matched=None):
    X, _ = engine.synth(321, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: int(0.4 * p)] = 1.0
    g = torch.Generator(device="cuda").manual_seed(9)
    t = torch.empty(n, dtype=torch.float64, device="cuda").exponential_(generator=g) / torch.exp(X @ beta)
    ev = (torch.rand(n, dtype=torch.float64, device="cuda", generator=g) > 0.3).to(torch.float64)
    if tie_levels:
        if tie_levels == 1:
            t = torch.ones_like(t)
        else:       # the quantile levels of an evenly spaced sample of the sorted times (torch.quantile is limited to 16M elements)
            q = torch.sort(t).values[torch.linspace(0, n - 1, tie_levels + 1, device="cuda").round().long()[1:]]
            t = q[torch.clamp(torch.searchsorted(q, t), max=tie_levels - 1)]
    codes = None
    if matched:
        n = n // matched * matched
        X, t = X[:n], t[:n]
        codes = (torch.arange(n, device="cuda") // matched).to(torch.int32)
        ev = torch.zeros(n, dtype=torch.float64, device="cuda")
        ev[torch.arange(n // matched, device="cuda") * matched + t.view(-1, matched).argmin(1)] = 1.0
    elif strata:
        codes = torch.randint(0, strata, (n,), device="cuda", generator=g).to(torch.int32)
    order = torch.sort(-t, stable=True).indices
    if codes is not None:
        order = order[torch.sort(codes[order], stable=True).indices]
    if not shuffled:                 # store the rows in the order they are read: `order` becomes the identity
        X = X[order].contiguous(); t = t[order].contiguous(); ev = ev[order].contiguous()
        if codes is not None:
            codes = codes[order].contiguous()
        order = torch.arange(n, device="cuda", dtype=torch.int64)
    b = beta * 0.5
    extra = {} if ties == "breslow" and not tie_levels else {"ties": ties}      # (the default run calls what it always called)
    if codes is not None:
        extra["ties"] = ties
        extra["strata"] = codes
    for _ in range(2):
        engine.cox_pass(X, t, ev, order, b, **extra)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        H, gr, ll, _ = engine.cox_pass(X, t, ev, order, b, **extra)
        engine.spd_solve(H, gr)
    e1.record()
    torch.cuda.synchronize()
    it_ms = e0.elapsed_time(e1) / reps
    events = float(ev.sum().item())
    if not extra:
        traffic = 8.0 * p * (3 * n + 2 * events)
        return {"n": n, "p": p, "order": "shuffled" if shuffled else "sorted", "newton_iter_ms": round(it_ms, 3),
                "events": int(events), "model_bytes": traffic, "algorithmic_TBps_iter": round(traffic / (it_ms * 1e-3) / 1e12, 3)}
    rows = a_rows(t, ev, ties, codes)
    traffic = 8.0 * p * (3 * n + 2 * rows)
    out = {"n": n, "p": p, "order": "shuffled" if shuffled else "sorted", "ties": ties, "tie_levels": tie_levels or 0}
    if codes is not None:
        traffic += 3.0 * n + 12.0 * n          # flag reads of the three walks + the flag kernel (per call of the pass entry)
        out["strata"] = int(torch.unique(codes).numel())
        out["matched"] = matched or 0
    out.update({"newton_iter_ms": round(it_ms, 3), "events": int(events), "a_rows": rows, "model_bytes": traffic,
                "algorithmic_TBps_iter": round(traffic / (it_ms * 1e-3) / 1e12, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1e6 x 100 only (a quick check)")
    ap.add_argument("--ties", choices=["breslow", "efron"], default="breslow")
    ap.add_argument("--tie-levels", type=int, default=None, help="round the times onto N quantile levels (1: all rows tied)")
    ap.add_argument("--strata", type=int, default=None, help="random stratum codes over S strata")
    ap.add_argument("--matched", type=int, default=None, help="matched sets of M rows with one event each (n / M strata)")
    ap.add_argument("--shape", default=None, help="N,P: that shape alone")
    ap.add_argument("--layout", choices=["sorted", "shuffled"], default=None, help="that row layout alone")
    a = ap.parse_args()
    shapes = [(1_000_000, 100)] if a.small else [(10_000_000, 100), (2_000_000, 500)]
    if a.shape:
        shapes = [tuple(int(v) for v in a.shape.split(","))]
    for n, p in shapes:
        for sh in (False, True):
            if a.layout and (a.layout == "shuffled") != sh:
                continue
            print(json.dumps(case(n, p, sh, a.reps, a.ties, a.tie_levels, a.strata, a.matched)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
