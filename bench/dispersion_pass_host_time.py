#!/usr/bin/env python3
"""Wall time per call of the four Gamma / Tweedie pass entries at a size where the host side dominates (n = 700, p = 5 with the
intercept and offsets; the structured entries on 2 numerics and factors of 3 and 4 levels): `rounds` rounds of `calls` back-to-back
calls of the C ABI with prepared arguments, one synchronisation per round.  Prints one JSON line per entry with the median round
and the spread (min .. max of the rounds), in microseconds per call.  Run it in a checkout of each build to compare two builds."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    from dlsa_amd import _lib, engine
    lib = _lib.load()
    n, p = 700, 5
    rng = np.random.default_rng(21)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    X, off = dev(rng.uniform(-0.5, 0.5, (n, p))), dev(np.log(rng.uniform(0.5, 2.0, n)))
    y = dev(rng.gamma(2.0, 0.5, n))
    num = dev(rng.normal(size=(n, 2)) * 0.3)
    codes = dev(np.stack([rng.integers(0, 3, n), rng.integers(0, 4, n)], 1).astype(np.int32))
    arr = lambda v, t: np.asarray(v, dtype=t)
    plan = engine.OnehotPlan(8, arr([0, 1, 1], np.int32), arr([0, 0, 1], np.int32), arr([0.0, 0.2, -0.1], np.float64),
                             arr([1.0, 1.5, 0.8], np.float64), [0, 1, 2], [3, 4], [-1, 3, 4, -1, 5, 6, 7])
    keep = []          # the tensors the prepared pointers refer to
    for fam, onehot in (("gamma", False), ("tweedie", False), ("gamma", True), ("tweedie", True)):
        pe = 8 if onehot else p + 1
        H, g, ll, w, st, beta = new(pe, pe), new(pe), new(1), new(n), new(2), dev(np.linspace(-0.3, 0.4, pe))
        scal = ((1.5,) if fam == "tweedie" else ()) + (2.5,)
        if onehot:
            need = getattr(lib, "dlsa_onehot_%s_workspace_bytes" % fam)(plan._h, n, 1)
            fn, head, shape = getattr(lib, "dlsa_onehot_%s_pass_f64" % fam), (plan._h, *engine._oh_args(plan, num, codes)), (n,)
        else:
            need = getattr(lib, "dlsa_%s_workspace_bytes" % fam)(n, p, 1, 1)
            fn, head, shape = getattr(lib, "dlsa_%s_pass_f64" % fam), (engine._ptr(X), X.stride(0)), (n, p, 1)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        keep += [H, g, ll, w, st, beta, ws]
        a = (*head, engine._ptr(y), engine._ptr(off), engine._ptr(beta), *scal, *shape, engine._ptr(H), pe, engine._ptr(g), engine._ptr(ll),
             engine._ptr(w), engine._ptr(st), engine._ptr(ws), need, engine._stream())
        for _ in range(200):
            _lib.check(fn(*a))
        torch.cuda.synchronize()
        us = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn(*a)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / args.calls * 1e6)
        us.sort()
        print(json.dumps({"entry": fn.__name__, "n": n, "pe": pe, "calls": args.calls, "rounds": args.rounds,
                          "us_per_call": round(us[len(us) // 2], 3), "spread_us": [round(us[0], 3), round(us[-1], 3)]}), flush=True)


if __name__ == "__main__":
    main()
