"""Time lars_path with the library named on the command line (A/B of two builds): lars_q.hip at p = 300, lars_c.hip at p = 500 and
2000 (logistic-Hessian-like Sigma, no intercept), lar and lasso, 1 warm-up + 9 timed calls, median.
   python bench/lars_path_time.py dlsa_amd/libdlsa_hip.so"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from dlsa_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from dlsa_amd import engine
for p in (300, 500, 2000):
    rng = np.random.default_rng(p)
    n = 40 * p
    X = rng.random((n, p)) - 0.5
    S = torch.from_numpy(X.T @ ((rng.random(n) * 0.25)[:, None] * X)).cuda()
    b = torch.from_numpy(np.where(np.arange(p) < 0.4 * p, 1.0, 0.0) + 0.05 * rng.standard_normal(p)).cuda()
    out = []
    for typ in ("lar", "lasso"):
        engine.lars_path(S, b, False, float(n), type=typ); torch.cuda.synchronize()
        reps = []
        for _ in range(9):
            t = time.perf_counter(); r = engine.lars_path(S, b, False, float(n), type=typ); torch.cuda.synchronize()
            reps.append((time.perf_counter() - t) * 1e3)
        out.append("%s median %.2f ms (min %.2f, max %.2f; %d steps)" % (typ, float(np.median(reps)), min(reps), max(reps), r["beta"].shape[0] - 1))
    print("%s p=%d: %s" % (os.path.basename(sys.argv[1]), p, "  ".join(out)), flush=True)
