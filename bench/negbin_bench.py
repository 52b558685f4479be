"""Timing of the negative-binomial map step (csrc/negbin.hip) next to the Poisson one on the same rows.  Prints one JSON line per case:
  pass    the NB pass alone (w, mu, g, row log-likelihood) next to dlsa_poisson_pass_f64, alternating in one call (medians), with the
          algorithmic bandwidth of one read of the rows (8 p bytes per row); expectation: ratio <= 1.15;
  theta   the pass entry with the dispersion terms at p and over a one-column design (8 bytes per row of rows next to the theta step's
          own 16): an upper bound of one theta evaluation's time and a lower bound of its bandwidth;
  eval    a Newton evaluation (pass + H + the Cholesky solve) next to the Poisson evaluation, alternating;
  fit     a whole fit with an intercept and offsets (one partition) next to the Poisson fit of the same rows and to the NB fit at
          the fixed alpha-hat: times, row passes, and the share of the fit the theta iterations take at most (1 - fixed / estimated).
With --structured (a leg of its own; the plain run stays as it is) the structured one-hot path (csrc/onehot_negbin.hip) on
bench/surrogates.airline_shaped rows (p = 260) with NB2 counts (alpha = 0.5, exposure ~ U(0.5, 2)), every pair alternating in one
process, medians of five:
  oh_pass   the structured NB pass next to the structured Poisson pass on the same rows (under rocprofv3 --kernel-trace --stats:
            oh_row_kernel<OhNbRow<true>> against oh_row_kernel<OhPoisRow<true>>);
  oh_newton a structured Newton evaluation (pass + H) next to the structured Poisson evaluation;
  oh_fit    the structured fit of 1e6-row i % K partitions next to the dense NB2 fit of the same partitions on the built matrix
            (build time reported separately; condition: structured <= dense + build), with the peak device memory of both.
Without --case every case runs in a child process of its own under its own time limit, one after another; the first failure
stops the run.  Run one case under rocprofv3 --kernel-trace --stats for the per-kernel split."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHA = 0.5


def timed(fn, reps):
    import torch
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


def data(n, p, seed=321, intercept=0.2):
    """synth rows, beta* = 0.5 on the first 40 % of the columns, offsets log U(0.5, 2), counts Poisson(mu G) with G ~ Gamma(2, 1/2)
    (the sum of two exponentials, drawn on the device): NB2 with alpha = 0.5"""
    import torch
    from dlsa_amd import engine
    X, _ = engine.synth(seed, 0, n, p, labels=False)
    beta = torch.zeros(p, dtype=torch.float64, device="cuda")
    beta[: int(0.4 * p)] = 0.5
    g = torch.Generator(device="cuda").manual_seed(9)
    o = torch.log(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5)
    u = torch.rand((2, n), dtype=torch.float64, device="cuda", generator=g).clamp_min_(1e-300)
    mix = -ALPHA * (torch.log(u[0]) + torch.log(u[1]))
    y = torch.poisson(torch.exp(X @ beta + intercept + o) * mix, generator=g)
    return X, y, o, beta


def pass_case(n, p, reps):
    from dlsa_amd import engine
    X, y, o, beta = data(n, p)
    b = beta * 0.5
    t_nb, t_po = alternating(lambda: engine.negbin_pass(X, y, b, ALPHA, offset=o, want_H=False, want_w=True),
                             lambda: engine.poisson_pass(X, y, b, offset=o, want_H=False, want_w=True), reps)
    gb = 8.0 * n * p
    return {"case": "pass", "n": n, "p": p, "negbin_ms": round(t_nb, 3), "poisson_ms": round(t_po, 3), "ratio": round(t_nb / t_po, 3),
            "expected_ratio": 1.15, "met": bool(t_nb / t_po <= 1.15), "negbin_TBps": round(gb / (t_nb * 1e-3) / 1e12, 3),
            "poisson_TBps": round(gb / (t_po * 1e-3) / 1e12, 3),
            "note": "both passes include their beta-free reduction (lgamma(y+1); c(theta) with lgamma(y+1))"}


def theta_case(n, p, reps):
    import torch
    from dlsa_amd import engine
    X, y, o, beta = data(n, p)
    b = beta * 0.5
    # the pass entry returns the full log-likelihood, so it runs negbin_kernel + one theta evaluation (with lgamma(y + 1))
    with_t = lambda: engine.negbin_pass(X, y, b, ALPHA, offset=o, want_H=False, want_w=True, want_theta=True)
    t_with = timed(with_t, reps)
    del X
    torch.cuda.empty_cache()
    # nearly alone: over a one-column design the row pass reads 8 bytes per row, less than the theta step's own 16
    X1 = y.reshape(-1, 1).contiguous() * 0.0
    b1 = torch.zeros(1, dtype=torch.float64, device="cuda")
    t_small = timed(lambda: engine.negbin_pass(X1, y, b1, ALPHA, offset=o, want_H=False, want_w=True, want_theta=True), reps * 2)
    return {"case": "theta", "n": n, "p": p, "pass_with_theta_ms": round(t_with, 3), "p1_pass_with_theta_ms": round(t_small, 3),
            "theta_upper_bound_TBps": round(16.0 * n / (t_small * 1e-3) / 1e12, 3),
            "note": "p1 = row pass over one column + theta evaluation + finish launches: an upper bound of the theta step's time"}


def eval_case(n, p, reps):
    from dlsa_amd import engine
    X, y, o, beta = data(n, p)
    b = beta * 0.5

    def nb():
        H, g = engine.negbin_pass(X, y, b, ALPHA, offset=o)[:2]
        engine.spd_solve(H, g)

    def po():
        H, g = engine.poisson_pass(X, y, b, offset=o)[:2]
        engine.spd_solve(H, g)
    t_nb, t_po = alternating(nb, po, reps)
    return {"case": "eval", "n": n, "p": p, "negbin_eval_ms": round(t_nb, 3), "poisson_eval_ms": round(t_po, 3), "ratio": round(t_nb / t_po, 3)}


def fit_case(n, p, reps):
    import torch
    import dlsa_amd
    X, y, o, _ = data(n, p)

    def wall(fn):
        mb = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            mb = fn()
        torch.cuda.synchronize()
        return mb, (time.perf_counter() - t0) * 1e3 / reps
    nb, t_nb = wall(lambda: dlsa_amd.fit_negbin_partitions(X, y, fit_intercept=True, offset=o))
    po, t_po = wall(lambda: dlsa_amd.fit_poisson_partitions(X, y, fit_intercept=True, offset=o))
    fx, t_fx = wall(lambda: dlsa_amd.fit_negbin_partitions(X, y, fit_intercept=True, offset=o, alpha=nb.extra["alpha"][0]))
    return {"case": "fit", "n": n, "p": p, "negbin_fit_ms": round(t_nb, 2), "poisson_fit_ms": round(t_po, 2),
            "negbin_fixed_alpha_fit_ms": round(t_fx, 2), "negbin_row_passes": nb.n_iter[0], "poisson_row_passes": po.n_iter[0],
            "fixed_alpha_row_passes": fx.n_iter[0], "alpha_hat": nb.extra["alpha"][0], "pearson_over_n": nb.extra["pearson"][0] / n,
            "theta_share_upper_bound": round(max(0.0, 1.0 - t_fx / t_nb), 3), "status_ok": nb.status == [0] and po.status == [0]}


def airline_negbin(n, seed=7):
    """airline_shaped rows with counts y ~ Poisson(exposure * exp(eta) * G) from its beta, G ~ Gamma(2, 1/2) as in data():
    NB2 with alpha = 0.5, exposure ~ U(0.5, 2)"""
    import torch
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
    u = torch.rand((2, n), dtype=torch.float64, device="cuda", generator=g).clamp_min_(1e-300)
    mix = -ALPHA * (torch.log(u[0]) + torch.log(u[1]))
    d["counts"] = torch.poisson(torch.exp(eta + o) * mix, generator=g)
    d["offset"] = o
    del d["y"]
    return d


def oh_pass_case(n, p, reps):
    from dlsa_amd import engine
    d = airline_negbin(n)
    plan, num, codes, y, o = d["plan"], d["num"], d["codes"], d["counts"], d["offset"]
    b = d["beta"] * 0.5
    q, f = num.shape[1], codes.shape[1]
    # (the NB entry's full log-likelihood costs a theta evaluation on top of the row pass; the kernel pair is read off the trace)
    t_nb, t_po = alternating(lambda: engine.onehot_negbin_pass(plan, num, codes, y, b, ALPHA, offset=o, want_H=False, want_w=True),
                             lambda: engine.onehot_poisson_pass(plan, num, codes, y, b, offset=o, want_H=False, want_w=True), reps * 4)
    bn, bp = 8 * q + 4 * f + 32, 8 * q + 4 * f + 24
    return {"case": "oh_pass", "n": n, "p": d["p"], "negbin_ms": round(t_nb, 4), "poisson_ms": round(t_po, 4),
            "ratio": round(t_nb / t_po, 3), "bytes_ratio": round(bn / bp, 3),
            "note": "entries, each with its beta-free reduction; the kernel pair: rocprofv3 --kernel-trace --stats"}


def oh_newton_case(n, p, reps):
    from dlsa_amd import engine
    d = airline_negbin(n)
    plan, num, codes, y, o = d["plan"], d["num"], d["codes"], d["counts"], d["offset"]
    b = d["beta"] * 0.5
    t_nb, t_po = alternating(lambda: engine.onehot_negbin_pass(plan, num, codes, y, b, ALPHA, offset=o),
                             lambda: engine.onehot_poisson_pass(plan, num, codes, y, b, offset=o), reps * 2)
    return {"case": "oh_newton", "n": n, "p": d["p"], "negbin_eval_ms": round(t_nb, 4), "poisson_eval_ms": round(t_po, 4),
            "ratio": round(t_nb / t_po, 3)}


def oh_fit_case(n, p, reps):
    import torch
    from dlsa_amd import engine
    K = max(1, n // 1_000_000)
    d = airline_negbin(n)
    plan, num, codes, y, o = d["plan"], d["num"], d["codes"], d["counts"], d["offset"]
    first, rows = list(range(K)), [len(range(k, n, K)) for k in range(K)]
    raw = num.numel() * 8 + codes.numel() * 4 + y.numel() * 8 + o.numel() * 8

    def fresh():
        torch.cuda.synchronize()
        engine.release_workspace()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3 / reps
    structured = lambda: engine.onehot_negbin_fit_ex(plan, num, codes, y, first, rows, row_step=K, offset=o)
    fresh()
    rs = structured()
    torch.cuda.synchronize()
    peak_s = torch.cuda.max_memory_allocated()
    fresh()
    t0 = time.perf_counter()
    X, _ = engine.design(num, codes, *d["spec"])
    torch.cuda.synchronize()
    t_build = (time.perf_counter() - t0) * 1e3
    dense = lambda: engine.negbin_fit_ex(X, y, first, rows, row_step=K, offset=o)
    rd = dense()
    torch.cuda.synchronize()
    peak_d = torch.cuda.max_memory_allocated()
    ts, td = [], []
    for _ in range(5):                       # the pair in turns, in this process: medians of five
        ts.append(wall(structured)[1])
        td.append(wall(dense)[1])
    rs, rd = structured(), dense()
    t_s, t_d = sorted(ts)[2], sorted(td)[2]
    gap = float((rs["coef"] - rd["coef"]).abs().max() / rd["coef"].abs().max())
    return {"case": "oh_fit", "n": n, "p": d["p"], "partitions": K, "structured_fit_ms": round(t_s, 2), "dense_fit_ms": round(t_d, 2),
            "dense_build_ms": round(t_build, 2), "ratio_vs_dense_plus_build": round(t_s / (t_d + t_build), 3),
            "ratio_vs_dense_fit": round(t_s / t_d, 3), "not_slower": bool(t_s <= t_d + t_build),
            "iters_structured": rs["n_iter"][:4], "iters_dense": rd["n_iter"][:4], "alpha_hat": rs["alpha"][:4],
            "status_ok": all(s == 0 for s in rs["status"]) and all(s == 0 for s in rd["status"]), "coef_rel_gap": gap,
            "raw_GB": round(raw / 1e9, 3), "structured_peak_GB": round(peak_s / 1e9, 3), "dense_peak_GB": round(peak_d / 1e9, 3),
            "structured_peak_below_raw_plus_1GB": bool(peak_s < raw + 1e9)}


CASES = {"pass": pass_case, "theta": theta_case, "eval": eval_case, "fit": fit_case, "oh_pass": oh_pass_case, "oh_newton": oh_newton_case,
         "oh_fit": oh_fit_case}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1e6 x 100 only (a quick check)")
    ap.add_argument("--case", choices=sorted(CASES), help="run this case in this process")
    ap.add_argument("--structured", action="store_true", help="the structured one-hot leg only (airline-shaped rows, p = 260)")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--p", type=int, default=100)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process, seconds")
    a = ap.parse_args()
    if a.case:
        reps = max(1, a.reps // 2) if a.case in ("fit", "oh_fit") else a.reps
        print(json.dumps(CASES[a.case](a.n, a.p, reps)), flush=True)
        return 0
    shapes = [(1_000_000, 100)] if a.small else [(10_000_000, 100), (2_000_000, 500)]
    jobs = [(c, n, p) for n, p in shapes for c in ("pass", "theta", "eval")] + [("fit", shapes[0][0], shapes[0][1])]
    if a.structured:
        jobs = [("oh_pass", 1_000_000, 260), ("oh_newton", 1_000_000, 260), ("oh_fit", 1_000_000 if a.small else 4_000_000, 260)]
    for c, n, p in jobs:             # a fresh child per case, each under its own time limit; nothing more after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", c, "--n", str(n), "--p", str(p),
               "--reps", str(a.reps)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(json.dumps({"case": c, "n": n, "p": p, "failed_with_exit_status": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
