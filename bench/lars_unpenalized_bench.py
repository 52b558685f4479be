"""Timing of dlsa_lars_lsa_f64 with unpenalised leading coefficients.  Calls are timed alternating in one process: 5 rounds of 3
calls each side, each side reports its median round and its run-to-run spread [fastest, slowest] (ms per call; the C entry is
called directly on buffers allocated once, and every call is followed by a stream synchronise, so the finish kernel of u >= 2 is
inside the window).  Prints one JSON line per case:

  parent    u = 0 and u = 1 at m = 100, 500, 2000: this build next to ANOTHER build of the library (--parent PATH, the parent
            commit's libdlsa_hip.so) on the same problem.  "inside" says whether this build's median lies inside the parent's own
            [fastest, slowest]; the outputs of the two builds are compared bit for bit ("same_bits").  Without --parent the leg is
            skipped.
  unpen     u = 7 next to u = 0 on the SAME path (the u = 0 problem is the reduced matrix, formed beforehand on the host by tests/lars_unpenalized_reference.py): a record
            of what the prepare kernel, the V'V term of the prologues and the finish kernel cost.

The problems are tests/lars_problems.py's correlated designs (rho = 0.5, lasso)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dlsa_amd import _lib  # noqa: E402
from gamma_bench import alternating, sides  # noqa: E402
import lars_problems  # noqa: E402
import lars_unpenalized_reference as ur  # noqa: E402

LARS = ("dlsa_lars_workspace_bytes", "dlsa_lars_lsa_f64", "dlsa_last_error")


def other_build(path):
    lib = ctypes.CDLL(path)
    for name in LARS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


class Call:
    """one (library, problem, u): buffers allocated once, run() = one call + synchronise"""

    def __init__(self, lib, S, b, n, u, typ=1):
        self.lib, self.S, self.b, self.n, self.u, self.typ = lib, S, b, float(n), u, typ
        self.p = S.shape[0]
        m = self.p - u
        self.ms = 8 * m
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
        self.out = {"beta": z(self.ms + 1, m), "beta0": z(self.ms + 1, max(1, u)), "AIC": z(self.ms + 1), "BIC": z(self.ms + 1)}
        self.ws = torch.empty(int(lib.dlsa_lars_workspace_bytes(self.p)), dtype=torch.uint8, device="cuda")
        self.steps = ctypes.c_int(0)

    def run(self):
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        o = self.out
        rc = self.lib.dlsa_lars_lsa_f64(P(self.S), self.S.stride(0), P(self.b), self.p, self.u, self.n, self.typ, 2.220446049250313e-16, self.ms,
                                        P(o["beta"]), P(o["beta0"]), P(o["AIC"]), P(o["BIC"]), ctypes.byref(self.steps), P(self.ws),
                                        self.ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()

    def result(self):
        k = self.steps.value
        return {key: t[: k + 1].clone() for key, t in self.out.items()}


def problem(p, seed=3):
    S, b, n = lars_problems.problem(("corr", p, 0.5, seed))
    return torch.from_numpy(S).cuda(), torch.from_numpy(b).cuda(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="another build of libdlsa_hip.so (the parent commit's) for the u <= 1 leg")
    ap.add_argument("--widths", type=int, nargs="*", default=[100, 500, 2000])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    this = _lib.load()
    parent = other_build(a.parent) if a.parent else None
    for m in a.widths:
        if parent is not None:
            for u in (0, 1):
                S, b, n = problem(m + u)
                new, old = Call(this, S, b, n, u), Call(parent, S, b, n, u)
                tn, to = alternating(new.run, old.run, a.reps)
                rn, ro = new.result(), old.result()
                print(json.dumps({"case": "parent", "m": m, "u": u, "steps": new.steps.value, **sides("this", tn, "parent", to),
                                  "inside": bool(to[1] <= tn[0] <= to[2]),
                                  "same_bits": new.steps.value == old.steps.value and all(torch.equal(rn[k], ro[k]) for k in rn)}), flush=True)
        Sh, bh, n = lars_problems.problem(("corr", m + 7, 0.5, 3))
        red, bR, _, _ = ur.reduce(Sh, bh, range(7))          # the same path: the reduced problem (numpy, on the host), handed over as u = 0
        with7 = Call(this, torch.from_numpy(Sh).cuda(), torch.from_numpy(bh).cuda(), n, 7)
        none = Call(this, torch.from_numpy(np.ascontiguousarray(red)).cuda(), torch.from_numpy(np.ascontiguousarray(bR)).cuda(), n, 0)
        t7, t0 = alternating(with7.run, none.run, a.reps)
        print(json.dumps({"case": "unpen", "m": m, "steps_u7": with7.steps.value, "steps_u0": none.steps.value,
                          **sides("u7", t7, "u0", t0), "ms_per_step_u7": round(t7[0] / max(1, with7.steps.value), 5),
                          "ms_per_step_u0": round(t0[0] / max(1, none.steps.value), 5)}), flush=True)


if __name__ == "__main__":
    main()
