"""LARS path of the least-squares approximation -- host mirror of the reference's dlsa/lsa.py.

`lars_lsa` keeps the reference's signature and result keys (lsa.py:90-212) and runs the whole
path in the HIP engine's persistent LARS kernel.  Inputs may be numpy arrays / np.matrix /
pandas objects / torch tensors; outputs are numpy arrays (`beta` is (steps+1) x m).
Differences from the reference as shipped: plain ndarrays are accepted
(D2), the intercept branch indexes by the matrix dimension and uses `n` only inside log(n) (D4).
Beyond the reference: `unpenalized` names any coefficients that are not to be shrunk (the J
intercepts of a multinomial block, a treatment indicator, the controls).
"""
import numpy as np
import torch

from . import engine


def _dev(a):
    if isinstance(a, torch.Tensor):
        return a.to(device="cuda", dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def unpenalized_order(unpenalized, p, intercept=False):
    """(U, perm) for `unpenalized`, a sequence of distinct indices into the p coefficients: U as a list of ints in the order given,
    perm = U followed by the remaining indices in their original order -- the order in which the engine takes the coefficients
    (its unpenalised ones lead).  Raises ValueError, before any GPU work, for an index that is not a whole number in [0, p), a
    duplicate, more than engine.LARS_MAX_UNPENALIZED indices, none left to penalise, or `intercept` given as well."""
    if intercept:
        raise ValueError("lars_lsa: give the unpenalised coefficients either as intercept=True or as unpenalized=[...], not both")
    U = []
    for v in unpenalized:
        i = int(v)
        if i != v or not 0 <= i < p:
            raise ValueError("lars_lsa: unpenalized index %r is not a whole number in [0, %d)" % (v, p))
        U.append(i)
    if len(set(U)) != len(U):
        raise ValueError("lars_lsa: unpenalized indices must be distinct, got %r" % (U,))
    if len(U) > engine.LARS_MAX_UNPENALIZED:
        raise ValueError("lars_lsa: %d unpenalized coefficients, at most %d" % (len(U), engine.LARS_MAX_UNPENALIZED))
    if len(U) >= p:
        raise ValueError("lars_lsa: %d unpenalized coefficients leave nothing to select among p = %d" % (len(U), p))
    chosen = set(U)
    return U, U + [j for j in range(p) if j not in chosen]


def lars_path_device(Sigma0, b0, intercept, n, type="lar", eps=np.finfo(float).eps, max_steps=None, unpenalized=None):
    """Device-tensor variant: returns dict of cuda tensors (no host copy of the path).

    `unpenalized` (a sequence of distinct indices into b0, any positions) asks for a path that shrinks every coefficient but
    these: (Sigma0, b0) are gathered on the device so that they lead and the engine is called with their count.  The result then
    holds `beta` [steps+1, p-u] over the remaining coordinates in their original order, `beta0` [steps+1, u] in the order given
    (b0[unpenalized] not included, as for the reference's intercept) and `theta` [steps+1, p], the whole coefficient path in the
    caller's order with b0[unpenalized] + beta0 at the unpenalised positions."""
    if unpenalized is not None:
        p = int(Sigma0.shape[0]) if hasattr(Sigma0, "shape") else len(Sigma0)
        U, perm = unpenalized_order(unpenalized, p, intercept)       # refusals first: nothing has touched the GPU yet
    S = _dev(Sigma0)
    b = _dev(b0).reshape(-1)
    if S.dim() != 2 or S.shape[0] != S.shape[1] or S.shape[0] != b.shape[0]:
        raise ValueError("Sigma0 must be p x p and b0 of length p")
    if unpenalized is None:
        return engine.lars_path(S, b, bool(intercept), float(n), type=type, eps=float(eps), max_steps=max_steps)
    u = len(U)
    idx = torch.tensor(perm, dtype=torch.int64, device=S.device)
    Sp, bp = S.index_select(0, idx).index_select(1, idx).contiguous(), b.index_select(0, idx).contiguous()      # a gather: no arithmetic
    r = engine.lars_path(Sp, bp, u, float(n), type=type, eps=float(eps), max_steps=max_steps)
    beta0 = r["beta0"].reshape(-1, u) if u else r["beta0"].new_zeros((r["beta0"].shape[0], 0))
    theta = torch.empty((r["beta"].shape[0], p), dtype=torch.float64, device=S.device)
    theta[:, idx[u:]] = r["beta"]
    if u:
        theta[:, idx[:u]] = beta0 + bp[:u]
    return {"AIC": r["AIC"], "BIC": r["BIC"], "beta": r["beta"], "beta0": beta0, "theta": theta}


def lars_lsa(Sigma0, b0, intercept, n, type="lar", eps=np.finfo(float).eps, max_steps=None, unpenalized=None):
    """Compute the Least Angle Regression or Lasso path of the LSA objective (lsa.py:90-212).
    Returns {'AIC', 'BIC', 'beta', 'beta0'}; with `unpenalized` (see lars_path_device) also 'theta'."""
    r = lars_path_device(Sigma0, b0, intercept, n, type=type, eps=eps, max_steps=max_steps, unpenalized=unpenalized)
    return {k: v.cpu().numpy() for k, v in r.items()}
