"""An oracle-free certificate for a LARS / lasso path of the LSA objective (dlsa/lsa.py:90-212).

certify(S, b0, intercept, n, type, r, tol) checks a returned path r (beta [K+1, m], beta0, AIC, BIC) against the optimality
conditions of the path, not against another implementation of it: whatever algorithm produced r, the conditions below hold for
the LARS / lasso path and (with the step structure) for nothing else.  Only the problem transform of lsa.py:98-109 is shared with
the reference: the intercept's Schur complement, Sigma_s = |b| Sigma |b| and s = sign(b).  With bs_k = beta_k / |b| the point k
has the correlations c_k = Sigma_s (s - bs_k) and C_k = max |c_k|; the step k goes from point k - 1 to point k.  Residuals are in
units of C_0 (conditions 1-6) or relative to the size of the output (7):

  1. equicorrelation  every j with beta_kj != 0 has |c_kj| = C_k
  2. step support     beta_k - beta_{k-1} is supported inside {j : |c_{k-1,j}| = C_{k-1}}
  3. breakpoint       every point before the last has at least nnz(beta_k) + 1 variables at C_k (a step ends where a variable
                      joins or, for the lasso, leaves; a step that stops short has only its active set there -- one that runs
                      past the breakpoint breaks 1)
  4. lasso sign       for the lasso, sign(beta_kj) = sign(c_kj) on the support (residual |c_kj| where the signs differ)
  5. monotone C       C_k <= C_{k-1}
  6. final point      a path that ends before max_steps ends at C = 0 (with every variable active: beta = b)
  7. derived outputs  RSS, dof = #{|beta| > eps}, AIC, BIC and beta0 recomputed from the returned beta (dlsa_oracle.py:410-420)

c is linear along a segment, so |c_j| <= C inside a segment follows from the endpoints.  A path that goes on after the reference has
'ignored' a machine-singular column (a rank-deficient Sigma past its rank) is outside the certificate's scope: it is not the LARS
path of a nonsingular problem, and only the oracle can be the reference.  (An all-zero column is ignored only where C = 0 already.)
"""
import math

import numpy as np

CONDITIONS = ("equicorrelation", "step_support", "breakpoint", "lasso_sign", "monotone_C", "final_point", "derived")

# Calibration (tests/test_gpu_lars_wide.py prints the worst residual per width class).  The oracle's paths (p <= 300, rho <= 0.98,
# ties, zero columns, tiny b) stay below 1e-14; lars_c.hip / lars.hip on one MI355X at 449 <= m <= 2045 below 6e-14 (all seven
# conditions).  TOL = 1e-10 leaves a margin of over 1000 and still sees a coefficient nudged by 1e-6, a step length scaled by
# 1 +- 1e-6 (test_lars_certificate_cpu.py); TOL_DERIVED = 1e-11 sees beta0, AIC or BIC off by 1e-9.
TOL = 1e-10
TOL_DERIVED = 1e-11


class CertificateError(AssertionError):
    pass


def transform(S, b0, intercept):
    """lsa.py:98-109: (Sigma_s, s, |b|, a12 / a11, beta0_hat) of the penalised variables"""
    S = np.asarray(S, dtype=np.float64)
    b0 = np.asarray(b0, dtype=np.float64).ravel()
    if intercept:
        a11 = S[0, 0]
        a12 = S[1:, 0].copy()
        Sig = S[1:, 1:] - np.outer(a12, a12) / a11
        b = b0[1:]
        g = a12 / a11
        beta0_hat = float(np.dot(a12, b) / a11)
    else:
        Sig, b, g, beta0_hat = S, b0, None, 0.0
    absb = np.abs(b)
    return absb[:, None] * Sig * absb[None, :], np.sign(b), absb, g, beta0_hat


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def certify(S, b0, intercept, n, type, r, tol=TOL, tol_derived=TOL_DERIVED, max_steps=None, eps=np.finfo(float).eps):
    """Worst residual of each condition (dict); raises CertificateError naming the step and the variable when one exceeds tol."""
    Ss, s, absb, g, beta0_hat = transform(S, b0, intercept)
    m = Ss.shape[0]
    beta = np.asarray(_np(r["beta"]), dtype=np.float64)
    K = beta.shape[0] - 1
    if max_steps is None or max_steps <= 0:
        max_steps = 8 * m
    if beta.ndim != 2 or beta.shape[1] != m or K < 0:
        raise CertificateError("beta has shape %s; expected [steps + 1, %d]" % (beta.shape, m))
    if K > max_steps:
        raise CertificateError("%d steps, more than max_steps = %d" % (K, max_steps))
    if not np.all(np.isfinite(beta)):
        k, j = np.argwhere(~np.isfinite(beta))[0]
        raise CertificateError("beta[%d, %d] is not finite" % (k, j))
    if np.any(beta[:, absb == 0] != 0):
        k, j = np.argwhere(beta[:, absb == 0] != 0)[0]
        raise CertificateError("step %d: variable %d has b = 0 but beta != 0" % (k, np.flatnonzero(absb == 0)[j]))
    bs = np.divide(beta, absb, out=np.zeros_like(beta), where=absb > 0)
    if np.any(beta[0] != 0):
        raise CertificateError("point 0: beta is not zero (variable %d)" % int(np.flatnonzero(beta[0])[0]))
    c = (Ss @ s)[None, :] - bs @ Ss                     # c_k = Sigma_s (s - bs_k); Sigma_s is symmetric
    ac = np.abs(c)
    C = ac.max(axis=1)
    C0 = C[0]
    if not C0 > 0:
        raise CertificateError("C_0 = %r: nothing to select" % C0)
    res = dict.fromkeys(CONDITIONS, 0.0)

    def fail(cond, msg):
        raise CertificateError("%s: %s (tol %.1e)" % (cond, msg, tol_derived if cond == "derived" else tol))

    def note(cond, v, k, j, what):
        v = float(v)
        res[cond] = max(res[cond], v)
        if v > (tol_derived if cond == "derived" else tol):
            fail(cond, "%s %.3e at step %d%s" % (what, v, k, "" if j is None else ", variable %d" % j))

    supp = beta != 0
    for k in range(K + 1):
        act = np.flatnonzero(supp[k])
        # 1: every variable of the support is at C_k
        if act.size:
            d = (C[k] - ac[k, act]) / C0
            i = int(np.argmax(d))
            note("equicorrelation", d[i], k, int(act[i]), "|c_j| below C_k by")
        # 4: the lasso's coefficients carry the signs of their correlations
        if type == "lasso" and act.size:
            bad = np.sign(beta[k, act]) != np.sign(c[k, act])
            if bad.any():
                d = np.where(bad, ac[k, act], 0.0) / C0
                i = int(np.argmax(d))
                note("lasso_sign", d[i], k, int(act[i]), "sign(beta_j) != sign(c_j) with |c_j| / C_0 =")
        if k == 0:
            continue
        # 2: the step moved only variables that were at C_{k-1}
        mov = np.flatnonzero(beta[k] != beta[k - 1])
        if mov.size:
            d = (C[k - 1] - ac[k - 1, mov]) / C0
            i = int(np.argmax(d))
            note("step_support", d[i], k, int(mov[i]), "moved a variable below C_{k-1} by")
        # 5: C does not increase
        note("monotone_C", (C[k] - C[k - 1]) / C0, k, None, "C_k - C_{k-1} =")
    # 3: a step ends at a breakpoint: the (nnz + 1)-th largest |c| is at C_k
    for k in range(K):
        nz = int(supp[k].sum())
        if nz + 1 > m:
            fail("breakpoint", "step %d: all %d variables are active before the last point" % (k, m))
        kth = np.partition(-ac[k], nz)[nz] * -1.0
        d = (C[k] - kth) / C0
        if d > tol:
            cand = np.flatnonzero(~supp[k])
            j = int(cand[np.argmax(ac[k, cand])]) if cand.size else -1
            note("breakpoint", d, k, j, "fewer than nnz + 1 variables at C_k: the next one (variable %d) is below by" % j)
        res["breakpoint"] = max(res["breakpoint"], float(d))
    # 6: a path that stops before max_steps (every variable active, or nothing left to add) ends at C = 0
    if K < max_steps or supp[K].all():
        note("final_point", C[K] / C0, K, None, "the path ends with C_last / C_0 =")
    # 7: RSS, dof, AIC, BIC and beta0 from the returned beta (lsa.py:191-209)
    dff = s[None, :] - bs
    RSS = np.einsum("ki,ki->k", dff, c)              # (s - bs)' Sigma_s (s - bs)
    dof = np.sum(np.abs(beta) > eps, axis=1)
    for key, want in (("AIC", RSS + 2 * dof), ("BIC", RSS + math.log(n) * dof)):
        got = np.asarray(_np(r[key]), dtype=np.float64).ravel()
        if got.shape != want.shape:
            fail("derived", "%s has %d points, beta %d" % (key, got.size, want.size))
        scale = max(float(np.max(np.abs(want))), float(np.max(np.abs(RSS))), 1e-300)
        d = np.abs(got - want) / scale
        i = int(np.argmax(d))
        note("derived", d[i], i, None, "%s differs from RSS + penalty x dof (dof %d) by" % (key, dof[i]))
    if "beta0" in r:
        got = np.asarray(_np(r["beta0"]), dtype=np.float64).ravel()
        want = beta0_hat - beta @ g if intercept else np.zeros(K + 1)
        if got.shape != want.shape:
            fail("derived", "beta0 has %d points, beta %d" % (got.size, want.size))
        scale = max(float(np.max(np.abs(want))), abs(beta0_hat), 1e-300) if intercept else 1.0
        d = np.abs(got - want) / scale
        i = int(np.argmax(d))
        note("derived", d[i], i, None, "beta0 differs from beta0_hat - beta a12 / a11 by")
    return res
