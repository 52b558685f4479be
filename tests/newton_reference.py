"""numpy reference of the UNDAMPED Newton iteration (no step halving) on a model's `terms(beta) -> (loglik, g, H)`: what the GPU
fits do as long as no step overshoots, and the count that a halved fit must exceed."""
import numpy as np


def undamped(terms, beta, tol, cap=100):
    """Newton from `beta` with full steps.  Returns (evals, iterates, logliks): iterates[i] is where evaluation i + 1 took place,
    logliks[i] its log-likelihood; evals is the number of evaluations up to the one whose step meets the IRLS stopping rule
    |step|_inf <= tol max(1, |beta|_inf), or None where an evaluation is not finite (the iteration diverged: the lists end
    there) or `cap` evaluations did not suffice."""
    beta = np.array(beta, dtype=np.float64)
    iterates, logliks = [], []
    for it in range(cap):
        ll, g, H = terms(beta)
        iterates.append(beta.copy())
        logliks.append(float(ll))
        if not (np.isfinite(ll) and np.all(np.isfinite(g)) and np.all(np.isfinite(H))):
            return None, iterates, logliks
        step = np.linalg.solve(H, g)
        if np.max(np.abs(step)) <= tol * max(1.0, np.max(np.abs(beta))):
            return it + 1, iterates, logliks
        beta = beta + step
    return None, iterates, logliks


def monotone(logliks):
    """no value drops below its predecessor by more than the fits' overshoot band (1e-12 relative): no step would be halved"""
    return all(b >= a - 1e-12 * abs(a) for a, b in zip(logliks[:-1], logliks[1:]))
