"""Reference, designs and bounds for the logistic row terms (csrc/logistic.h and its copies in irls_pass.hip / onehot.hip):
e = exp(-|eta|), mu = sigmoid(eta), w = e / (1 + e)^2, softplus(eta) = max(eta, 0) + log1p(e), over the WHOLE range of eta.

* terms(eta): the textbook forms in mpmath at 50 digits, cached per grid.
* Design: rows with ONE nonzero entry and beta = +-1 (alternating), so that eta_i is known exactly in every kernel whatever
  its summation order -- clamped columns and the phantom column of packed odd-p rows meet beta = 0, added zeros are exact.
  With the implicit intercept b0, x_i = eta_i - b0 and the reference takes eta_i := fl(b0 + x_i), which is what one fp64
  addition gives.  Rows are permuted (the neighbours of a batch or chunk carry unrelated eta) and columns 0 and p - 1 always
  receive some of the largest |eta|.
* Bounds (u = 2^-53, sp(v) = np.spacing(|v|), subnormals included, sp(0) = 5e-324):
    per row  |w - w*| <= B_w sp(w*), B_w = max(4, 2 E_w), E_w the worst ulp error of the PLAIN fp64 evaluation (numpy's
             exp / log1p / division) against the 50-digit values on the same grid -- the convention of test_special_functions;
             the factor 2 is for an algorithm of the same accuracy class with different roundings.  B_mu, B_sp alike.
    any sum  S = sum t_i of m nonzero terms in any order: |S - S*| <= sum delta_i + 2 (m + 2) u sum |t_i*|, with
             H_jj, t = w x^2:            delta = B_w sp(w*) x^2 + 2 sp(t*)
             g_j,  t = (y - mu) x:       delta = |x| (B_mu sp(mu*) + y u) + sp(t*)
             l,    t = y eta - softplus: delta = B_sp sp(softplus*) + y sp(eta) + sp(t*)
  The y u and y sp(eta) terms are the floor of the FORMULATION y - mu and y eta - softplus: 1 - mu cannot be better than an
  ulp of 1 once mu is rounded, eta - softplus(eta) not better than an ulp of eta.  The reference project computes the same
  differences and has the same floor; the kernels are not to be changed for it.
No row, column or regime is left out of any check."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

U = 2.0 ** -53
DPS = 50


def sp(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------ grids
BRANCH_POINTS = (0.881373587019543, 36.04, 36.8, 708.4, 744.44, 745.13, 745.2, 746.0, 800.0, 1e6)
REGIMES = (-745.0, -720.0, -700.0, -400.0, -100.0, -37.5, -36.0, -20.0, -5.0, -0.88, "tiny", 0.88, 5.0, 20.0, 36.0, 37.5, 100.0,
           400.0, 700.0, 720.0, 745.0, 1e6)
REGIME_POINTS = 257


@functools.lru_cache(maxsize=None)
def full_grid():
    """~4100 eta: a sweep of [-760, 760], a random fill of [-40, 40], +-10^k for k = -300 .. 0, +-0, +-5e-324 and the branch
    and range points of logistic.h."""
    rng = np.random.default_rng(20240607)
    pw = 10.0 ** np.arange(-300, 1, dtype=np.float64)
    bp = np.array(BRANCH_POINTS)
    g = np.concatenate([np.linspace(-760.0, 760.0, 2001), rng.uniform(-40.0, 40.0, 1473), pw, -pw,
                        [0.0, -0.0, 5e-324, -5e-324], bp, -bp])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def regime_grid(c):
    if c == "tiny":
        g = 10.0 ** np.linspace(-8.0, -300.0, REGIME_POINTS) * np.where(np.arange(REGIME_POINTS) % 2 == 0, 1.0, -1.0)
    else:
        g = float(c) + np.linspace(-0.5, 0.5, REGIME_POINTS)
    g.setflags(write=False)
    return g


def grid(name):
    return full_grid() if name == "full" else regime_grid(name)


def regime_centre(c):
    return 0.0 if c in ("tiny", "full") else float(c)


# ------------------------------------------------------------------------------------------------ reference
class Terms:
    """50-digit values at the points eta[k]: lists of mpf (e, mu, w, l1p, sp) and their fp64 roundings (arrays .f_*)."""

    def __init__(self, eta):
        self.eta = np.array(eta, dtype=np.float64)
        with mpmath.workdps(DPS):
            self.e, self.mu, self.w, self.l1p, self.sp = [], [], [], [], []
            for v in self.eta:
                x = mpmath.mpf(float(v))
                e = mpmath.exp(-abs(x))
                self.e.append(e)
                self.mu.append(1 / (1 + e) if v >= 0 else e / (1 + e))
                self.w.append(e / (1 + e) ** 2)
                l = mpmath.log1p(e)
                self.l1p.append(l)
                self.sp.append((x if v > 0 else 0) + l)
        for name in ("e", "mu", "w", "l1p", "sp"):
            setattr(self, "f_" + name, np.array([float(t) for t in getattr(self, name)]))


_terms_cache = {}


def terms(eta):
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    key = eta.tobytes()
    if key not in _terms_cache:
        _terms_cache[key] = Terms(eta)
    return _terms_cache[key]


def ulp_errors(got, ref_mp, ref_f):
    """|got - ref| / sp(ref) per point, the difference formed at 50 digits (exact down to the subnormals)."""
    got = np.asarray(got, dtype=np.float64)
    s = sp(ref_f)
    out = np.empty(got.shape)
    with mpmath.workdps(DPS):
        for i in range(got.size):
            g = float(got[i])
            out[i] = float(abs(mpmath.mpf(g) - ref_mp[i]) / mpmath.mpf(float(s[i]))) if math.isfinite(g) else math.inf
    return out


def plain_terms(eta, mutant=None):
    """The plain fp64 evaluation (numpy's exp, log1p, division), or one of the mutants the checkers must reject."""
    eta = np.asarray(eta, dtype=np.float64)
    a = np.abs(eta)
    if mutant == "clamp700":
        a = np.minimum(a, 700.0)
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp(-a.astype(np.float32)).astype(np.float64) if mutant == "exp_fp32" else np.exp(-a)
        if mutant == "flush_subnormal":
            e = np.where(e < 2.2250738585072014e-308, 0.0, e)
        inv = 1.0 / (1.0 + e)
        mu = inv if mutant == "mu_of_positive" else np.where(eta >= 0, inv, e * inv)
        w = mu * (1.0 - mu) if mutant == "w_mu_1_minus_mu" else e / (1.0 + e) ** 2
        if mutant == "log_1_plus_e":
            l1p = np.log(1.0 + e)
        elif mutant == "branch_at_half":
            # logistic.h's log: t = 1 + e halved above the switch, + ln 2 where halved -- the halving moved to e > 0.5, the ln 2 not
            half = e > 0.5
            l1p = np.where(half, np.log1p(0.5 * e - 0.5), np.log1p(e)) + np.where(e > 0.41421356237309503, math.log(2.0), 0.0)
        else:
            l1p = np.log1p(e)
        soft = np.maximum(eta, 0.0) + l1p
    return {"e": e, "mu": mu, "w": w, "l1p": l1p, "sp": soft}


# ------------------------------------------------------------------------------------------------ logistic.h, emulated
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))        # one rounding (int / int division is correctly rounded)


def _rcp_newton(d):
    x = float(np.float32(1.0 / d))                               # the hardware seed, modelled as the fp32-rounded reciprocal
    x = _fma(_fma(-d, x, 1.0), x, x)
    x = _fma(_fma(-d, x, 1.0), x, x)
    return x


_EXP_C = (2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05,
          1.984126984126984e-04, 1.388888888888889e-03, 8.333333333333333e-03, 4.1666666666666664e-02, 1.6666666666666666e-01,
          0.5, 1.0, 1.0)
_LOG_C = tuple(1.0 / k for k in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0)) + (1.0,)


def _emulate_one(eta):
    a = min(abs(eta), 745.2)
    kf = float(np.rint(a * 1.4426950408889634))
    r = _fma(kf, 6.93147180369123816490e-01, -a)
    r = _fma(kf, 1.90821492927058770002e-10, r)
    q = 1.6059043836821613e-10
    for c in _EXP_C:
        q = _fma(q, r, c)
    e = math.ldexp(q, -int(kf))
    inv = _rcp_newton(1.0 + e)
    mu = inv if eta >= 0.0 else e * inv
    w = e * inv * inv
    big = e > 0.41421356237309503
    num = _fma(0.5, e, -0.5) if big else e
    den = _fma(0.5, e, 1.5) if big else 2.0 + e
    sv = num * _rcp_newton(den)
    z = sv * sv
    q = 1.0 / 21.0
    for c in _LOG_C:
        q = _fma(q, z, c)
    l1p = _fma(2.0 * sv, q, 6.931471805599453094e-01 if big else 0.0)
    return e, mu, w, l1p, max(eta, 0.0) + l1p


def emulate_logistic_h(eta):
    """csrc/logistic.h operation by operation: exact fma through fractions.Fraction, plain IEEE products and sums."""
    rows = [_emulate_one(float(v)) for v in np.asarray(eta, dtype=np.float64).ravel()]
    cols = np.array(rows, dtype=np.float64).reshape(-1, 5)
    return {"e": cols[:, 0], "mu": cols[:, 1], "w": cols[:, 2], "l1p": cols[:, 3], "sp": cols[:, 4]}


# ------------------------------------------------------------------------------------------------ bounds
class Bounds:
    """E_* = the plain evaluation's worst ulp error on the grid, B_* = max(4, 2 E_*)."""

    def __init__(self, name):
        g = grid(name)
        t = terms(g)
        pl = plain_terms(g)
        self.name = name
        self.E = {}
        for key, mp_list, f in (("w", t.w, t.f_w), ("mu", t.mu, t.f_mu), ("sp", t.sp, t.f_sp)):
            self.E[key] = float(np.max(ulp_errors(pl[key], mp_list, f)))
        self.B = {k: max(4.0, 2.0 * v) for k, v in self.E.items()}

    def __repr__(self):
        return "E_w %.2f E_mu %.2f E_sp %.2f" % (self.E["w"], self.E["mu"], self.E["sp"])


@functools.lru_cache(maxsize=None)
def bounds(name):
    """The B_* of the checks on grid `name` ("full" or a regime's centre), measured on that grid."""
    return Bounds(name)


# ------------------------------------------------------------------------------------------------ designs
class Design:
    """n rows over p columns, one nonzero each: row i carries grid point k_i in column col[k_i]; the tile index i // G decides
    y, so every eta meets both labels; rows permuted with a fixed seed.  b0: the implicit intercept (x = eta - b0)."""

    def __init__(self, name, n, p, b0=None, seed=7):
        g = grid(name)
        G = g.size
        self.name, self.n, self.p, self.b0, self.G = name, int(n), int(p), b0, G
        rng = np.random.default_rng(seed + 1000 * p + n)
        col = rng.integers(0, p, G)
        order = np.argsort(-np.abs(g), kind="stable")
        col[order[0]] = 0; col[order[2 % G]] = 0
        col[order[1 % G]] = p - 1; col[order[3 % G]] = p - 1
        self.col_k = col
        self.beta = np.where(np.arange(p) % 2 == 0, 1.0, -1.0)
        self.dot_k = (g - b0) if b0 is not None else g.copy()              # x_i beta_c(i): what the row's dot product is, exactly
        self.x_k = self.dot_k * self.beta[col]
        i = np.arange(self.n)
        perm = rng.permutation(self.n)
        self.k = rng.permutation(G)[i % G][perm]                           # (n < G: a random subset of the grid, not its first points)
        self.y = ((i // G) % 2).astype(np.float64)[perm]
        self.col = col[self.k]
        self.x = self.x_k[self.k]

    def eta_k(self, scale=1.0, b0=None):
        """fl(b0 + scale * dot) per grid point (scale a power of two: the product is exact)."""
        b0 = self.b0 if b0 is None else b0
        d = scale * self.dot_k
        return d + b0 if b0 is not None else d

    def eta(self):
        return self.eta_k()[self.k]

    def dense(self):
        X = np.zeros((self.n, self.p))
        X[np.arange(self.n), self.col] = self.x
        return X

    def beta_full(self):
        return np.concatenate([[self.b0], self.beta]) if self.b0 is not None else self.beta

    def counts(self, rows=None):
        """multiplicity of (grid point, label) among the rows: [G, 2]"""
        k, y = (self.k, self.y) if rows is None else (self.k[rows], self.y[rows])
        return np.bincount(2 * k + y.astype(np.int64), minlength=2 * self.G).reshape(self.G, 2)


class GatherDesign:
    """A pure gather (the one-hot pass with one factor and no numeric column): row i has level k_i, whose coefficient IS its eta;
    column k of g collects the residuals of level k with x = 1.  Serves check_rows / check_sums like a Design."""

    def __init__(self, name, eta_levels, k, y):
        self.name, self.b0 = name, None
        self._eta_k = np.ascontiguousarray(eta_levels, dtype=np.float64)
        self.G = self.p = self._eta_k.size
        self.k, self.y, self.n = np.asarray(k, dtype=np.int64), np.asarray(y, dtype=np.float64), len(k)
        self.col_k, self.beta, self.dot_k = np.arange(self.G), np.ones(self.G), np.ones(self.G)
        self.col, self.x = self.k, np.ones(self.n)

    def eta_k(self, scale=1.0, b0=None):
        return self._eta_k

    def eta(self):
        return self._eta_k[self.k]

    counts = Design.counts


# ------------------------------------------------------------------------------------------------ checkers
def check_rows(got, key, eta_rows, bounds, what=""):
    """per-row values of w / mu / sp at the rows' eta against B sp(ref); returns (worst ulp, eta there).  Rows that carry the
    same (eta, value) bit patterns are checked once."""
    eta_rows = np.ascontiguousarray(eta_rows, dtype=np.float64)
    got = np.ascontiguousarray(got, dtype=np.float64)
    assert got.shape == eta_rows.shape, (what, got.shape, eta_rows.shape)
    pairs = np.unique(np.stack([eta_rows.view(np.int64), got.view(np.int64)], 1), axis=0)      # by bit pattern: +-0 stay apart
    eta_u, got_u = pairs[:, 0].copy().view(np.float64), pairs[:, 1].copy().view(np.float64)
    uniq, inv = np.unique(pairs[:, 0], return_inverse=True)
    t = terms(uniq.view(np.float64))
    mp_list, f = getattr(t, key), getattr(t, "f_" + key)
    err = ulp_errors(got_u, [mp_list[j] for j in inv], f[inv])
    worst = int(np.argmax(err))
    print("%s: %s worst %.3f ulp at eta = %r (bound %.2f)" % (what, key, err[worst], float(eta_u[worst]), bounds.B[key]))
    assert err[worst] <= bounds.B[key], (what, key, float(err[worst]), float(eta_u[worst]), float(got_u[worst]))
    return float(err[worst]), float(eta_u[worst])


_point_cache = {}


def _point_terms(eta_k, dot_k, B):
    """Per grid point and label: the 50-digit terms of H_jj, g_j (for x = +dot; x = -dot flips its sign) and loglik with
    their delta, as the module docstring defines them."""
    key = (eta_k.tobytes(), dot_k.tobytes(), B["w"], B["mu"], B["sp"])
    if key in _point_cache:
        return _point_cache[key]
    t = terms(eta_k)
    mp = mpmath.mpf
    out = {n: [] for n in ("tH", "dH", "tg", "dg", "tl", "dl", "t0", "d0")}
    with mpmath.workdps(DPS):
        for k in range(eta_k.size):
            xm = mp(float(dot_k[k]))
            tH = t.w[k] * xm * xm
            out["tH"].append(tH)
            out["dH"].append(mp(B["w"] * float(sp(t.f_w[k]))) * xm * xm + 2 * float(sp(float(tH))))
            smu, ssp, seta = float(sp(t.f_mu[k])), float(sp(t.f_sp[k])), float(sp(eta_k[k]))
            tg, dg, tl, dl, t0, d0 = [], [], [], [], [], []
            for yv in (0, 1):
                r = yv - t.mu[k]
                tg.append(r * xm)
                dg.append(abs(xm) * (B["mu"] * smu + yv * U) + float(sp(float(r * xm))))
                t0.append(r)                                                 # the ones column: x = 1
                d0.append(mp(B["mu"] * smu + yv * U + float(sp(float(r)))))
                term = yv * mp(float(eta_k[k])) - t.sp[k]
                tl.append(term)
                dl.append(mp(B["sp"] * ssp + yv * seta + float(sp(float(term)))))
            for n, v in (("tg", tg), ("dg", dg), ("tl", tl), ("dl", dl), ("t0", t0), ("d0", d0)):
                out[n].append(v)
    _point_cache[key] = out
    return out


def _sum_check(got, S, slack, abs_sum, m, what):
    with mpmath.workdps(DPS):
        bound = slack + 2 * (m + 2) * mpmath.mpf(U) * abs_sum
        err = abs(mpmath.mpf(float(got)) - S) if math.isfinite(float(got)) else mpmath.inf
        ok = err <= bound
        ratio = float(err / bound) if bound > 0 else (0.0 if err == 0 else math.inf)
    assert ok, (what, "got %r" % float(got), "ref %s" % mpmath.nstr(S, 20), "err %s" % mpmath.nstr(err, 5), "bound %s" % mpmath.nstr(bound, 5))
    return ratio


def check_sums(d, bounds, g=None, H=None, ll=None, scale=1.0, b0=None, what=""):
    """g [p (+1)], H [p, p] (no intercept) and loglik of a pass over design d against the 50-digit sums and the derived bounds;
    exact zeros where no row contributes.  Returns the worst error / bound ratio seen."""
    eta_k = np.ascontiguousarray(d.eta_k(scale, b0))
    pt = _point_terms(eta_k, np.ascontiguousarray(d.dot_k), bounds.B)
    icpt = (d.b0 if b0 is None else b0) is not None
    worst = 0.0
    mp = mpmath.mpf
    cnt = d.counts()
    present = np.nonzero(cnt.sum(1))[0]
    with mpmath.workdps(DPS):
        def total(ks, tname, dname, sign=None, per_label=True):
            S = slack = ab = mp(0); m = 0
            for k in ks:
                for yv in (0, 1):
                    c = int(cnt[k, yv])
                    if c:
                        term = pt[tname][k][yv] if per_label else pt[tname][k]
                        S += c * (term if sign is None or sign[k] > 0 else -term)
                        slack += c * (pt[dname][k][yv] if per_label else pt[dname][k]); ab += c * abs(term); m += c
            return S, slack, ab, m
        if ll is not None:
            worst = max(worst, _sum_check(float(np.asarray(ll).reshape(-1)[0]), *total(present, "tl", "dl"), what + " loglik"))
        gv = None if g is None else np.asarray(g, dtype=np.float64)
        Hv = None if H is None else np.asarray(H, dtype=np.float64)
        off = 0
        if gv is not None:
            assert gv.size == d.p + (1 if icpt else 0), (what, gv.size)
            if icpt:
                off = 1
                worst = max(worst, _sum_check(gv[0], *total(present, "t0", "d0"), what + " g[intercept]"))
        if gv is not None or Hv is not None:
            sign = d.beta[d.col_k]                                           # x = dot * beta_col
            by_col = [[] for _ in range(d.p)]
            for k in present:
                by_col[d.col_k[k]].append(k)
            for j in range(d.p):
                ks = by_col[j]
                if not ks:                                                   # no row in this column: exact zeros
                    if gv is not None:
                        assert gv[off + j] == 0.0, (what, "g of empty column", j, gv[off + j])
                    if Hv is not None:
                        assert Hv[j, j] == 0.0, (what, "H of empty column", j, Hv[j, j])
                    continue
                if gv is not None:
                    worst = max(worst, _sum_check(gv[off + j], *total(ks, "tg", "dg", sign), what + " g[%d]" % j))
                if Hv is not None:
                    worst = max(worst, _sum_check(Hv[j, j], *total(ks, "tH", "dH", per_label=False), what + " H[%d,%d]" % (j, j)))
        if Hv is not None:
            assert Hv.shape == (d.p, d.p), (what, Hv.shape)
            assert np.array_equal(Hv, Hv.T), (what, "H not symmetric bit for bit")
            offd = Hv[~np.eye(d.p, dtype=bool)]
            assert not np.any(offd != 0.0), (what, "nonzero off-diagonal of H", float(np.max(np.abs(offd))))
    return worst


def numpy_pass(d, term_fn=plain_terms, scale=1.0):
    """w per row, g, H, loglik of design d in plain numpy from the row terms term_fn gives (the CPU stand-in for a kernel)."""
    eta = d.eta_k(scale)[d.k]
    tr = term_fn(eta)
    resid = d.y - tr["mu"]
    g = np.bincount(d.col, weights=resid * d.x, minlength=d.p)
    if d.b0 is not None:
        g = np.concatenate([[np.sum(resid)], g])
    H = np.diag(np.bincount(d.col, weights=tr["w"] * d.x * d.x, minlength=d.p))
    ll = float(np.sum(d.y * eta - tr["sp"]))
    return tr["w"], g, H, ll
