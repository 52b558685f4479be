"""Reference, grids, designs and bounds for the row terms of the probit and cloglog map steps (csrc/binary_terms.h), over the WHOLE
range of eta, and a CPU Newton fit of both models.  No GPU, no torch.

Per row (y in {0, 1}, eta): l = the log-likelihood term, r = dl / deta, w = -d2l / deta2 (the observed information).
  probit   s = 2y - 1, z = s eta, lambda = phi(z) / Phi(z):  l = log Phi(z), r = s lambda, w = lambda (z + lambda)
  cloglog  mu = e^eta;  y = 0: l = -mu, r = -mu, w = mu;  y = 1: l = log(1 - e^-mu), r = mu / (e^mu - 1), w = r (mu + r - 1)

* ref_terms(link, eta, y): the TEXTBOOK forms in mpmath.  Probit at 60 digits, with log Phi(z) for z > 0 taken as log1p(-Phi(-z))
  (the plain log Phi is itself wrong beyond z = 16 at 60 digits); z + lambda loses 14 digits at z = -1e7.  Cloglog at 900 digits:
  mu + r - 1 at mu = 1e-300 cancels 600 of them (200 digits between eta = -100 and 5.5, where at most 110 cancel).
* model_terms(link, eta, y): a plain fp64 evaluation in numpy / scipy of the cancellation-free forms (below), and the mutants -- the
  textbook forms -- that the bounds must reject.  It is NOT the kernel's evaluation (which fits K and the two cloglog series); it
  is the fp64 yardstick the kernel's accuracy class is measured by:
    probit, z <= 0, a = -z:  lambda = sqrt(2 / pi) / erfcx(a / sqrt 2), l = -a^2 / 2 + log(erfcx(a / sqrt 2) / 2), w = lambda K(a) with
                             K = lambda - a for a < 1/4 (lambda / K <= 1.4 there: the subtraction is harmless) and Laplace's continued
                             fraction 1 / (a + 2 / (a + 3 / ...)) for a >= 1/4, with as many terms as its convergence there asks
    probit, z > 0:           E = exp(-z^2 / 2) with the square split by one fma, Q = erfcx(z / sqrt 2) E / 2, l = log1p(-Q),
                             lambda = E / (sqrt(2 pi) (1 - Q)), w = lambda (z + lambda)
    cloglog, y = 1:          mu < 1/4: the Bernoulli series of A = mu + r - 1 = mu / 2 + mu^2 / 12 - ..., r = 1 - mu + A, and
                             l = eta + log(-expm1(-mu) / mu) by its series;  mu >= 1/4: r = mu / expm1(mu) (mu e^-mu / (1 - e^-mu)
                             where e^mu overflows), A = (mu + expm1(-mu)) / (-expm1(-mu)), l = log(-expm1(-mu)) below log 2 and
                             log1p(-exp(-mu)) above
* Grids (z = s eta: a grid in eta meets z on both sides through the two responses): a full sweep, regime grids of 257 points (a
  unit interval round each centre, and the tiny values), the seams of every branch the kernel has (probit: z = 0, a = 2, 4, 8, 39;
  cloglog: mu = 1, the subnormal mu below eta = -708, mu = 0 below -745.13, e^-mu = 0 above mu = 745), +-0, +-5e-324, +-10^k.
  Probit: |eta| up to 1e7 (z = +1e7 has l = r = w = 0).  Cloglog: eta from -745.5 to 6.6; "beyond" runs on to 710 for the y = 0 rows.
* Designs: logistic_reference.Design on these grids -- rows with ONE nonzero entry and beta = +-1, so eta is known exactly in any
  summation order -- with n = 2 G rows, so that every grid point meets both responses.  With the implicit intercept b0 the reference
  takes eta := fl(b0 + x); with offsets eta := fl(fl(x [+ b0]) + o), where o = the grid point rounded to an integer and x = the rest
  (exact), so the sum is the grid point again.
* Bounds, the convention of logistic_reference (u = 2^-53, sp(v) = np.spacing(|v|): subnormal results compare in absolute spacing):
    per row  |t - t*| <= B_t sp(t*) + floor_t, t in {l, r, w}, B_t = max(4, 2 E_t), E_t = the worst ulp error of model_terms against
             ref_terms on the same grid and response, MEASURED when the bounds are built.  floor_t = 2 sp(mu*) |dt / dmu| for
             cloglog, y = 1, eta > 2 (the derivative in mpmath), else 0: the terms are functions of the ROUNDED mu, and e^-mu
             amplifies one ulp of mu by mu.  That is the floor of the formulation (as y - mu is for the logistic terms).
    any sum  S = sum t_i of m terms in any order: |S - S*| <= sum delta_i + 2 (m + 2) u sum |t_i*|, with
             H_jj, t = w x^2:  delta = (B_w sp(w*) + floor_w) x^2 + 2 sp(t*)
             g_j,  t = r x:    delta = |x| (B_r sp(r*) + floor_r) + sp(t*)          (x = 1 for the intercept's entry)
             l:                delta = B_l sp(l*) + floor_l
No row, column or regime is left out of any check."""
import contextlib
import functools
import math

import mpmath
import numpy as np
from scipy import special

import logistic_reference as lr

U = lr.U
sp = lr.sp
LINKS = ("probit", "cloglog")
KEYS = ("l", "r", "w")
DPS = {"probit": 60, "cloglog": 900}
REGIME_POINTS = 257

# ------------------------------------------------------------------------------------------------ grids
# the centres of the unit intervals; z = +-centre through the two responses
REGIMES = {
    "probit": ("tiny", 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 7.5, 8.0, 20.0, 30.0, 38.0, 39.0, 100.0, 1e4, 1e7),
    "cloglog": (-745.0, -720.0, -708.0, -400.0, -100.0, -37.0, -20.0, -5.0, -3.5, -2.5, -1.4, -0.7, "tiny", 0.5, 1.0, 1.5, 2.5, 3.5, 5.0, 6.1),
}
# where the kernel (and the model evaluation) changes branch
SEAMS = {
    "probit": (2.0, 4.0, 8.0, 16.0, 38.5, 38.6, 39.0, 1e154, 1.4e154),
    "cloglog": (0.0, -1.3862943611198906, -0.36651292058166435, 6.6, 6.5, 6.563, -708.0, -708.4, -744.44, -745.13, -745.2),
}


@functools.lru_cache(maxsize=None)
def grid(link, name):
    rng = np.random.default_rng(20250309)
    pw = 10.0 ** np.arange(-300, 1, dtype=np.float64)
    seams = np.array([v for v in SEAMS[link] if abs(v) < 1e100])
    near = np.concatenate([np.nextafter(seams, -np.inf), seams, np.nextafter(seams, np.inf)])
    if name == "full":
        if link == "probit":
            g = np.concatenate([np.linspace(-40.0, 40.0, 2001), rng.uniform(-9.0, 9.0, 1473), pw, -pw, 10.0 ** np.arange(1, 8), -10.0 ** np.arange(1, 8),
                                [0.0, -0.0, 5e-324, -5e-324], near, -near])
        else:
            g = np.concatenate([np.linspace(-745.5, 6.6, 2001), rng.uniform(-5.0, 2.0, 1473), pw, -pw, -10.0 ** np.arange(1, 3),
                                [0.0, -0.0, 5e-324, -5e-324], near[near <= 6.6]])
    elif name == "beyond":                                  # cloglog past eta = 6.6: bounds for y = 0, no NaN for y = 1
        g = np.concatenate([np.linspace(6.6, 709.5, REGIME_POINTS), [709.7, 709.78, 709.782712893384]])
    elif name == "tiny":
        g = 10.0 ** np.linspace(-8.0, -300.0, REGIME_POINTS) * np.where(np.arange(REGIME_POINTS) % 2 == 0, 1.0, -1.0)
    else:
        # one point in each of 257 cells of the unit interval, at a seeded random place: points on a dyadic lattice have exact
        # squares and would hide the rounding of z * z
        g = float(name) - 0.5 + (np.arange(REGIME_POINTS) + rng.uniform(0.0, 1.0, REGIME_POINTS)) / REGIME_POINTS
    g = np.ascontiguousarray(g, dtype=np.float64)
    g.setflags(write=False)
    return g


def regime_centre(name):
    return 0.0 if name in ("tiny", "full", "beyond") else float(name)


# ------------------------------------------------------------------------------------------------ reference (mpmath)
def _probit_mp(eta, y):
    z = eta if y else -eta
    if z > 0:
        Q = mpmath.ncdf(-z)
        l, lam = mpmath.log1p(-Q), mpmath.npdf(z) / (1 - Q)
    else:
        P = mpmath.ncdf(z)
        l, lam = mpmath.log(P), mpmath.npdf(z) / P
    return l, (lam if y else -lam), lam * (z + lam), (0, 0, 0)


def _cloglog_mp(eta, y):
    mu = mpmath.exp(eta)
    if not y:
        return -mu, -mu, mu, (0, 0, 0)
    l = mpmath.log(-mpmath.expm1(-mu))
    r = mu / mpmath.expm1(mu)
    A = mu + r - 1
    w = r * A
    # d / dmu = (d / deta) / mu:  l' = r / mu,  r' = -w / mu,  w' = r' A + r (1 + r')
    dr = -w / mu
    return l, r, w, (r / mu, dr, dr * A + r * (1 + dr))


def _dps(link, eta):
    """probit: 60 digits.  cloglog: 900 where mu + r - 1 (2 |eta| / ln 10 digits cancel below 0) or 1 - e^-mu (mu / ln 10 digits above)
    needs them, 200 between eta = -100 and 5.5, where at most 110 digits cancel"""
    return DPS[link] if link == "probit" or eta < -100.0 or eta > 5.5 else 200


_point_cache = {}


def _point(link, eta, y):
    """(l, r, w) as mpf rounded to 60 digits and the three floors at one (eta, y), cached by eta's bits"""
    key = (link, y, float(eta).hex())
    if key not in _point_cache:
        fn = _probit_mp if link == "probit" else _cloglog_mp
        with mpmath.workdps(_dps(link, eta)):
            l, r, w, d = fn(mpmath.mpf(float(eta)), y)
            floors = (0.0, 0.0, 0.0)
            if link == "cloglog" and y and eta > 2.0:
                smu = float(sp(float(mpmath.exp(mpmath.mpf(float(eta))))))
                floors = tuple(2.0 * smu * abs(float(t)) for t in d)
            with mpmath.workdps(60):
                _point_cache[key] = (+l, +r, +w, floors)
    return _point_cache[key]


class Terms:
    """The textbook values at (eta[k], y): lists of mpf (.l, .r, .w), their fp64 roundings (.f_l ...) and the floors (.floor_l ...)."""

    def __init__(self, link, eta, y):
        self.eta = np.array(eta, dtype=np.float64)
        pts = [_point(link, float(v), y) for v in self.eta]
        for j, key in enumerate(KEYS):
            setattr(self, key, [q[j] for q in pts])
            setattr(self, "f_" + key, np.array([float(q[j]) for q in pts]))
            setattr(self, "floor_" + key, np.array([q[3][j] for q in pts]))


_terms_cache = {}


def ref_terms(link, eta, y):
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    key = (link, int(y), eta.tobytes())
    if key not in _terms_cache:
        _terms_cache[key] = Terms(link, eta, int(y))
    return _terms_cache[key]


# ------------------------------------------------------------------------------------------------ the plain fp64 evaluation
K_SEAM = 0.25         # the model evaluation takes K by the continued fraction from here on, by the subtraction below


def _laplace_K(a):
    """1 / (a + 2 / (a + 3 / (a + ...))) from the tail, for a > 0.  Measured against mpmath: 1000 / a^2 terms leave a truncation below
    an ulp (16000 at a = 1/4, 4000 at 1/2, 250 at 2) and the backward recurrence adds no rounding to speak of (0.2 ulp); the points are taken
    in three bands so that only the small a pay for their term count."""
    out = np.empty_like(a)
    for lo, hi in ((0.0, 1.0), (1.0, 2.0), (2.0, np.inf)):
        sel = (a >= lo) & (a < hi)
        if np.any(sel):
            v = a[sel]
            t = v.copy()
            for k in range(int(1200.0 / float(np.min(v)) ** 2) + 40, 1, -1):
                t = v + k / t
            out[sel] = 1.0 / t
    return out


_BERNOULLI_A = (1 / 2, 1 / 12, 0.0, -1 / 720, 0.0, 1 / 30240, 0.0, -1 / 1209600, 0.0, 1 / 47900160, 0.0, -691 / 1307674368000)
# log((1 - e^-m) / m) = -m/2 + m^2/24 - m^4/2880 + m^6/181440 - m^8/9676800 + m^10/479001600 - 691 m^12 / 15692092416000
_SERIES_L = (-1 / 2, 1 / 24, 0.0, -1 / 2880, 0.0, 1 / 181440, 0.0, -1 / 9676800, 0.0, 1 / 479001600, 0.0, -691 / 15692092416000)


def _square_error(a, zz):
    """fma(a, a, -zz) for zz = fl(a * a) by Veltkamp's splitting (exact where nothing over- or underflows; 0 elsewhere)"""
    c = 134217729.0 * a
    hi = c - (c - a)
    lo = a - hi
    err = ((hi * hi - zz) + 2.0 * hi * lo) + lo * lo
    return np.where(np.isfinite(err) & (zz > 1e-290), err, 0.0)


def _horner_up(c, m):
    q = np.zeros_like(m)
    for v in reversed(c):
        q = q * m + v
    return q


def model_terms(link, eta, y, mutant=None, k_seam=K_SEAM):
    """{l, r, w} at (eta, y) in plain fp64 (numpy's exp / log / log1p / expm1, scipy's erfcx), or with one textbook form put back:
    probit "w_lam_plus_z" (w = lambda (lambda + z) for z < 0), "square_unsplit" (exp(-(z * z) / 2)); cloglog "w_direct" (r (mu + r - 1)),
    "ll_log_expm1" (l = log(-expm1(-mu)) everywhere).  k_seam: where the probit K changes from the subtraction to the continued
    fraction (newton_fit's fp64 iterations, which mpmath steps finish, take 2.0 for speed)."""
    eta = np.asarray(eta, dtype=np.float64)
    with np.errstate(all="ignore"):
        if link == "probit":
            z = eta if y else -eta
            a = np.abs(z)
            c = special.erfcx(a * math.sqrt(0.5))
            # z <= 0
            lam_n = math.sqrt(2.0 / math.pi) / c
            K = np.where(a < k_seam, lam_n - a, _laplace_K(np.maximum(a, k_seam)))
            w_n = lam_n * (lam_n - a) if mutant == "w_lam_plus_z" else lam_n * K
            l_n = -0.5 * a * a + np.log(0.5 * c)
            # z > 0
            zz = a * a
            if mutant == "square_unsplit":
                E = np.exp(-0.5 * zz)
            else:
                lo = _square_error(a, zz)
                E = np.exp(-0.5 * zz) * (1.0 - 0.5 * lo)
            Q = 0.5 * c * E
            lam_p = E / (math.sqrt(2.0 * math.pi) * (1.0 - Q))
            neg = z <= 0
            lam = np.where(neg, lam_n, lam_p)
            return {"l": np.where(neg, l_n, np.log1p(-Q)), "r": lam if y else -lam, "w": np.where(neg, w_n, lam_p * (a + lam_p))}
        mu = np.exp(eta)
        if not y:
            return {"l": -mu, "r": -mu, "w": mu}
        small = mu < 0.25
        ms = np.where(small, mu, 0.0)
        A_s = ms * _horner_up(_BERNOULLI_A, ms)
        r_s = 1.0 - ms + A_s
        l_s = eta + ms * _horner_up(_SERIES_L, ms)
        mb = np.where(small, 1.0, mu)
        em1 = np.expm1(-mb)                                  # -(1 - e^-mu)
        em = np.exp(-mb)
        r_b = np.where(em == 0.0, 0.0, np.where(mb > 700.0, mb * em / (-em1), mb / np.expm1(mb)))      # (expm1(mu) overflows at 709.8)
        A_b = np.where(np.isinf(mb), mb, (mb + em1) / (-em1))
        l_b = np.where(mb < math.log(2.0), np.log(-em1), np.log1p(-em))
        r = np.where(small, r_s, r_b)
        A = np.where(small, A_s, A_b)
        l = np.where(small, l_s, l_b)
        w = np.where(r == 0.0, 0.0, r * A)
        if mutant == "w_direct":
            rd = mu / np.expm1(mu)
            r, w = rd, rd * (mu + rd - 1.0)
        if mutant == "ll_log_expm1":
            l = np.log(-np.expm1(-mu))
        return {"l": l, "r": r, "w": w}


def ulp_errors(got, t, key):
    """|got - ref| / sp(ref) per point against Terms t (the difference at 50 digits)"""
    return lr.ulp_errors(got, getattr(t, key), getattr(t, "f_" + key))


# ------------------------------------------------------------------------------------------------ bounds
class Bounds:
    """E[y][key] = the model evaluation's worst ulp error on the grid with response y, B = max(4, 2 E)."""

    def __init__(self, link, name):
        g = grid(link, name)
        self.link, self.name = link, name
        self.E, self.B = {}, {}
        for y in (0, 1):
            t = ref_terms(link, g, y)
            m = model_terms(link, g, y)
            self.E[y] = {key: float(np.max(ulp_errors(m[key], t, key))) for key in KEYS}
            self.B[y] = {key: max(4.0, 2.0 * v) for key, v in self.E[y].items()}

    def __repr__(self):
        return "%s %s: " % (self.link, self.name) + "; ".join("y=%d " % y + " ".join("E_%s %.2f" % kv for kv in self.E[y].items()) for y in (0, 1))


@functools.lru_cache(maxsize=None)
def bounds(link, name):
    return Bounds(link, name)


def z_range(link, name, y):
    """probit: (min, max) of z = s eta over the grid with response y; cloglog: of eta"""
    g = grid(link, name)
    v = g if (y or link == "cloglog") else -g
    return float(np.min(v)), float(np.max(v))


# ------------------------------------------------------------------------------------------------ designs
@contextlib.contextmanager
def _grids_of(link):
    """logistic_reference.Design looks its grid up by name: for the time of the call the names are this module's"""
    saved = lr.grid
    lr.grid = lambda name: grid(link, name)
    try:
        yield
    finally:
        lr.grid = saved


class Design(lr.Design):
    """logistic_reference.Design on grid (link, name) with n = 2 G rows by default (every point meets both responses).  offset=True:
    every row carries the offset o = its grid point rounded to an integer (0 below 1 in size) and x = the rest; with an intercept as
    well, b0 must be 0.0."""

    def __init__(self, link, name, p, b0=None, offset=False, n=None):
        G = grid(link, name).size
        with _grids_of(link):
            super().__init__(name, 2 * G if n is None else n, p, b0=b0)
        self.link = link
        self.off_k = None
        if offset:
            assert b0 is None or b0 == 0.0
            g = grid(link, name)
            self.off_k = np.where(np.abs(g) >= 1.0, np.round(g), 0.0)
            self.dot_k = g - self.off_k                                     # exact
            assert np.array_equal(self.dot_k + self.off_k, g)
            self.x_k = self.dot_k * self.beta[self.col_k]
            self.x = self.x_k[self.k]

    def eta_k(self, scale=1.0, b0=None):
        e = super().eta_k(scale, b0)
        return e + self.off_k if self.off_k is not None else e

    def offset(self):
        return None if self.off_k is None else self.off_k[self.k]


# ------------------------------------------------------------------------------------------------ checkers
def check_rows(link, got, key, eta_rows, y_rows, b, what=""):
    """per-row values of l / r / w at the rows' (eta, y) against B sp(ref) + floor; returns the worst error / bound ratio and prints
    the worst ulp error.  Rows with the same (eta, y, value) bits are checked once."""
    eta_rows = np.ascontiguousarray(eta_rows, dtype=np.float64)
    got = np.ascontiguousarray(got, dtype=np.float64)
    assert got.shape == eta_rows.shape, (what, got.shape, eta_rows.shape)
    worst_ratio = 0.0
    for y in (0, 1):
        sel = np.asarray(y_rows) == y
        if not np.any(sel):
            continue
        pairs = np.unique(np.stack([eta_rows[sel].view(np.int64), got[sel].view(np.int64)], 1), axis=0)      # by bit pattern
        eta_u, got_u = pairs[:, 0].copy().view(np.float64), pairs[:, 1].copy().view(np.float64)
        uniq, inv = np.unique(pairs[:, 0], return_inverse=True)
        t = ref_terms(link, uniq.view(np.float64), y)
        mp_list, f, floor = getattr(t, key), getattr(t, "f_" + key)[inv], getattr(t, "floor_" + key)[inv]
        err = lr.ulp_errors(got_u, [mp_list[j] for j in inv], f)
        allowed = b.B[y][key] + floor / sp(f)
        ratio = err / allowed
        i = int(np.argmax(ratio))
        print("%s: y=%d %s worst %.3f ulp at eta = %r (allowed %.2f)" % (what, y, key, err[i], float(eta_u[i]), allowed[i]))
        assert ratio[i] <= 1.0, (what, y, key, float(err[i]), float(allowed[i]), float(eta_u[i]), float(got_u[i]), float(f[i]))
        worst_ratio = max(worst_ratio, float(ratio[i]))
    return worst_ratio


def _point_terms(link, eta_k, dot_k, b):
    """per grid point and response: the terms of H_jj, g_j (x = +dot), g_0 and loglik with their deltas, as the module docstring says"""
    mp = mpmath.mpf
    out = {n: [] for n in ("tH", "dH", "tg", "dg", "t0", "d0", "tl", "dl")}
    tt = [ref_terms(link, eta_k, y) for y in (0, 1)]
    with mpmath.workdps(60):
        for k in range(eta_k.size):
            xm = mp(float(dot_k[k]))
            row = {n: [] for n in out}
            for y in (0, 1):
                t, B = tt[y], b.B[y]
                tH = t.w[k] * xm * xm
                row["tH"].append(tH)
                row["dH"].append(mp(B["w"] * float(sp(t.f_w[k])) + t.floor_w[k]) * xm * xm + 2 * float(sp(float(tH))))
                dr = mp(B["r"] * float(sp(t.f_r[k])) + t.floor_r[k])
                row["tg"].append(t.r[k] * xm)
                row["dg"].append(abs(xm) * dr + float(sp(float(t.r[k] * xm))))
                row["t0"].append(t.r[k])
                row["d0"].append(dr + float(sp(t.f_r[k])))
                row["tl"].append(t.l[k])
                row["dl"].append(mp(B["l"] * float(sp(t.f_l[k])) + t.floor_l[k]))
            for n in out:
                out[n].append(row[n])
    return out


def check_sums(d, b, g=None, Hdiag=None, ll=None, what=""):
    """g [p (+1)], the diagonal of H over X's columns [p] and loglik of a pass over design d against the mpmath sums and the derived
    bounds; exact zeros where no row contributes.  Returns the worst error / bound ratio."""
    eta_k = np.ascontiguousarray(d.eta_k())
    pt = _point_terms(d.link, eta_k, np.ascontiguousarray(d.dot_k), b)
    icpt = d.b0 is not None
    cnt = d.counts()
    present = np.nonzero(cnt.sum(1))[0]
    worst = 0.0
    mp = mpmath.mpf
    with mpmath.workdps(60):
        def total(ks, tname, dname, sign=None):
            S = slack = ab = mp(0); m = 0
            for k in ks:
                for y in (0, 1):
                    c = int(cnt[k, y])
                    if c:
                        term = pt[tname][k][y]
                        S += c * (term if sign is None or sign[k] > 0 else -term)
                        slack += c * pt[dname][k][y]; ab += c * abs(term); m += c
            return S, slack, ab, m
        if ll is not None:
            worst = max(worst, lr._sum_check(float(np.asarray(ll).reshape(-1)[0]), *total(present, "tl", "dl"), what + " loglik"))
        gv = None if g is None else np.asarray(g, dtype=np.float64)
        Hv = None if Hdiag is None else np.asarray(Hdiag, dtype=np.float64)
        off = 0
        if gv is not None:
            assert gv.size == d.p + (1 if icpt else 0), (what, gv.size)
            if icpt:
                off = 1
                worst = max(worst, lr._sum_check(gv[0], *total(present, "t0", "d0"), what + " g[intercept]"))
        sign = d.beta[d.col_k]
        by_col = [[] for _ in range(d.p)]
        for k in present:
            by_col[d.col_k[k]].append(k)
        for j in range(d.p):
            ks = by_col[j]
            if not ks:
                assert gv is None or gv[off + j] == 0.0, (what, "g of empty column", j)
                assert Hv is None or Hv[j] == 0.0, (what, "H of empty column", j)
                continue
            if gv is not None:
                worst = max(worst, lr._sum_check(gv[off + j], *total(ks, "tg", "dg", sign), what + " g[%d]" % j))
            if Hv is not None:
                worst = max(worst, lr._sum_check(Hv[j], *total(ks, "tH", "dH"), what + " H[%d,%d]" % (j, j)))
    return worst


def numpy_pass(d, mutant=None):
    """w per row, g, diag H over X's columns and loglik of design d from model_terms: the CPU stand-in for a kernel"""
    eta = d.eta()
    tr = {key: np.empty(d.n) for key in KEYS}
    for y in (0, 1):
        sel = d.y == y
        m = model_terms(d.link, eta[sel], y, mutant)
        for key in KEYS:
            tr[key][sel] = m[key]
    g = np.bincount(d.col, weights=tr["r"] * d.x, minlength=d.p)
    if d.b0 is not None:
        g = np.concatenate([[np.sum(tr["r"])], g])
    Hd = np.bincount(d.col, weights=tr["w"] * d.x * d.x, minlength=d.p)
    return tr["w"], g, Hd, float(np.sum(tr["l"]))


# ------------------------------------------------------------------------------------------------ the CPU fit
def _row_terms_ld(link, eta, y, dps=40):
    """(l, r, w) per row as longdouble arrays, from mpmath at `dps` digits (eta: longdouble)"""
    fn = _probit_mp if link == "probit" else _cloglog_mp
    out = np.empty((3, eta.size), dtype=np.longdouble)
    with mpmath.workdps(dps):
        for i in range(eta.size):
            e = float(eta[i])
            em = mpmath.mpf(e) + mpmath.mpf(float(eta[i] - np.longdouble(e)))
            t = fn(em, int(y[i]))[:3]
            for j in range(3):
                hi = float(t[j])
                out[j, i] = np.longdouble(hi) + np.longdouble(float(t[j] - hi))
    return out


def newton_fit(link, X, y, offset=None, fit_intercept=False, max_iter=100):
    """The MLE of one partition and the block the map step returns: fp64 Newton on model_terms to convergence, then steps whose row
    terms come from mpmath and whose sums run in longdouble, until the step is below 1e-15 (relative to max(1, |beta|_inf)).  Returns
    (coef, Sig_inv = the observed information at coef, Sig_inv coef, loglik) in fp64."""
    n = X.shape[0]
    D = np.concatenate([np.ones((n, 1)), X], 1) if fit_intercept else np.asarray(X, dtype=np.float64)
    o = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
    beta = np.zeros(D.shape[1])
    if fit_intercept:
        ybar = float(np.mean(y))
        beta[0] = (special.ndtri(ybar) if link == "probit" else math.log(-math.log1p(-ybar))) - math.log(np.mean(np.exp(o)))

    def terms64(b):
        eta = D @ b + o
        out = {key: np.empty(n) for key in KEYS}
        for yy in (0, 1):
            sel = y == yy
            m = model_terms(link, eta[sel], yy, k_seam=2.0)
            for key in KEYS:
                out[key][sel] = m[key]
        return out

    ll_prev = -np.inf
    for _ in range(max_iter):
        t = terms64(beta)
        ll = float(np.sum(t["l"]))
        step = np.linalg.solve(D.T @ (D * t["w"][:, None]), D.T @ t["r"])
        while True:                                          # halve a step that lowers the likelihood
            cand = beta + step
            llc = float(np.sum(terms64(cand)["l"]))
            if np.isfinite(llc) and llc >= ll - 1e-12 * abs(ll):
                break
            step = step / 2
            if np.max(np.abs(step)) < 1e-300:
                break
        beta = cand
        if np.max(np.abs(step)) <= 1e-12 * max(1.0, np.max(np.abs(beta))) and abs(llc - ll_prev) >= 0:
            break
        ll_prev = ll
    Dl, ol = D.astype(np.longdouble), o.astype(np.longdouble)
    bl = beta.astype(np.longdouble)
    for _ in range(6):
        l, r, w = _row_terms_ld(link, Dl @ bl + ol, y)
        H64 = (D.T @ (D * w.astype(np.float64)[:, None]))
        step = np.linalg.solve(H64, (Dl.T @ r).astype(np.float64))
        small = np.max(np.abs(step)) <= 1e-15 * max(1.0, float(np.max(np.abs(bl))))
        if small:
            break
        bl = bl + step.astype(np.longdouble)
    else:
        raise AssertionError("newton_fit: the extended-precision steps did not settle")
    H = Dl.T @ (Dl * w[:, None])
    return bl.astype(np.float64), H.astype(np.float64), (H @ bl).astype(np.float64), float(np.sum(l))
