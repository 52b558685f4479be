/* The start value of the probit fit's intercept: the standard normal quantile of the response share.  Host code in plain C (no
 * library has the quantile), in a header of its own so that tests/test_binary_cpu.py compiles it into a small program and holds it
 * against scipy's ndtri.  Included by binary.hip inside namespace dlsa. */
#pragma once
#include <math.h>

/* Phi^-1(ones / rows) for 0 < ones < rows.  The quantile is taken in the LOWER tail, of m = min(ones, rows - ones) (so the share keeps
 * its relative accuracy next to 1), and mirrored: bisection of Phi(x) = erfc(-x / sqrt 2) / 2 on [-40, 0] -- Phi(-40) is 0 in fp64,
 * below any share -- until the bracket has no interior point.  A bracketed root cannot run away:
 * Newton from the logit's scaling overshoots across the flat tail for shares beyond 0.005 .. 0.995 and ends anywhere. */
static inline double dlsa_probit_quantile(double ones, double rows) {
    const double m = ones <= rows - ones ? ones : rows - ones;
    const double target = m / rows;
    if (m + m == rows) return 0.0;                             /* the median, exactly */
    double lo = -40.0, hi = 0.0;                              /* Phi(lo) < target <= Phi(hi) = 1/2 */
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (0.5 * erfc(-mid * 0.70710678118654752440) < target) lo = mid; else hi = mid;
    }
    return m == ones ? hi : -hi;
}
