// exp over the whole signed range for the Poisson kernels (poisson.hip, onehot_poisson.hip).  Included inside namespace dlsa.
#pragma once

// exp(a) over the whole signed range in ~20 instructions (CDNA has no fp64 exp): k = rint(a log2 e), r = a - k ln2 with a
// two-part ln2 (|r| <= 0.347), the degree-13 Taylor polynomial of exp_neg (logistic.h), ldexp.  <= 2 ulp over the normal
// range.  a below -746 gives 0 (exp(-745.13) is the smallest subnormal), a above 709.78 gives +inf (2^k overflows), NaN
// stays NaN (the clamps are comparisons, not fmin / fmax).
__device__ __forceinline__ double exp_full(double a) {
    a = a < -746.0 ? -746.0 : (a > 710.0 ? 710.0 : a);
    const double kf = rint(a * 1.4426950408889634);
    double r = fma(kf, -6.93147180369123816490e-01, a);
    r = fma(kf, -1.90821492927058770002e-10, r);
    double q = 1.6059043836821613e-10;                      // 1/13!
    q = fma(q, r, 2.08767569878681e-09);
    q = fma(q, r, 2.505210838544172e-08);
    q = fma(q, r, 2.755731922398589e-07);
    q = fma(q, r, 2.7557319223985893e-06);
    q = fma(q, r, 2.48015873015873e-05);
    q = fma(q, r, 1.984126984126984e-04);
    q = fma(q, r, 1.388888888888889e-03);
    q = fma(q, r, 8.333333333333333e-03);
    q = fma(q, r, 4.1666666666666664e-02);
    q = fma(q, r, 1.6666666666666666e-01);
    q = fma(q, r, 0.5);
    q = fma(q, r, 1.0);
    q = fma(q, r, 1.0);
    return ldexp(q, (int)kf);
}
