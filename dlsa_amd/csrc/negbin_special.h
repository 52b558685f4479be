// fp64 digamma, trigamma and log-gamma pieces for the negative-binomial dispersion step (negbin.hip).  HIP has no fp64
// digamma / trigamma.  Included inside namespace dlsa.
#pragma once

// One shift of x > 0 by the recurrence to xs = x + n >= 10, then the Bernoulli (asymptotic) series at xs.  At xs >= 10 the
// first dropped terms are B16 / (16 xs^16) < 5e-17 (psi), B16 / xs^17 < 8e-17 (psi') and B16 / (240 xs^15) < 3e-17 (lgamma).
//   psi(x)    = log(xs) + d1          d1 = -sum_{k<n} 1/(x+k) - 1/(2 xs) - sum B2k / (2k xs^2k)
//   psi'(x)   = 1/xs    + d2          d2 =  sum_{k<n} 1/(x+k)^2 + 1/(2 xs^2) + sum B2k / xs^(2k+1)
//   lgamma(x) = (xs - 1/2) log(xs) - xs + log(2 pi)/2 + st - log(prod)     prod = prod_{k<n} (x+k)
// The logarithms stay with the caller, so a DIFFERENCE of two values takes them as one log1p of the arguments' ratio.
struct NbGamma {
    double xs, d1, d2, st, prod;
};

__device__ __forceinline__ NbGamma nb_gamma_parts(double x) {
    NbGamma r;
    double xs = x, d1 = 0.0, d2 = 0.0, prod = 1.0;
    for (int k = 0; k < 10 && xs < 10.0; ++k) {
        const double inv = 1.0 / xs;
        d1 -= inv;
        d2 = fma(inv, inv, d2);
        prod *= xs;
        xs += 1.0;
    }
    const double v = 1.0 / xs, v2 = v * v;
    double s1 = 8.3333333333333333e-02;                                   // B14/14 = 1/12
    s1 = fma(s1, v2, -2.1092796092796093e-02);                             // B12/12 = -691/32760
    s1 = fma(s1, v2, 7.5757575757575758e-03);                              // B10/10 = 1/132
    s1 = fma(s1, v2, -4.1666666666666667e-03);                             // B8/8 = -1/240
    s1 = fma(s1, v2, 3.9682539682539683e-03);                              // B6/6 = 1/252
    s1 = fma(s1, v2, -8.3333333333333333e-03);                             // B4/4 = -1/120
    s1 = fma(s1, v2, 8.3333333333333333e-02);                              // B2/2 = 1/12
    r.d1 = d1 - fma(s1, v2, 0.5 * v);
    double s2 = 1.1666666666666667e+00;                                   // B14 = 7/6
    s2 = fma(s2, v2, -2.5311355311355311e-01);                             // B12 = -691/2730
    s2 = fma(s2, v2, 7.5757575757575758e-02);                              // B10 = 5/66
    s2 = fma(s2, v2, -3.3333333333333333e-02);                             // B8 = -1/30
    s2 = fma(s2, v2, 2.3809523809523810e-02);                              // B6 = 1/42
    s2 = fma(s2, v2, -3.3333333333333333e-02);                             // B4 = -1/30
    s2 = fma(s2, v2, 1.6666666666666667e-01);                              // B2 = 1/6
    r.d2 = d2 + v2 * fma(s2, v, 0.5);
    double s3 = 6.4102564102564103e-03;                                   // B14/(14 13) = 1/156
    s3 = fma(s3, v2, -1.9175269175269175e-03);                             // B12/(12 11) = -691/360360
    s3 = fma(s3, v2, 8.4175084175084175e-04);                              // B10/(10 9) = 1/1188
    s3 = fma(s3, v2, -5.9523809523809524e-04);                             // B8/(8 7) = -1/1680
    s3 = fma(s3, v2, 7.9365079365079365e-04);                              // B6/(6 5) = 1/1260
    s3 = fma(s3, v2, -2.7777777777777778e-03);                             // B4/(4 3) = -1/360
    s3 = fma(s3, v2, 8.3333333333333333e-02);                              // B2/(2 1) = 1/12
    r.st = s3 * v;
    r.xs = xs;
    r.prod = prod;
    return r;
}

// psi(x) itself (x > 0).  From 10 upwards the series above.  Below, log(xs) alone would cost an ulp of 2.3 where psi is small (its
// root lies at 1.4616...), so x is moved into [1, 2) by the recurrence (exact subtractions of 1 going down) and
// psi(z) = (z - root) P(z - 3/2) there: root in two parts, P the degree-25 Chebyshev interpolant of psi(z) / (z - root) on
// [1, 2] in monomial form (relative error 5e-17 with the rounded coefficients).
__device__ __forceinline__ double nb_digamma(double x) {
    if (x >= 10.0) {
        const NbGamma a = nb_gamma_parts(x);
        return log(a.xs) + a.d1;
    }
    constexpr double P[26] = {
        -3.84048718862478651e-05, 5.76073316565046880e-05, -2.40031402421727776e-05, 3.60048205921819966e-05,
        -9.88631967219178544e-05, 1.48295512145961222e-04, -2.03673930272925966e-04, 3.05515369168641584e-04,
        -4.63350318212085493e-04, 6.95053487852584232e-04, -1.04172760469211636e-03, 1.56276704770233390e-03,
        -2.34470620723264533e-03, 3.51816426246369341e-03, -5.28001393866993091e-03, 7.92701824461559609e-03,
        -1.19082153427545936e-02, 1.79072484512251204e-02, -2.69757968398763488e-02, 4.07608339380280474e-02,
        -6.19221332717157860e-02, 9.49887244529180885e-02, -1.48404923053917309e-01, 2.40542484240786891e-01,
        -4.23627421281460470e-01, 9.51055876031832836e-01,
    };
    double acc = 0.0, z = x;
    if (z < 1.0) { acc = -1.0 / z; z += 1.0; }
    if (z < 1.0) { acc -= 1.0 / z; z += 1.0; }               // (z + 1 rounded up to 1 only for x below 2^-53: psi ~ -1/x there)
    for (int k = 0; k < 9 && z >= 2.0; ++k) { z -= 1.0; acc += 1.0 / z; }
    const double t = z - 1.5;
    double q = P[0];
#pragma unroll
    for (int k = 1; k < 26; ++k) q = fma(q, t, P[k]);
    const double r = (z - 1.4616321449683622) - 9.549995429965697e-17;
    return fma(r, q, acc);
}
__device__ __forceinline__ double nb_trigamma(double x) {
    const NbGamma a = nb_gamma_parts(x);
    return 1.0 / a.xs + a.d2;
}

constexpr int NB_SUM_MAX = 32;      // integer counts below this take the finite sums

// The three differences of the dispersion step at theta = 1 / alpha > 0 and a count y >= 0:
//   D1 = psi(y + theta) - psi(theta),  D2 = psi'(theta) - psi'(y + theta),  C = lgamma(y + theta) - lgamma(theta) - y log(theta).
// All three tend to 0 like alpha as theta grows, while the functions themselves grow: taken naively at theta = 1e6 they keep
// 6 to 9 digits.  An integer y < NB_SUM_MAX takes the finite sums, every term of which is small itself:
//   D1 = sum_{j<y} alpha / (1 + alpha j),  D2 = sum_{j<y} (alpha / (1 + alpha j))^2,  C = sum_{j<y} log1p(alpha j) = log1p(prod (1 + alpha j) - 1)
// (the product stays below (1 + 31 alpha)^31 and is carried as its excess over 1, e <- e + alpha j + e alpha j, so a small
// alpha keeps its digits).
// Any other y takes the shifted series of both arguments with the leading logarithms merged into log1p of the ratio and the
// leading reciprocals into one quotient; what is then subtracted are the O(1/x) tails.
__device__ __forceinline__ void nb_diffs(double y, double theta, double alpha, double& D1, double& D2, double& C) {
    if (y < (double)NB_SUM_MAX && y == floor(y)) {
        double d1 = 0.0, d2 = 0.0, e = 0.0;                // e = prod (1 + alpha j) - 1, carried as such: small stays small
        const int m = (int)y;
        for (int j = 0; j < m; ++j) {
            const double aj = alpha * (double)j;
            const double t = alpha / (1.0 + aj);
            d1 += t;
            d2 = fma(t, t, d2);
            e = fma(e, aj, e + aj);
        }
        D1 = d1; D2 = d2; C = log1p(e);
        return;
    }
    const NbGamma a = nb_gamma_parts(y + theta), b = nb_gamma_parts(theta);
    const double gap = a.xs - b.xs;                       // y + (shift of y + theta) - (shift of theta)
    const double lp = log1p(gap / b.xs);                  // log(a.xs / b.xs)
    D1 = lp + (a.d1 - b.d1);
    D2 = gap / (a.xs * b.xs) + (b.d2 - a.d2);
    if (theta >= 10.0) {                                  // no shift: (a - 1/2) log1p(y / theta) - y + the tails
        C = fma(a.xs - 0.5, lp, -y) + (a.st - b.st);
    } else {
        const double lb = log(b.xs);
        C = fma(a.xs - 0.5, lp, gap * lb - gap) + (a.st - b.st) - log(a.prod / b.prod) - y * log(theta);
    }
}
