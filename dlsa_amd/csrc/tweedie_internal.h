// The arithmetic of a Tweedie row that the family's two row models share (tweedie.hip: TweedieRow of the dense pass,
// onehot_tweedie.hip: OhTweedieRow of the structured one), and the compensated exp of a product that tweedie.hip's sum kernels
// use too.  The family's record and everything on the host is dispersion_internal.h's.
#pragma once
#include "common.h"

namespace dlsa {

#include "poisson_exp.h"  // exp_full

// exp(c x) without the rounding of the product c x: the product's low part enters as the factor 1 + lo (|lo| <= ulp(c x) / 2)
static __device__ __forceinline__ double tweedie_exp_prod(double c, double x) {
    const double hi = c * x, lo = fma(c, x, -hi);
    const double e = exp_full(hi);
    return fma(e, lo, e);
}

// what both row models compute of a row at unit dispersion, with a = mu^(1 - xi): y a, b = mu a and the weight (xi - 1) y a + (2 - xi) b.
// The residual is ya - b, the term ya / (1 - xi) - b / (2 - xi).
static __device__ __forceinline__ void tweedie_row(double one_m_xi, double two_m_xi, double y, double eta, double mu, double& ya,
                                                   double& b, double& w) {
    const double a = tweedie_exp_prod(one_m_xi, eta);
    b = mu * a;
    ya = y * a;
    w = fma(-one_m_xi, ya, two_m_xi * b);
}

}  // namespace dlsa
