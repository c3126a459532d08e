// The acquisition criteria of gprhip_acquire at one test point: the value a and its partial derivatives c_mu = da/dmu,
// c_v = da/dsigma2 from the predictive mean and variance (include/gprhip.h has the table).  Every criterion is "larger is
// better".  With s = +-1 the direction, v = max(variance, var_floor), sigma = sqrt(v), delta = s (mu - best) - xi,
// u = delta / sigma, Phi / phi the standard normal cdf / pdf and h(u) = phi(u) + u Phi(u):
//   EI      a = sigma h(u)             c_mu = s Phi(u)                c_v = phi(u) / (2 sigma)
//   LOG_EI  a = log sigma + log h(u)   c_mu = s Phi(u) / (sigma h(u)) c_v = phi(u) / (2 v h(u))
//   PI      a = Phi(u)                 c_mu = s phi(u) / sigma        c_v = -u phi(u) / (2 v)
//   BOUND   a = s mu + kappa sigma     c_mu = s                       c_v = kappa / (2 sigma)
// and c_v = 0 where the variance was clamped.
// No formula subtracts two close numbers:
//   * Phi(u) = erfc(-u / sqrt 2) / 2 keeps its relative accuracy in the lower tail;
//   * for u < 0, with x = -u and the Mills ratio R(x) = Phi(u) / phi(u) = sqrt(pi / 2) erfcx(x / sqrt 2), h(u) = phi(u) g with
//     g = 1 - x R(x).  That difference is taken as it stands for x < 5 (g(5) = 0.036: at most the factor 1 + u^2 that the
//     conditioning of Phi in u costs anyway); beyond, R and g come from Laplace's continued fraction
//     R = 1 / (x + 1 / (x + 2 / (x + 3 / ...))), g = c / (x + c) with c = 1 / (x + 2 / (x + 3 / ...)): sums of positive terms;
//   * log h(u) = -u^2 / 2 - log sqrt(2 pi) + log g for u < 0: finite and accurate where phi, and EI with it, underflows;
//   * PI's coefficients phi / sigma and u phi / (2 v) are taken from a scaled phi where phi itself is subnormal.
#pragma once
#include <math.h>

#ifndef GPRHIP_ACQ_FN
#define GPRHIP_ACQ_FN __device__ __forceinline__
#endif

namespace gprhip {

enum { ACQ_EI = 0, ACQ_LOG_EI = 1, ACQ_PI = 2, ACQ_BOUND = 3 };  // GPRHIP_ACQ_*

struct AcqPoint {
  double a, cmu, cv;
};

// R(x) and g(x) = 1 - x R(x) for x >= 0
GPRHIP_ACQ_FN void acq_mills(double x, double& R, double& g) {
  if (x < 5.0) {
    R = 1.2533141373155002512 * erfcx(0.70710678118654752440 * x);  // sqrt(pi / 2), 1 / sqrt 2
    g = 1.0 - x * R;
    return;
  }
  // 32 levels reach 2.4e-16 of g at x = 5, 16 levels 5.5e-18 at x = 8 (measured against 50-digit arithmetic)
  const int levels = x < 8.0 ? 32 : 16;
  double t = x;
  for (int k = levels; k >= 2; --k) t = x + (double)k / t;
  const double c = 1.0 / t;
  R = 1.0 / (x + c);
  g = c * R;
}

// var: the variance the criterion sees before the clamp (sigma2 added when predictive)
GPRHIP_ACQ_FN AcqPoint acq_point(int kind, double s, double best, double xi, double kappa, double var_floor, double mu,
                                 double var) {
  const bool clamped = !(var >= var_floor);
  const double v = clamped ? var_floor : var;
  const double sigma = sqrt(v);
  AcqPoint o;
  if (kind == ACQ_BOUND) {
    // s mu + kappa sigma changes sign where the two terms meet: the rounding of the square root and of the product would be
    // the whole of a small sum.  Both are carried along (sqrt(v) - sigma to first order from the exact residual v - sigma^2,
    // the product's and the sum's errors exactly), so that the value is good to a few ulp of itself.
    const double p = kappa * sigma, pe = fma(kappa, sigma, -p);
    const double sl = fma(-sigma, sigma, v) / (2.0 * sigma);
    const double t = s * mu, sum = t + p, bb = sum - t;
    const double se = (t - (sum - bb)) + (p - bb);
    o.a = sum + (se + (pe + kappa * sl));
    o.cmu = s;
    o.cv = clamped ? 0.0 : kappa / (2.0 * sigma);
    return o;
  }
  const double delta = s * (mu - best) - xi;
  const double u = delta / sigma;
  const double inv_sqrt_2pi = 0.39894228040143267794, log_sqrt_2pi = 0.91893853320467274178;
  const double phi = inv_sqrt_2pi * exp(-0.5 * u * u);
  double cv;
  if (kind == ACQ_PI) {
    o.a = 0.5 * erfc(-0.70710678118654752440 * u);
    if (phi < 2.2250738585072014e-308) {
      // phi is subnormal (or 0) for |u| > 37.6, yet its quotients by sigma and by v need not be and must not inherit its
      // few bits: they are formed from 2^128 phi and scaled back, one rounding into the subnormal range at the end
      const double phs = inv_sqrt_2pi * exp(-0.5 * u * u + 88.722839111672999);  // 128 log 2
      o.cmu = s * ldexp(phs / sigma, -128);
      cv = ldexp(-u * phs / (2.0 * v), -128);
    } else {
      o.cmu = s * phi / sigma;
      cv = -u * phi / (2.0 * v);
    }
  } else if (u < 0.0) {
    double R, g;
    acq_mills(-u, R, g);
    if (kind == ACQ_EI) {
      o.a = sigma * (phi * g);
      o.cmu = s * (phi * R);
      cv = phi / (2.0 * sigma);
    } else {
      o.a = log(sigma) + ((-0.5 * u * u - log_sqrt_2pi) + log(g));
      o.cmu = s * R / (sigma * g);
      cv = 1.0 / (2.0 * v * g);
    }
  } else {
    const double Phi = 0.5 * erfc(-0.70710678118654752440 * u);
    const double h = phi + u * Phi;
    if (kind == ACQ_EI) {
      o.a = sigma * h;
      o.cmu = s * Phi;
      cv = phi / (2.0 * sigma);
    } else {
      o.a = log(sigma) + log(h);
      o.cmu = s * Phi / (sigma * h);
      cv = phi / (2.0 * v * h);
    }
  }
  o.cv = clamped ? 0.0 : cv;
  return o;
}

}  // namespace gprhip
