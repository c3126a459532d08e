// Max-value entropy search (gprhip_acquire_max_value) at one test point: from the predictive mean mu and variance, the direction
// s = +-1 and the extreme values e_j (j < S) of S drawn paths, with v = max(variance, var_floor), sigma = sqrt(v),
//   gamma_j = s (e_j - mu) / sigma,  lambda = phi / Phi,
//   psi(gamma)  = gamma lambda / 2 - log Phi(gamma)           (> 0, decreasing)
//   psi'(gamma) = -(lambda / 2) (1 + gamma (gamma + lambda))
//   a = (1 / S) sum_j psi(gamma_j),  c_mu = da/dmu = (1 / S) sum_j psi'(gamma_j) (-s / sigma),
//   c_v = da/dsigma2 = (1 / S) sum_j psi'(gamma_j) (-gamma_j / (2 v)), 0 where the variance was clamped.
// No formula subtracts two close numbers.  With R, g of acq_mills (acq_math.h) at x = |gamma|:
//   * gamma < 0: lambda = 1 / R, log Phi = -x^2 / 2 - log sqrt(2 pi) + log R, so psi = log sqrt(2 pi) - log R - x g / (2 R) -- the
//     two x^2 / 2 have gone --, and 1 + gamma (gamma + lambda) = 1 - x g / R: psi' = -(1 - x g / R) / (2 R);
//   * gamma >= 0: the upper tail q = 1 - Phi = phi R, and psi = phi (gamma / (2 Phi) + R L) with L = -log(1 - q) / q >= 1: both
//     terms positive, and psi keeps its relative accuracy where it is tiny.
// psi and psi' fall below the normal range with phi (gamma > 37.6), yet a quotient by sigma or v need not: every term is carried
// times 2^128 -- phi 2^128 = (exp(-gamma^2 / 4) 2^64)^2 / sqrt(2 pi) --, and the three results are scaled back at the end, one
// rounding into the subnormal range.  (|gamma| beyond 1e130 overflows for that: psi ~ gamma^2 / 2.)
// A point's sums are split into partial sums (mv_accumulate: every `step`-th extreme from `first`) that the caller joins in an
// order of its own; mv_finish scales the joined sums.  The kernels give the four lanes of a test point one partial sum each.
#pragma once
#include "acq_math.h"

namespace gprhip {

constexpr int MV_MAX_EXTREMES = 64;  // GPRHIP_MAX_EXTREMES

struct MvSums {
  double psi, dpsi, gdpsi;  // 2^128 times the sums of psi(gamma_j), psi'(gamma_j), gamma_j psi'(gamma_j)
};

// 2^128 psi and 2^128 psi' at gamma
GPRHIP_ACQ_FN void mv_psi(double gamma, double& psi, double& dpsi) {
  const double inv_sqrt_2pi = 0.39894228040143267794, log_sqrt_2pi = 0.91893853320467274178;
  const double two128 = 3.4028236692093846346e38, two64 = 18446744073709551616.0;
  double R, g;
  if (gamma < 0.0) {
    const double x = -gamma;
    acq_mills(x, R, g);
    const double xg = x * g / R;
    psi = two128 * ((log_sqrt_2pi - log(R)) - 0.5 * xg);
    dpsi = two128 * (-(1.0 - xg) / (2.0 * R));
  } else {
    acq_mills(gamma, R, g);
    const double eh = two64 * exp(-0.25 * gamma * gamma);
    const double phs = inv_sqrt_2pi * (eh * eh);  // 2^128 phi
    const double q = ldexp(phs, -128) * R;        // 1 - Phi <= 1 / 2 (its own accuracy matters only while it is not tiny)
    const double Phi = 1.0 - q;
    const double L = q < 1e-4 ? 1.0 + q * (0.5 + q * (1.0 / 3.0 + 0.25 * q)) : -log1p(-q) / q;
    const double lams = phs / Phi;                // 2^128 lambda
    psi = phs * (0.5 * gamma / Phi + R * L);
    dpsi = -0.5 * lams * (1.0 + gamma * (gamma + ldexp(lams, -128)));
  }
}

// the part of a point's three sums that the extremes first, first + step, ... < S make up, in that order
GPRHIP_ACQ_FN MvSums mv_accumulate(const double* extremes, int S, int first, int step, double s, double mu, double sigma) {
  MvSums o{0.0, 0.0, 0.0};
  for (int j = first; j < S; j += step) {
    const double gamma = s * (extremes[j] - mu) / sigma;
    double psi, dpsi;
    mv_psi(gamma, psi, dpsi);
    o.psi += psi;
    o.dpsi += dpsi;
    o.gdpsi += gamma * dpsi;
  }
  return o;
}

GPRHIP_ACQ_FN AcqPoint mv_finish(const MvSums& t, int S, double s, double sigma, double v, bool clamped) {
  const double n = (double)S;
  AcqPoint o;
  o.a = ldexp(t.psi / n, -128);
  o.cmu = ldexp(-s * (t.dpsi / n) / sigma, -128);
  o.cv = clamped ? 0.0 : ldexp(-(t.gdpsi / n) / (2.0 * v), -128);
  return o;
}

// the whole point in the kernels' order: four partial sums (every fourth extreme), joined as (0 + 1) + (2 + 3)
// var: the variance before the clamp
GPRHIP_ACQ_FN AcqPoint mv_point(double s, double var_floor, double mu, double var, const double* extremes, int S) {
  const bool clamped = !(var >= var_floor);
  const double v = clamped ? var_floor : var;
  const double sigma = sqrt(v);
  MvSums p[4];
  for (int l = 0; l < 4; ++l) p[l] = mv_accumulate(extremes, S, l, 4, s, mu, sigma);
  MvSums t;
  t.psi = (p[0].psi + p[1].psi) + (p[2].psi + p[3].psi);
  t.dpsi = (p[0].dpsi + p[1].dpsi) + (p[2].dpsi + p[3].dpsi);
  t.gdpsi = (p[0].gdpsi + p[1].gdpsi) + (p[2].gdpsi + p[3].gdpsi);
  return mv_finish(t, S, s, sigma, v, clamped);
}

}  // namespace gprhip
