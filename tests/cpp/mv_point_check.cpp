// mv_point (gpr_amd/csrc/mv_math.h) on the host: reads lines "s var_floor mu var S e_1 ... e_S" (the doubles as hexadecimal
// floats) and prints "a c_mu c_v" in hexadecimal floats.  tests/test_max_value_host.py holds them to tests/max_value_ref.py.
// An argument plants a defect that the test's bounds must catch:
//   naive     psi = gamma lambda / 2 - log Phi as it stands (the two gamma^2 / 2 cancel below gamma = 0)
//   noclamp   c_v not zeroed where the variance was clamped
//   nomean    the 1 / S left out
#include <cmath>
#include <cstdio>
#include <cstring>

namespace gprhip {
// (the device's erfcx; the C library has none.  acq_mills uses it below x = 5.)
inline double erfcx(double x) { return std::exp(x * x) * std::erfc(x); }
}  // namespace gprhip
#define GPRHIP_ACQ_FN inline
#include "../../gpr_amd/csrc/mv_math.h"

namespace {

gprhip::AcqPoint naive_point(double s, double var_floor, double mu, double var, const double* e, int S) {
  const bool clamped = !(var >= var_floor);
  const double v = clamped ? var_floor : var, sigma = std::sqrt(v);
  double a = 0.0, d = 0.0, gd = 0.0;
  for (int j = 0; j < S; ++j) {
    const double gamma = s * (e[j] - mu) / sigma;
    const double Phi = 0.5 * std::erfc(-0.70710678118654752440 * gamma);
    const double lambda = 0.39894228040143267794 * std::exp(-0.5 * gamma * gamma) / Phi;
    const double dpsi = -0.5 * lambda * (1.0 + gamma * (gamma + lambda));
    a += 0.5 * gamma * lambda - std::log(Phi);
    d += dpsi;
    gd += gamma * dpsi;
  }
  gprhip::AcqPoint o;
  o.a = a / S;
  o.cmu = -s * (d / S) / sigma;
  o.cv = clamped ? 0.0 : -(gd / S) / (2.0 * v);
  return o;
}

}  // namespace

int main(int argc, char** argv) {
  const char* const mode = argc > 1 ? argv[1] : "";
  double s, var_floor, mu, var, e[gprhip::MV_MAX_EXTREMES];
  int S;
  while (std::scanf("%la %la %la %la %d", &s, &var_floor, &mu, &var, &S) == 5) {
    if (S < 1 || S > gprhip::MV_MAX_EXTREMES) return 3;
    for (int j = 0; j < S; ++j)
      if (std::scanf("%la", &e[j]) != 1) return 3;
    gprhip::AcqPoint p;
    if (!std::strcmp(mode, "naive")) {
      p = naive_point(s, var_floor, mu, var, e, S);
    } else {
      p = gprhip::mv_point(s, var_floor, mu, var, e, S);
      if (!std::strcmp(mode, "noclamp") && !(var >= var_floor)) p.cv = gprhip::mv_point(s, var_floor, mu, var_floor, e, S).cv;
      if (!std::strcmp(mode, "nomean")) {
        p.a *= S;
        p.cmu *= S;
        p.cv *= S;
      }
    }
    std::printf("%a %a %a\n", p.a, p.cmu, p.cv);
  }
  return 0;
}
