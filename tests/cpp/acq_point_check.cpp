// acq_point (gpr_amd/csrc/acq_math.h) on the host: reads lines "kind mu var" (mu, var as hexadecimal floats) and prints the
// value and the two coefficients "a c_mu c_v" in hexadecimal floats, for maximise, best = 0, xi = 0, kappa = 0 and
// var_floor = 1e-10.  tests/test_refine_host.py holds PI's coefficients to tests/acquire_ref.py where phi(u) is subnormal
// (37.6 < |u| < 38.6): the band that starts refined out of PI's lower tail cross.
#include <cmath>
#include <cstdio>

namespace gprhip {
// (the device's erfcx; the C library has none.  Only EI and LOG_EI below u = 0 use it.)
inline double erfcx(double x) { return std::exp(x * x) * std::erfc(x); }
}  // namespace gprhip
#define GPRHIP_ACQ_FN inline
#include "../../gpr_amd/csrc/acq_math.h"

int main() {
  int kind;
  double mu, var;
  while (std::scanf("%d %la %la", &kind, &mu, &var) == 3) {
    const gprhip::AcqPoint p = gprhip::acq_point(kind, 1.0, 0.0, 0.0, 0.0, 1e-10, mu, var);
    std::printf("%a %a %a\n", p.a, p.cmu, p.cv);
  }
  return 0;
}
