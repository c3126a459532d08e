// Exercises Path_sampler::refine of the C++ mirror (include/gprhip.hpp) on a small model of its own:
//   path_refine_check run  ->  lines "values ...", "x ..." (D x ns, column-major), "status ...", "evals ..."
// n = 200 points of sin(3 x0) cos(2 x1) in [0, 1]^2, m = 20 inducing points, 2 draws refined from ns = 6 starts.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "gprhip.hpp"

using gpr::Mat;
using gpr::Vec;

static void put(const char* key, const double* v, size_t n) {
  std::printf("%s", key);
  for (size_t i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2 || std::strcmp(argv[1], "run") != 0) {
    std::fprintf(stderr, "usage: path_refine_check run\n");
    return 2;
  }
  const int n = 200, d = 2, m = 20, ns = 6, nd = 2;
  auto X = std::make_shared<Mat>(d, n);
  auto Z = std::make_shared<Mat>(d, m);
  auto S0 = std::make_shared<Mat>(d, ns);
  Vec y((size_t)n);
  unsigned long long state = 12345;
  auto uni = [&] {  // a linear congruential generator: the same points every run
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  for (int i = 0; i < n; ++i) {
    const double a = uni(), b = uni();
    X->data()[(size_t)i * d] = a;
    X->data()[(size_t)i * d + 1] = b;
    y[(size_t)i] = std::sin(3.0 * a) * std::cos(2.0 * b);
  }
  for (int i = 0; i < d * m; ++i) Z->data()[i] = uni();
  for (int i = 0; i < d * ns; ++i) S0->data()[i] = uni();
  Mat z(m, nd);
  for (int i = 0; i < m * nd; ++i) z.data()[i] = 2.0 * uni() - 1.0;
  try {
    using S = gpr::Cov_se_iso;
    using GP = gpr::Make_deriv<S>;
    using V = GP::FITC;
    auto kernel = S::Kernel::create({std::log(0.4), 0.0});
    auto inducing = V::Inducing::calc(kernel, Z);
    auto inputs = V::Inputs::calc(inducing, X);
    auto model = V::Model::calc(inputs, 1e-3);
    auto trained = V::Trained::calc(model, y);
    auto tin = V::Inputs::calc(inducing, S0, /*train=*/false);
    const gprhip_refine_options opt{40, 0.1, 1e-4, 0.5, 2.0, 1e-8};
    const Vec lower{0.0, 0.0}, upper{1.0, 1.0};
    auto sampler = V::Path_sampler::calc(trained, z);
    auto r = V::Path_sampler::refine(sampler, tin, {0, 1, 0, 1, 0, 1}, opt, lower, upper);
    put("values", r.values.data(), r.values.size());
    put("x", r.x.data(), (size_t)d * ns);
    Vec st(r.status.begin(), r.status.end()), ev(r.evals.begin(), r.evals.end());
    put("status", st.data(), st.size());
    put("evals", ev.data(), ev.size());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "path_refine_check: %s\n", e.what());
    return 1;
  }
  return 0;
}
