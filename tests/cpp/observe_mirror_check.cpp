// Observe::observe / save / restore / count of include/gprhip.hpp (the C++ mirror) on a small synthetic problem:
//   observe_mirror_check run  ->  "observe_mirror_check: ok" (tests/test_gpu_observe_surfaces.py); without arguments the usage.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "gprhip.hpp"

using gpr::Mat;
using gpr::Vec;

static int failures = 0;
#define CHECK(c, what)                         \
  do {                                         \
    if (!(c)) {                                \
      ++failures;                              \
      std::printf("FAIL line %d: %s\n", __LINE__, what); \
    }                                          \
  } while (0)

static double unit(unsigned& s) {
  s = s * 1664525u + 1013904223u;
  return (double)(s >> 8) / (double)(1u << 24) * 2.0 - 1.0;
}

static bool same_bits(const Vec& a, const Vec& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: observe_mirror_check run\n");
    return 2;
  }
  using S = gpr::Cov_se_iso;
  using V = gpr::Make_deriv<S>::FITC;
  const int n = 200, m = 30, d = 2, nt = 20, k = 3;
  unsigned seed = 12345u;
  auto X = std::make_shared<Mat>(d, n), Z = std::make_shared<Mat>(d, m), Xt = std::make_shared<Mat>(d, nt), Xn = std::make_shared<Mat>(d, k);
  Vec y((size_t)n), yn((size_t)k);
  auto f = [](const double* p) { return std::sin(2.0 * p[0]) + 0.5 * p[1]; };
  for (int i = 0; i < n; ++i) {
    for (int b = 0; b < d; ++b) X->data()[(size_t)i * d + b] = unit(seed);
    y[(size_t)i] = f(X->data() + (size_t)i * d) + 0.05 * unit(seed);
  }
  for (int i = 0; i < m; ++i)
    for (int b = 0; b < d; ++b) Z->data()[(size_t)i * d + b] = X->data()[(size_t)(i * 6) * d + b] + 0.01 * unit(seed);
  for (int i = 0; i < nt; ++i)
    for (int b = 0; b < d; ++b) Xt->data()[(size_t)i * d + b] = 0.9 * unit(seed);
  for (int i = 0; i < k; ++i) {
    for (int b = 0; b < d; ++b) Xn->data()[(size_t)i * d + b] = 0.8 * unit(seed);
    yn[(size_t)i] = f(Xn->data() + (size_t)i * d) + 1.0;  // (off the surface: the posterior must move)
  }
  try {
    auto kernel = S::Kernel::create({std::log(0.4), 0.0});
    auto inducing = V::Inducing::calc(kernel, Z);
    auto inputs = V::Inputs::calc(inducing, X);
    auto model = V::Model::calc(inputs, 0.05);
    auto trained = V::Trained::calc(model, y);
    auto tin = V::Inputs::calc(inducing, Xt, /*train=*/false);
    auto nin = V::Inputs::calc(inducing, Xn, /*train=*/false);
    const Vec before = V::Means::calc(trained, tin);
    CHECK(V::Observe::count(trained) == 0, "count before");
    V::Observe::save(trained);
    const double dl = V::Observe::observe(trained, nin, yn);
    CHECK(std::isfinite(dl) && dl < 0.0, "dlog_evidence of targets one unit off the surface");
    CHECK(V::Observe::count(trained) == k, "count after observe");
    const Vec after = V::Means::calc(trained, tin);
    double moved = 0.0;
    for (size_t i = 0; i < after.size(); ++i) moved = std::fmax(moved, std::fabs(after[i] - before[i]));
    CHECK(moved > 1e-3, "the conditioned means differ");
    V::Observe::restore(trained);
    CHECK(V::Observe::count(trained) == 0, "count after restore");
    CHECK(same_bits(V::Means::calc(trained, tin), before), "restore gives the bits back");
    // a model: factors only, no targets
    const auto v0 = V::Variances::get(V::Variances::calc(model, 0.05, tin), false);
    const double dl1 = V::Observe::observe(model, nin);
    const auto v1 = V::Variances::get(V::Variances::calc(model, 0.05, tin), false);
    bool shrank = true, some = false;
    for (size_t i = 0; i < v0.size(); ++i) {
      shrank = shrank && v1[i] <= v0[i] * (1.0 + 1e-12);
      some = some || v1[i] < v0[i] * (1.0 - 1e-6);
    }
    CHECK(std::isfinite(dl1) && shrank && some, "observing without targets shrinks the variances");
    std::printf("dl %.17g dl1 %.17g moved %.3g\n", dl, dl1, moved);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  if (failures) return 1;
  std::printf("observe_mirror_check: ok\n");
  return 0;
}
