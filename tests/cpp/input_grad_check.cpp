// Exercises gpr::Make_deriv<Cov_se_iso>::run_input_grad (include/gprhip.hpp) on a problem dumped by
// tests/test_gpu_input_grad.py:
//   input_grad_check <in.bin>  ->  lines "l v", "trained v1 v2 ..." (D x n, column-major), "l1 v", "model v1 v2 ..."
// Input: 3 int64 [n d m], then doubles log_ell log_sf2 sigma2 | X (d*n) | y (n) | Z (d*m), matrices column-major.
#include <cstdio>
#include <fstream>

#include "gprhip.hpp"

using gpr::Mat;
using gpr::Vec;

static void put(const char* key, const double* v, size_t n) {
  std::printf("%s", key);
  for (size_t i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: input_grad_check <dump.bin>\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  int64_t dims[3];
  double hy[3];
  f.read(reinterpret_cast<char*>(dims), sizeof(dims));
  f.read(reinterpret_cast<char*>(hy), sizeof(hy));
  const int n = (int)dims[0], d = (int)dims[1], m = (int)dims[2];
  auto X = std::make_shared<Mat>(d, n);
  auto Z = std::make_shared<Mat>(d, m);
  Vec y((size_t)n);
  f.read(reinterpret_cast<char*>(X->data()), sizeof(double) * (size_t)d * n);
  f.read(reinterpret_cast<char*>(y.data()), sizeof(double) * (size_t)n);
  f.read(reinterpret_cast<char*>(Z->data()), sizeof(double) * (size_t)d * m);
  if (!f) {
    std::fprintf(stderr, "input_grad_check: short input file\n");
    return 2;
  }
  try {
    using S = gpr::Cov_se_iso;
    using GP = gpr::Make_deriv<S>;
    using V = GP::FITC;
    auto kernel = S::Kernel::create({hy[0], hy[1]});
    auto inputs = V::Inputs::calc(V::Inducing::calc(kernel, Z), X);
    auto model = V::Model::calc(inputs, hy[2]);
    Mat g;
    gpr::Evaluation ev = GP::run_input_grad(model, &y, g, model.id);
    put("l", &ev.l, 1);
    put("trained", g.data(), (size_t)d * n);
    ev = GP::run_input_grad(model, nullptr, g, model.id);  // (the same kernel and inducing points: V is reused)
    put("l1", &ev.l1, 1);
    put("model", g.data(), (size_t)d * n);
  } catch (const gpr::Failure& e) {
    std::fprintf(stderr, "input_grad_check: %s (status %d)\n", e.what(), e.status);
    return 1;
  }
  return 0;
}
