// Exercises Means::calc_input_gradient / Variances::calc_input_gradient of the C++ mirror (include/gprhip.hpp) on a problem
// dumped by tests/test_gpu_predict_grad.py:
//   predict_grad_check <in.bin>  ->  lines "dmeans v1 v2 ...", "dvariances v1 v2 ..." (D x nt, column-major)
// Input: 4 int64 [n d m nt], then doubles log_ell log_sf2 sigma2 | X (d*n) | y (n) | Z (d*m) | Xt (d*nt), matrices column-major.
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
    std::fprintf(stderr, "usage: predict_grad_check <dump.bin>\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  int64_t dims[4];
  double hy[3];
  f.read(reinterpret_cast<char*>(dims), sizeof(dims));
  f.read(reinterpret_cast<char*>(hy), sizeof(hy));
  const int n = (int)dims[0], d = (int)dims[1], m = (int)dims[2], nt = (int)dims[3];
  auto X = std::make_shared<Mat>(d, n);
  auto Z = std::make_shared<Mat>(d, m);
  auto Xt = std::make_shared<Mat>(d, nt);
  Vec y((size_t)n);
  f.read(reinterpret_cast<char*>(X->data()), sizeof(double) * (size_t)d * n);
  f.read(reinterpret_cast<char*>(y.data()), sizeof(double) * (size_t)n);
  f.read(reinterpret_cast<char*>(Z->data()), sizeof(double) * (size_t)d * m);
  f.read(reinterpret_cast<char*>(Xt->data()), sizeof(double) * (size_t)d * nt);
  if (!f) {
    std::fprintf(stderr, "predict_grad_check: short input file\n");
    return 2;
  }
  try {
    using S = gpr::Cov_se_iso;
    using GP = gpr::Make_deriv<S>;
    using V = GP::FITC;
    auto kernel = S::Kernel::create({hy[0], hy[1]});
    auto inducing = V::Inducing::calc(kernel, Z);
    auto inputs = V::Inputs::calc(inducing, X);
    auto model = V::Model::calc(inputs, hy[2]);
    auto trained = V::Trained::calc(model, y);
    auto tin = V::Inputs::calc(inducing, Xt, /*train=*/false);
    Mat dm = V::Means::calc_input_gradient(trained, tin);
    Mat dv = V::Variances::calc_input_gradient(model, hy[2], tin);
    put("dmeans", dm.data(), (size_t)d * nt);
    put("dvariances", dv.data(), (size_t)d * nt);
  } catch (const gpr::Failure& e) {
    std::fprintf(stderr, "predict_grad_check: %s (status %d)\n", e.what(), e.status);
    return 1;
  }
  return 0;
}
