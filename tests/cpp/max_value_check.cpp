// Exercises Acquisition::calc_max_value of the C++ mirror (include/gprhip.hpp) on a problem dumped by
// tests/test_gpu_max_value.py:
//   max_value_check <in.bin>  ->  lines "values v1 ...", "dvalues ..." (D x nt, column-major), "top_index ...", "top_values ...",
//                                 "top_dvalues ..." (D x top_k)
// Input: 6 int64 [n d m nt top_k S], then doubles log_ell log_sf2 sigma2 | maximise var_floor | extremes (S) |
// X (d*n) | y (n) | Z (d*m) | Xt (d*nt), matrices column-major.
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
    std::fprintf(stderr, "usage: max_value_check <dump.bin>\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  int64_t dims[6];
  double hy[3], mv[2];
  f.read(reinterpret_cast<char*>(dims), sizeof(dims));
  f.read(reinterpret_cast<char*>(hy), sizeof(hy));
  f.read(reinterpret_cast<char*>(mv), sizeof(mv));
  if (!f || dims[5] < 0 || dims[5] > 1024) {
    std::fprintf(stderr, "max_value_check: short input file\n");
    return 2;
  }
  const int n = (int)dims[0], d = (int)dims[1], m = (int)dims[2], nt = (int)dims[3], top_k = (int)dims[4];
  Vec extremes((size_t)dims[5]);
  auto X = std::make_shared<Mat>(d, n);
  auto Z = std::make_shared<Mat>(d, m);
  auto Xt = std::make_shared<Mat>(d, nt);
  Vec y((size_t)n);
  f.read(reinterpret_cast<char*>(extremes.data()), sizeof(double) * extremes.size());
  f.read(reinterpret_cast<char*>(X->data()), sizeof(double) * (size_t)d * n);
  f.read(reinterpret_cast<char*>(y.data()), sizeof(double) * (size_t)n);
  f.read(reinterpret_cast<char*>(Z->data()), sizeof(double) * (size_t)d * m);
  f.read(reinterpret_cast<char*>(Xt->data()), sizeof(double) * (size_t)d * nt);
  if (!f) {
    std::fprintf(stderr, "max_value_check: short input file\n");
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
    auto a = V::Acquisition::calc_max_value(trained, tin, extremes, mv[0] != 0.0, mv[1], top_k);
    put("values", a.values.data(), (size_t)nt);
    put("dvalues", a.dvalues.data(), (size_t)d * nt);
    Vec idx(a.top_index.begin(), a.top_index.end());
    put("top_index", idx.data(), idx.size());
    put("top_values", a.top_values.data(), a.top_values.size());
    put("top_dvalues", a.top_dvalues.data(), (size_t)d * top_k);
  } catch (const gpr::Failure& e) {
    std::fprintf(stderr, "max_value_check: %s (status %d)\n", e.what(), e.status);
    return 1;
  }
  return 0;
}
