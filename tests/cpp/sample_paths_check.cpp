// Stand-alone check of the host-side pieces of gprhip_sample_paths (gpr_amd/csrc/sample_paths_host.h): every argument
// refusal, and the cross-chunk merge of the per-draw best-k lists against a stable sort of all values.  No device, no
// library: built with -fsanitize=address,undefined and run on the CPU by tests/test_sample_paths_host.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../gpr_amd/csrc/sample_paths_host.h"

using namespace gprhip;

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);             \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static SpCall good_call(const double* buf, const int64_t* idx) {
  SpCall c;
  c.have_p = 1; c.D = 3; c.d = 3; c.m = 5; c.f32 = 0;
  c.z = buf; c.ldz = 5; c.ns = 4; c.test_inputs = buf; c.ld = 3; c.nt = 7;
  c.eps = buf; c.lde = 7; c.samples = buf; c.lds = 7; c.top_k = 2; c.top_index = idx; c.on_device = 0;
  return c;
}

static bool refused(const SpCall& c, const char* word) {
  const char* why = sp_check_args(c);
  return why && std::strstr(why, word);
}

static void check_args() {
  double buf[64] = {0};
  int64_t idx[8] = {0};
  SpCall c = good_call(buf, idx);
  EXPECT(sp_check_args(c) == nullptr);
  { SpCall b = c; b.ns = 0; EXPECT(refused(b, "ns")); }
  { SpCall b = c; b.ns = 65; EXPECT(refused(b, "ns")); }
  { SpCall b = c; b.ns = 64; EXPECT(sp_check_args(b) == nullptr); }
  { SpCall b = c; b.top_k = -1; EXPECT(refused(b, "top_k")); }
  { SpCall b = c; b.top_k = 65; EXPECT(refused(b, "top_k")); }
  { SpCall b = c; b.top_index = nullptr; EXPECT(refused(b, "top_index")); }
  { SpCall b = c; b.samples = nullptr; b.top_k = 0; EXPECT(refused(b, "nothing is requested")); }
  { SpCall b = c; b.samples = nullptr; EXPECT(sp_check_args(b) == nullptr); }
  { SpCall b = c; b.have_p = 0; EXPECT(refused(b, "invalid arguments")); }
  { SpCall b = c; b.z = nullptr; EXPECT(refused(b, "invalid arguments")); }
  { SpCall b = c; b.test_inputs = nullptr; EXPECT(refused(b, "invalid arguments")); }
  { SpCall b = c; b.nt = 0; EXPECT(refused(b, "invalid arguments")); }
  { SpCall b = c; b.f32 = 1; EXPECT(refused(b, "fp64 only")); }
  { SpCall b = c; b.d = 65; EXPECT(refused(b, "64 point dimensions")); }
  { SpCall b = c; b.ldz = 4; EXPECT(refused(b, "ldz")); }
  { SpCall b = c; b.ld = 2; EXPECT(refused(b, "bad ld ")); }
  { SpCall b = c; b.ld = 4; EXPECT(sp_check_args(b) == nullptr); }
  { SpCall b = c; b.ld = 4; b.on_device = 1; EXPECT(refused(b, "bad ld ")); }
  { SpCall b = c; b.lde = 6; EXPECT(refused(b, "lde")); }
  { SpCall b = c; b.lde = 6; b.eps = nullptr; EXPECT(sp_check_args(b) == nullptr); }
  { SpCall b = c; b.lds = 6; EXPECT(refused(b, "lds")); }
  { SpCall b = c; b.lds = 6; b.samples = nullptr; EXPECT(sp_check_args(b) == nullptr); }
}

// the chunk's own sorted best-k list, as the device leaves it: [k] indices as doubles (-1 fill), [k] values, [k][D] rows
static void chunk_list(const std::vector<double>& v, int lo, int rows, int k, double sign, int D, std::vector<double>& blk) {
  std::vector<int> order;
  for (int i = 0; i < rows; ++i)
    if (!std::isnan(v[lo + i])) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sign * v[lo + a] > sign * v[lo + b]; });
  blk.assign((size_t)k * (D + 2), 0.0);
  for (int j = 0; j < k; ++j) {
    const bool have = j < (int)order.size();
    blk[j] = have ? order[j] : -1.0;
    blk[k + j] = have ? v[lo + order[j]] : 0.0;
    for (int b = 0; b < D; ++b) blk[2 * k + (size_t)j * D + b] = have ? 1000.0 * (lo + order[j]) + b : 0.0;
  }
}

static void check_merge() {
  std::mt19937 gen(7);
  for (int trial = 0; trial < 200; ++trial) {
    const int n = 1 + (int)(gen() % 90), chunk = 1 + (int)(gen() % 40), k = 1 + (int)(gen() % 64), D = (int)(gen() % 4);
    const double sign = (trial & 1) ? -1.0 : 1.0;
    std::vector<double> v(n);
    for (auto& x : v) {
      const unsigned r = gen() % 16;                      // few distinct values: many ties; some NaN, +0 and -0
      x = r == 0 ? std::nan("") : r == 1 ? 0.0 : r == 2 ? -0.0 : (double)(r % 7) - 3.0;
    }
    SpBest best;
    std::vector<double> blk;
    for (int lo = 0; lo < n; lo += chunk) {
      const int rows = std::min(chunk, n - lo);
      chunk_list(v, lo, rows, k, sign, D, blk);
      sp_merge_topk(best, k, sign, blk.data(), blk.data() + k, D ? blk.data() + 2 * k : nullptr, D, lo);
    }
    std::vector<int> order;
    for (int i = 0; i < n; ++i)
      if (!std::isnan(v[i])) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sign * v[a] > sign * v[b]; });
    const size_t want = std::min<size_t>(k, order.size());
    EXPECT(best.idx.size() == want && best.val.size() == want);
    EXPECT(best.grad.size() == (D ? want * D : 0));
    for (size_t j = 0; j < want && j < best.idx.size(); ++j) {
      EXPECT(best.idx[j] == order[j]);
      EXPECT(std::memcmp(&best.val[j], &v[order[j]], sizeof(double)) == 0);
      for (int b = 0; b < D; ++b) EXPECT(best.grad[j * D + b] == 1000.0 * order[j] + b);
    }
  }
}

int main() {
  check_args();
  check_merge();
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("sample_paths_check: ok\n");
  return 0;
}
