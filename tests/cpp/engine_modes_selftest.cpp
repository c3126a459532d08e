// CPU self-test of the reference and bound code of tools/engine_modes_check.hip (tools/engine_modes_ref.h): an emulated
// launch -- the contract of mfma_gemm.h evaluated in the working precision, k ascending, slice by slice -- passes the
// check; the same launch with one k-term dropped, with beta applied with the wrong sign, or with the second problem of
// a batch stored one window further fails it.  Run by tests/test_engine_modes_ref.py.
//   g++ -O2 -std=c++17 -pthread -I tools tests/cpp/engine_modes_selftest.cpp -o engine_modes_selftest
#include "engine_modes_ref.h"
using namespace emc;

enum Perturb { P_NONE, P_DROP_K, P_BETA_SIGN, P_BATCH_SHIFT, P_TOUCH_LOWER, P_NAN_SKIPPED };

template <typename T>
static Result<T> emulate(const Spec<T>& s, int perturb) {
  Result<T> r;
  r.M = s.M;
  r.ar = s.ar;
  const int BK = sizeof(T) == 8 ? 16 : 32;
  const Win Bw = s.same_ab ? s.A : s.B;
  for (int b = 0; b < s.nbatch; ++b) {
    Win A = s.A, B = Bw, C = s.C;
    A.off += b * s.batch_a; B.off += b * s.batch_b; C.off += b * s.batch_c;
    if (perturb == P_BATCH_SHIFT && b == 1) C.off += s.N;  // one window to the right
    for (int i = 0; i < s.M; ++i)
      for (int j = 0; j < s.N; ++j) {
        const int bm = i / TILE_, bn = j / TILE_;
        if (!tile_runs(s, bm, bn)) {
          if (perturb == P_TOUCH_LOWER && i == s.M - 1 && j == 0) r.ar[C.arena][C.off + (int64_t)i * C.ld + j] = (T)0;
          continue;
        }
        int lo, hi;
        k_range(s, bm, bn, lo, hi);
        if (perturb == P_NAN_SKIPPED && lo > 0 && i == s.M - 1 && j == s.N - 1) lo -= 1;  // reads one element of a skipped block
        const int ks = std::max(1, s.kslices);
        const int gran = s.tri != T_NONE ? TILE_ : BK;
        const int per = ks > 1 ? ((s.K / gran + ks - 1) / ks) * gran : s.K;
        for (int z = 0; z < ks; ++z) {
          const int zlo = std::max(lo, std::min(s.K, z * per)), zhi = std::min(hi, std::min(s.K, z * per + per));
          T acc = 0;
          for (int k = zlo; k < zhi; ++k) {
            if (perturb == P_DROP_K && i == 3 && j == s.N - 1 && k == hi - 1) continue;
            acc += s.ar[A.arena][ia(s, A, i, k)] * s.ar[B.arena][ib(s, B, k, j)];
          }
          const int64_t ic = C.off + (int64_t)z * s.slice_stride + (int64_t)i * C.ld + j;
          T v = (T)s.alpha * acc;
          if (s.beta != 0.0) v += (T)(perturb == P_BETA_SIGN ? -s.beta : s.beta) * s.ar[C.arena][ic];
          r.ar[C.arena][ic] = v;
        }
      }
  }
  return r;
}

template <typename T>
static Spec<T> make(int which) {
  Spec<T> s;
  const int F = 64;
  if (which == 0) {  // NN 2 x 2 tiles, alpha = -1, beta = 1, padded leading dimensions
    s.name = "nn_beta"; s.op = NN; s.M = s.N = 256; s.K = sizeof(T) == 8 ? 48 : 96; s.alpha = -1; s.beta = 1;
    s.A = {0, F, s.K + 4}; s.B = {1, F, s.N + 4}; s.C = {2, F, s.N + 4};
    s.ar.resize(3);
    s.ar[0].assign(F + 256 * (s.K + 4) + F, poison<T>()); s.ar[1].assign(F + s.K * (s.N + 4) + F, poison<T>()); s.ar[2].assign(F + 256 * (s.N + 4) + F, poison<T>());
  } else if (which == 1) {  // batched in-buffer join: NN + KHI_BN, two windows of 128 in 512-wide buffers
    const int mp = 512, sz = 128;
    s.name = "batch_join"; s.op = NN; s.M = s.N = s.K = sz; s.tri = T_KHI_BN; s.nbatch = 2;
    s.batch_a = s.batch_b = s.batch_c = (int64_t)2 * sz * (mp + 1);
    s.A = {0, F + sz, mp}; s.B = {1, F + (int64_t)sz * (mp + 1), mp}; s.C = {2, F + sz, mp};
    s.ar.resize(3);
    for (auto& a : s.ar) a.assign(F + mp * mp + F, poison<T>());
  } else {  // split-K over a triangular k-range, upper tiles only: NT + KLO_MAX, 3 slices of 384
    const int n = 384;
    s.name = "klo_max_upper_splitk"; s.op = NT; s.M = s.N = s.K = n; s.tri = T_KLO_MAX; s.upper = 1; s.kslices = 3; s.slice_stride = (int64_t)n * n;
    s.A = {0, F, n}; s.B = {1, F, n}; s.C = {2, F, n};
    s.ar.resize(3);
    s.ar[0].assign(F + n * n + F, poison<T>()); s.ar[1].assign(F + n * n + F, poison<T>()); s.ar[2].assign(F + 3 * n * n + F, poison<T>());
  }
  fill_operands(s, 7 + which);
  return s;
}

static int g_bad = 0;
template <typename T>
static void expect(int which, int perturb, bool pass, const char* what) {
  Spec<T> s = make<T>(which);
  std::vector<Result<T>> outs;
  outs.push_back(emulate(s, perturb));
  const Verdict vd = check(s, outs, 8);
  const bool ok = vd.ok() == pass;
  printf("selftest %s %s %s: worst=%.3e bad=%ld touched=%ld -> %s, expected %s %s\n", sizeof(T) == 8 ? "f64" : "f32", s.name.c_str(), what,
         vd.worst, vd.bad_entries, vd.touched, vd.ok() ? "passes" : "fails", pass ? "pass" : "fail", ok ? "OK" : "FAIL");
  if (!ok) ++g_bad;
}

template <typename T>
static void all() {
  for (int w = 0; w < 3; ++w) expect<T>(w, P_NONE, true, "unperturbed");
  for (int w = 0; w < 3; ++w) expect<T>(w, P_DROP_K, false, "one k-term dropped");
  expect<T>(0, P_BETA_SIGN, false, "beta with the wrong sign");
  expect<T>(1, P_BATCH_SHIFT, false, "second batch window shifted");
  expect<T>(2, P_TOUCH_LOWER, false, "a tile below the diagonal written");
  expect<T>(2, P_NAN_SKIPPED, false, "one element of a skipped operand block read");
}

int main() {
  all<double>();
  all<float>();
  printf("selftest failed: %d\n", g_bad);
  return g_bad ? 1 : 0;
}
