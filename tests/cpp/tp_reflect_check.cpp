// The reflector sequence of gprhip_observe (gpr_amd/csrc/tp_reflect.h, the text the device kernels compile) on the CPU, a
// program of its own for the address and undefined-behaviour sanitizers: the blocked update in double against the same
// update in long double, which is itself held to the definition R'^T R' = R^T R + W^T W and R'^T b' = R^T b + W^T eta.
// Prints, per case and overall, the worst column-wise ratio
//   |dR'[:, c]|_2 / (u |(R[:, c]; W[:, c])|_2)        and the same over (k + 1) (c + 1), the form of the GPU test's bound
// (the b | eta column counts as column mp).  Exact properties are asserted: a positive diagonal, sigma == 0 columns (the
// padding, and planted zero columns of W) left bit for bit, blocked == unblocked in long double to rounding.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../gpr_amd/csrc/tp_reflect.h"

using gprhip::tp_update_blocked;
typedef long double ld;

static int failures = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      ++failures;                                      \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
    }                                                  \
  } while (0)

struct Case {
  const char* name;
  int m, mp, k, nb;
  int extreme;  // 0: none; 1: one pivot of 1e-150 under W entries of 1e150; 2: zero columns of W inside the real part
};

static double worst = 0.0, worst_norm = 0.0;

static void run(const Case& c, unsigned seed) {
  const int m = c.m, mp = c.mp, k = c.k;
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> nrm;
  std::vector<double> R((size_t)mp * mp, 0.0), W((size_t)k * mp, 0.0), b(mp, 0.0), eta(k);
  for (int r = 0; r < mp; ++r)
    for (int col = r; col < mp; ++col)
      R[(size_t)r * mp + col] = (r < m && col < m) ? (r == col ? 1.0 + std::fabs(nrm(gen)) : 0.3 * nrm(gen)) : (r == col ? 1.0 : 0.0);
  for (int i = 0; i < k; ++i) {
    for (int col = 0; col < m; ++col) W[(size_t)i * mp + col] = nrm(gen);
    eta[i] = nrm(gen);
  }
  for (int r = 0; r < m; ++r) b[r] = nrm(gen);
  const int jx = m / 2;
  if (c.extreme == 1) {
    // a tiny pivot under huge entries: the column's own row entries right of the pivot are tiny as well
    for (int col = jx; col < m; ++col) R[(size_t)jx * mp + col] *= 1e-150;
    for (int i = 0; i < k; ++i) W[(size_t)i * mp + jx] = (i < 3 ? 1e150 : 0.0) * (1.0 + 0.1 * i);
  } else if (c.extreme == 2) {
    for (int i = 0; i < k; ++i) W[(size_t)i * mp + jx] = W[(size_t)i * mp + 1] = 0.0;
  }
  std::vector<ld> Rl(R.begin(), R.end()), Wl(W.begin(), W.end()), bl(b.begin(), b.end()), el(eta.begin(), eta.end());
  std::vector<ld> Ru(Rl), Wu(Wl), bu(bl), eu(el);
  const std::vector<double> R0(R), W0(W), b0(b), e0(eta);
  double ldet = 0.0;
  ld ldet_l = 0, ldet_u = 0;
  tp_update_blocked<double>(mp, k, c.nb, R.data(), W.data(), b.data(), eta.data(), &ldet);
  tp_update_blocked<ld>(mp, k, c.nb, Rl.data(), Wl.data(), bl.data(), el.data(), &ldet_l);
  tp_update_blocked<ld>(mp, k, mp, Ru.data(), Wu.data(), bu.data(), eu.data(), &ldet_u);
  // long double: blocked == unblocked (the same operations per column), and the definition
  ld dmax = 0;
  for (size_t i = 0; i < Rl.size(); ++i) dmax = std::fmax(dmax, std::fabs(Rl[i] - Ru[i]));
  for (int r = 0; r < mp; ++r) dmax = std::fmax(dmax, std::fabs(bl[r] - bu[r]));
  CHECK(dmax == 0, "%s: blocked and unblocked differ in long double by %Lg", c.name, dmax);
  std::vector<ld> cn(mp + 1, 0);  // |(R[:, c]; W[:, c])|_2, the b | eta column last
  for (int col = 0; col <= mp; ++col) {
    ld s = 0;
    for (int r = 0; r < mp; ++r) {
      const ld x = col < mp ? (ld)R0[(size_t)r * mp + col] : (ld)b0[r];
      s += x * x;
    }
    for (int i = 0; i < k; ++i) {
      const ld x = col < mp ? (ld)W0[(size_t)i * mp + col] : (ld)e0[i];
      s += x * x;
    }
    cn[col] = sqrtl(s);
  }
  ld def_worst = 0;
  for (int a = 0; a < mp; ++a)
    for (int col = a; col <= mp; ++col) {
      ld lhs = 0, rhs = 0;
      for (int r = 0; r <= a; ++r) {
        lhs += Rl[(size_t)r * mp + a] * (col < mp ? Rl[(size_t)r * mp + col] : bl[r]);
        rhs += (ld)R0[(size_t)r * mp + a] * (col < mp ? (ld)R0[(size_t)r * mp + col] : (ld)b0[r]);
      }
      for (int i = 0; i < k; ++i) rhs += (ld)W0[(size_t)i * mp + a] * (col < mp ? (ld)W0[(size_t)i * mp + col] : (ld)e0[i]);
      if (cn[a] > 0 && cn[col] > 0) def_worst = std::fmax(def_worst, std::fabs(lhs - rhs) / (cn[a] * cn[col]));
    }
  CHECK(def_worst < 1e-16L, "%s: the long double update misses the definition by %Lg of the column norms", c.name, def_worst);
  // exact properties of the double run
  for (int j = 0; j < mp; ++j) {
    CHECK(R[(size_t)j * mp + j] > 0.0, "%s: diagonal %d is %g", c.name, j, R[(size_t)j * mp + j]);
    bool zero_col = true;
    for (int i = 0; i < k; ++i) zero_col = zero_col && W0[(size_t)i * mp + j] == 0.0;
    if (zero_col && (j >= m || c.extreme == 2)) {
      // sigma == 0 (no earlier reflector fills a zero column under a zero row of R: true for the padding; the planted
      // columns are filled by the reflectors left of them, so only the padding is held bit for bit)
      if (j >= m)
        for (int r = 0; r < mp; ++r)
          CHECK(R[(size_t)r * mp + j] == R0[(size_t)r * mp + j], "%s: padded column %d changed in row %d", c.name, j, r);
    }
  }
  for (int r = m; r < mp; ++r) {
    CHECK(b[r] == 0.0, "%s: padded b[%d] = %g", c.name, r, b[r]);
    for (int col = r; col < mp; ++col)
      CHECK(R[(size_t)r * mp + col] == (r == col ? 1.0 : 0.0), "%s: padded row %d changed at column %d", c.name, r, col);
  }
  // the ratios
  const ld u = ldexpl(1.0L, -53);
  double w_case = 0.0, wn_case = 0.0;
  for (int col = 0; col <= mp; ++col) {
    ld e = 0;
    for (int r = 0; r < mp; ++r) {
      const ld dlt = col < mp ? (ld)R[(size_t)r * mp + col] - Rl[(size_t)r * mp + col] : (ld)b[r] - bl[r];
      e += dlt * dlt;
    }
    if (e == 0) continue;
    const double ratio = (double)(sqrtl(e) / (u * cn[col]));
    w_case = std::fmax(w_case, ratio);
    wn_case = std::fmax(wn_case, ratio / ((k + 1.0) * (col + 1.0)));
  }
  ld r2 = 0, r2l = 0;
  for (int i = 0; i < k; ++i) {
    r2 += (ld)eta[i] * eta[i];
    r2l += el[i] * el[i];
  }
  CHECK(std::fabs((double)(r2 - r2l)) <= 1e-12 * (double)(cn[mp] * cn[mp]), "%s: |rho|^2 %Lg against %Lg", c.name, r2, r2l);
  CHECK(std::fabs(ldet - (double)ldet_l) <= 1e-13 * (1.0 + std::fabs((double)ldet_l)) * mp, "%s: log-determinant ratio %.17g against %.17Lg", c.name, ldet, ldet_l);
  std::printf("case %s m %d mp %d k %d nb %d ratio %.4g normalised %.4g\n", c.name, m, mp, k, c.nb, w_case, wn_case);
  worst = std::fmax(worst, w_case);
  worst_norm = std::fmax(worst_norm, wn_case);
}

int main() {
  std::vector<Case> cases;
  const int ms[6] = {50, 64, 65, 128, 129, 300};
  const int ks[3] = {1, 3, 64};
  static char names[64][32];
  int n = 0;
  for (int a = 0; a < 6; ++a)
    for (int q = 0; q < 3; ++q) {
      std::snprintf(names[n], sizeof names[n], "m%d-k%d", ms[a], ks[q]);
      cases.push_back(Case{names[n], ms[a], (ms[a] + 127) / 128 * 128, ks[q], 128, 0});
      ++n;
    }
  cases.push_back(Case{"tiny-pivot-k3", 129, 256, 3, 128, 1});
  cases.push_back(Case{"tiny-pivot-k64", 300, 384, 64, 128, 1});
  cases.push_back(Case{"zero-columns", 129, 256, 3, 128, 2});
  cases.push_back(Case{"small-blocks", 10, 12, 3, 4, 2});
  unsigned seed = 77;
  for (const Case& c : cases) run(c, seed++);
  std::printf("worst ratio %.4g normalised %.4g\n", worst, worst_norm);
  if (failures) {
    std::printf("tp_reflect_check: %d failures\n", failures);
    return 1;
  }
  std::printf("tp_reflect_check: ok\n");
  return 0;
}
