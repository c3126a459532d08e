// The step rule of gprhip_acquire_refine (gpr_amd/csrc/refine_step.h) on analytic objectives, on the host: a program of its
// own, built with -fsanitize=address,undefined by tests/test_refine_host.py.  It drives the header's serial functions exactly
// as refine_step_kernel does -- refine_begin after the evaluation at the clipped start, refine_advance after every trial --
// asserts status, maximiser, monotone accepted values and the evaluation count per case, and prints every trace record in
// hexadecimal floats: the test holds tests/refine_ref.py to them step for step.
//   quadratic  -sum c_k (x_k - m_k)^2 with m inside the box, beyond one face, beyond a corner;  linear b . x;  a constant;
//   a NaN plateau: the quadratic where x_0 <= 0.6, NaN beyond
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define GPRHIP_REFINE_FN inline
#include "../../gpr_amd/csrc/refine_step.h"

using namespace gprhip;

namespace {

constexpr int D = 2;
const double LO[D] = {0.0, -1.0}, HI[D] = {1.0, 1.0};

struct Objective {
  std::string name;
  int kind;  // 0 quadratic, 1 linear, 2 constant, 3 quadratic with a NaN plateau
  double c[D], m[D];
};

double eval(const Objective& f, const double* x, double* g) {
  if (f.kind == 1) {
    double a = 0.0;
    for (int k = 0; k < D; ++k) {
      a += f.c[k] * x[k];
      g[k] = f.c[k];
    }
    return a;
  }
  if (f.kind == 2) {
    for (int k = 0; k < D; ++k) g[k] = 0.0;
    return 1.5;
  }
  double s = 0.0;
  for (int k = 0; k < D; ++k) {
    const double t = x[k] - f.m[k];
    s += f.c[k] * t * t;
    g[k] = -2.0 * f.c[k] * t;
  }
  if (f.kind == 3 && x[0] > 0.6) {
    for (int k = 0; k < D; ++k) g[k] = NAN;
    return NAN;
  }
  return -s;
}

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "refine_step_check: %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, what.c_str()); \
      std::exit(1);                                                                      \
    }                                                                                    \
  } while (0)

struct Run {
  std::vector<double> x, g;
  RefineStart st;
};

Run run(const Objective& f, const double* start, const double* scale, const RefineOpts& o, const std::string& what) {
  Run r;
  r.x.assign(D, 0.0);
  r.g.assign(D, 0.0);
  std::vector<double> y(D), gy(D);
  for (int k = 0; k < D; ++k) r.x[k] = y[k] = refine_clip(start[k], LO[k], HI[k]);
  double ay = eval(f, y.data(), gy.data());
  r.g = gy;
  auto record = [&](const double* py, double alpha, bool acc) {
    std::printf("rec");
    for (int k = 0; k < D; ++k) std::printf(" %a", py[k]);
    for (int k = 0; k < D; ++k) std::printf(" %a", gy[k]);
    std::printf(" %a %a %d\n", ay, alpha, acc ? 1 : 0);
  };
  std::printf("case %s\n", what.c_str());
  record(y.data(), 0.0, true);
  refine_begin(D, r.x.data(), r.g.data(), ay, LO, HI, scale, o, r.st, y.data());
  double last = r.st.a;
  int evals = 1, accepted = 0;
  while (r.st.status == REFINE_ACTIVE) {
    CHECK(evals < o.max_evals);
    for (int k = 0; k < D; ++k) CHECK(y[k] >= LO[k] && y[k] <= HI[k]);
    ay = eval(f, y.data(), gy.data());
    ++evals;
    const std::vector<double> at = y;
    const double alpha = r.st.alpha;
    const bool acc = refine_advance(D, r.x.data(), r.g.data(), y.data(), gy.data(), ay, LO, HI, scale, o, r.st);
    record(at.data(), alpha, acc);
    if (acc) {
      ++accepted;
      CHECK(r.st.a >= last);  // monotone over accepted steps (c1 >= 0)
      CHECK(r.st.a == ay && r.x == at && r.g == gy);
      last = r.st.a;
    }
  }
  CHECK(r.st.evals == evals && r.st.accepted == accepted && evals <= o.max_evals);
  std::printf("end %d %d %d", r.st.status, r.st.evals, r.st.accepted);
  for (int k = 0; k < D; ++k) std::printf(" %a", r.x[k]);
  std::printf(" %a\n", r.st.a);
  return r;
}

}  // namespace

int main() {
  // (xtol stays above sqrt(2^-53): where the optimum's value is not 0, Armijo's test cannot tell points closer than that apart)
  const RefineOpts o{400, 0.25, 1e-4, 0.5, 2.0, 1e-6};
  const double starts[][D] = {{0.1, -0.9}, {0.95, 0.7}, {0.5, 0.0}, {-3.0, 5.0}};  // the last one lies outside the box
  const double scale[D] = {1.0, 0.5};  // (it makes the anisotropic quadratic isotropic)
  const Objective inside{"inside", 0, {1.0, 1.0}, {0.3, 0.4}}, aniso{"aniso", 0, {1.0, 2.0}, {0.3, 0.4}};
  const Objective face{"face", 0, {1.0, 1.0}, {1.7, 0.25}}, corner{"corner", 0, {1.0, 2.0}, {-0.5, 1.5}};
  const Objective linear{"linear", 1, {0.7, -0.2}, {0.0, 0.0}}, constant{"constant", 2, {0.0, 0.0}, {0.0, 0.0}};
  const Objective plateau{"plateau", 3, {1.0, 1.0}, {0.3, 0.4}};
  struct Case {
    const Objective* f;
    double want[D];
  };
  const Case cases[] = {{&inside, {0.3, 0.4}}, {&aniso, {0.3, 0.4}}, {&face, {1.0, 0.25}}, {&corner, {0.0, 1.0}},
                        {&linear, {1.0, -1.0}}};
  for (const Case& c : cases)
    for (int si = 0; si < 4; ++si)
      for (int sc = 0; sc < 2; ++sc) {
        const std::string what = c.f->name + "." + std::to_string(si) + (sc ? ".scaled" : "");
        const Run r = run(*c.f, starts[si], sc ? scale : nullptr, o, what);
        CHECK(r.st.status == REFINE_CONVERGED);
        // The maximiser to xtol w.  The rule ends on the size of a step, alpha |dir_k| <= xtol w_k, and on a quadratic
        // dir_k = 2 s_k c_k (m_k - x_k); every alpha <= (1 - c1) / max_j s_j c_j passes Armijo's test there, so after a
        // rejection alpha >= shrink (1 - c1) / max_j s_j c_j, and |x_k - m_k| <= xtol w_k max_j s_j c_j / ((1 - c1) s_k c_k):
        // xtol w_k itself where all s_k c_k are equal (up to 1 / (1 - c1), which these cases do not use up), that multiple
        // of it on the anisotropic ones.
        double sck[D], mx = 0.0;
        for (int k = 0; k < D; ++k) mx = std::fmax(mx, sck[k] = (sc ? scale[k] : 1.0) * c.f->c[k]);
        for (int k = 0; k < D; ++k) {
          const double factor = (c.f->kind != 0 || sck[k] == mx) ? 1.0 : mx / ((1.0 - o.c1) * sck[k]);
          CHECK(std::fabs(r.x[k] - c.want[k]) <= factor * o.xtol * (HI[k] - LO[k]));
        }
      }
  {  // a constant: no step on a zero gradient
    const std::string what = "constant.0";
    const Run r = run(constant, starts[0], nullptr, o, what);
    CHECK(r.st.status == REFINE_CONVERGED && r.st.evals == 1 && r.st.accepted == 0);
    CHECK(r.x[0] == starts[0][0] && r.x[1] == starts[0][1] && r.st.a == 1.5);
  }
  {  // the NaN plateau: trials into it are rejected, a start inside it is NAN
    const RefineOpts big{200, 1.0, 1e-4, 0.5, 2.0, 1e-6};
    std::string what = "plateau.0";
    const Run r = run(plateau, starts[0], nullptr, big, what);
    CHECK(r.st.status == REFINE_CONVERGED && r.st.evals > r.st.accepted + 1);
    for (int k = 0; k < D; ++k) CHECK(std::fabs(r.x[k] - plateau.m[k]) <= big.xtol * (HI[k] - LO[k]));
    what = "plateau.1";
    const Run n = run(plateau, starts[1], nullptr, big, what);
    CHECK(n.st.status == REFINE_NAN && n.st.evals == 1 && n.st.accepted == 0 && n.x[0] == 0.95);
  }
  {  // max_evals = 1: the clipped start; and evaluations that run out
    const RefineOpts one{1, 0.25, 1e-4, 0.5, 2.0, 1e-6};
    std::string what = "one.3";
    const Run r = run(inside, starts[3], nullptr, one, what);
    CHECK(r.st.status == REFINE_MAX_EVALS && r.st.evals == 1 && r.x[0] == 0.0 && r.x[1] == 1.0);
    const RefineOpts few{4, 0.25, 1e-4, 0.5, 2.0, 1e-6};
    what = "few.0";
    const Run q = run(aniso, starts[0], nullptr, few, what);
    CHECK(q.st.status == REFINE_MAX_EVALS && q.st.evals == 4);
  }
  std::printf("refine_step_check: ok\n");
  return 0;
}
