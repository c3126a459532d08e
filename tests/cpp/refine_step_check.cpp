// The step rule of gprhip_acquire_refine (gpr_amd/csrc/refine_step.h) on analytic objectives, on the host: a program of its
// own, built with -fsanitize=address,undefined by tests/test_refine_host.py.  It runs refine_step_start -- the function that
// refine_step_kernel and path_refine_kernel call per start -- on [ns][D] arrays of its own: an evaluation at the clipped
// start, then one after every trial.  It asserts status, maximiser, monotone accepted values and the evaluation count per
// case, and prints every record of the trace array and the end state of the state arrays in hexadecimal floats: the test
// holds tests/refine_ref.py to them step for step.  Four starts in one set of arrays must give what each gives alone, and a
// start that has ended is not touched again.
//   quadratic  -sum c_k (x_k - m_k)^2 with m inside the box, beyond one face, beyond a corner;  linear b . x;  a constant;
//   a NaN plateau: the quadratic where x_0 <= 0.6, NaN beyond
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  std::vector<double> trace;  // [st.evals][2 D + 3]
};

bool same_bits(const double* p, const double* q, int n) { return std::memcmp(p, q, (size_t)n * sizeof(double)) == 0; }

// ns starts of one objective in one set of [ns][D] arrays, as the library-side loop and path_refine_kernel hold them: per
// round an evaluation at the trial point of every start that goes on, then refine_step_start for every start -- a frozen one
// included, which it must leave untouched.
template <bool AY_LATE>
std::vector<Run> run_many(const Objective& f, const double (*starts)[D], int ns, const double* scale, const RefineOpts& o,
                          const std::string& what) {
  constexpr int REC = 2 * D + 3;
  std::vector<double> X(ns * D, 0.0), G(ns * D, 0.0), Y(ns * D), GY(ns * D, 0.0), AY(ns, 0.0), A(ns, 0.0), AL(ns, 0.0);
  std::vector<double> trace((size_t)ns * o.max_evals * REC, -7.0);
  std::vector<int> evals(ns, 0), accepted(ns, 0), status(ns, REFINE_ACTIVE), nacc(ns, 0);
  std::vector<double> last(ns, 0.0);
  for (int i = 0; i < ns; ++i)
    for (int k = 0; k < D; ++k) Y[i * D + k] = refine_clip(starts[i][k], LO[k], HI[k]);
  RefineStepArgs a{};
  a.ns = ns; a.D = D; a.lower = LO; a.upper = HI; a.scale = scale; a.o = o;
  a.x = X.data(); a.g = G.data(); a.y = Y.data(); a.gy = GY.data(); a.ay = AY.data(); a.a = A.data(); a.alpha = AL.data();
  a.evals = evals.data(); a.accepted = accepted.data(); a.status = status.data(); a.trace = trace.data();
  bool first = true;
  for (int more = ns; more > 0; first = false) {
    more = 0;
    for (int i = 0; i < ns; ++i) {
      double* const y = &Y[i * D];
      const double* const gy = &GY[i * D];
      if (status[i] != REFINE_ACTIVE) {  // frozen
        const std::vector<double> fx = X, fg = G, fy = Y, fa = A, fal = AL, ftr = trace;
        const std::vector<int> fe = evals, fc = accepted, fs = status;
        CHECK(!refine_step_start<AY_LATE>(a, i, false));
        CHECK(fx == X && fg == G && fy == Y && fa == A && fal == AL && fe == evals && fc == accepted && fs == status);
        CHECK(same_bits(ftr.data(), trace.data(), (int)trace.size()));
        continue;
      }
      const int at_eval = first ? 0 : evals[i];
      CHECK(at_eval < o.max_evals);
      for (int k = 0; k < D; ++k) CHECK(y[k] >= LO[k] && y[k] <= HI[k]);
      AY[i] = eval(f, y, &GY[i * D]);
      const std::vector<double> at(y, y + D);
      const double alpha = first ? 0.0 : AL[i];
      const bool on = refine_step_start<AY_LATE>(a, i, first);
      CHECK(on == (status[i] == REFINE_ACTIVE) && evals[i] == at_eval + 1);
      more += on ? 1 : 0;
      // the record of this evaluation: (y, g_y, a_y, alpha, accepted)
      const double* const tr = &trace[((size_t)i * o.max_evals + at_eval) * REC];
      CHECK(same_bits(tr, at.data(), D) && same_bits(tr + D, gy, D) && same_bits(tr + 2 * D, &AY[i], 1));
      CHECK(tr[2 * D + 1] == alpha && (tr[2 * D + 2] == 1.0 || tr[2 * D + 2] == 0.0) && (!first || tr[2 * D + 2] == 1.0));
      if (first) {
        last[i] = A[i];
      } else if (tr[2 * D + 2] == 1.0) {
        ++nacc[i];
        CHECK(A[i] >= last[i]);  // monotone over accepted steps (c1 >= 0)
        CHECK(A[i] == AY[i] && same_bits(&X[i * D], at.data(), D) && same_bits(&G[i * D], gy, D));
        last[i] = A[i];
      }
    }
  }
  std::vector<Run> runs(ns);
  for (int i = 0; i < ns; ++i) {
    Run& r = runs[i];
    r.x.assign(&X[i * D], &X[i * D] + D);
    r.g.assign(&G[i * D], &G[i * D] + D);
    r.st.a = A[i]; r.st.alpha = AL[i]; r.st.evals = evals[i]; r.st.accepted = accepted[i]; r.st.status = status[i];
    CHECK(r.st.status != REFINE_ACTIVE && r.st.accepted == nacc[i] && r.st.evals >= 1 && r.st.evals <= o.max_evals);
    const double* const tr = &trace[(size_t)i * o.max_evals * REC];
    r.trace.assign(tr, tr + (size_t)r.st.evals * REC);
    for (size_t j = (size_t)r.st.evals * REC; j < (size_t)o.max_evals * REC; ++j) CHECK(tr[j] == -7.0);  // no record beyond
  }
  return runs;
}

// one start: the trace array and the state arrays that refine_step_start wrote, printed
Run run(const Objective& f, const double* start, const double* scale, const RefineOpts& o, const std::string& what) {
  constexpr int REC = 2 * D + 3;
  const double one[1][D] = {{start[0], start[1]}};
  const Run r = run_many<true>(f, one, 1, scale, o, what)[0];
  {  // the other place of the a_y load (path_refine_kernel's): the same bits
    const Run e = run_many<false>(f, one, 1, scale, o, what)[0];
    CHECK(e.st.status == r.st.status && e.st.evals == r.st.evals && e.st.accepted == r.st.accepted && e.x == r.x);
    CHECK(e.trace.size() == r.trace.size() && same_bits(e.trace.data(), r.trace.data(), (int)r.trace.size()));
  }
  std::printf("case %s\n", what.c_str());
  for (int e = 0; e < r.st.evals; ++e) {
    const double* const tr = &r.trace[(size_t)e * REC];
    std::printf("rec");
    for (int k = 0; k < 2 * D + 2; ++k) std::printf(" %a", tr[k]);
    std::printf(" %d\n", tr[2 * D + 2] == 1.0 ? 1 : 0);
  }
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
  for (int sc = 0; sc < 2; ++sc) {  // the four starts in one set of arrays: they end at different evaluations
    const std::string what = std::string("corner.together") + (sc ? ".scaled" : "");
    const std::vector<Run> all = run_many<false>(corner, starts, 4, sc ? scale : nullptr, o, what);
    bool differ = false;
    for (int si = 0; si < 4; ++si) {
      const double one[1][D] = {{starts[si][0], starts[si][1]}};
      const Run r = run_many<true>(corner, one, 1, sc ? scale : nullptr, o, what)[0];
      const Run& t = all[si];
      CHECK(t.st.status == r.st.status && t.st.evals == r.st.evals && t.st.accepted == r.st.accepted);
      CHECK(t.st.a == r.st.a && t.st.alpha == r.st.alpha && t.x == r.x && t.g == r.g);
      CHECK(t.trace.size() == r.trace.size() && same_bits(t.trace.data(), r.trace.data(), (int)r.trace.size()));
      differ = differ || t.st.evals != all[0].st.evals;
    }
    CHECK(differ);
  }
  std::printf("refine_step_check: ok\n");
  return 0;
}
