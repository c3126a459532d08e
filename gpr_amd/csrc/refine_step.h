// The step rule of gprhip_acquire_refine: projected gradient ascent with Armijo backtracking on one start inside a box
// (include/gprhip.h has the contract).  One copy for the host and the device: the persistent kernel of refine.hip (a start's
// components spread over 16 lanes) and refine_step_kernel (one start per thread) call these functions, and so does
// tests/cpp/refine_step_check.cpp on analytic objectives.  The objective is any "larger is better" function with a gradient:
// nothing here knows of the acquisition criteria (a drawn sample path would do as well).
//
// Per start, with w_k = upper_k - lower_k:
//   1. x = clip(start); (a, g) the objective and its gradient at x; evals = 1.  a NaN: status NAN.
//   2. dir_k = scale_k g_k, set to 0 where the bound is active and dir_k points out of the box (and where g_k is NaN: such a
//      component does not move).  All dir_k = 0: CONVERGED.  alpha = (step0 min_k w_k) / max_k |dir_k|.
//   3. while evals < max_evals:  y = clip(x + alpha dir) (y_k = x_k where dir_k = 0), delta = y - x;
//      max_k |delta_k| / w_k <= xtol: CONVERGED;  else (a_y, g_y) at y, ++evals;  a_y >= a + c1 sum_k g_k delta_k (false for
//      NaN): accept -- x, a, g = y, a_y, g_y, ++accepted, dir again (all zero: CONVERGED), alpha *= grow;  else alpha *= shrink.
//   4. MAX_EVALS when the evaluations run out.
// The functions of the first group are the rule's arithmetic, component by component; RefineStart and the three functions of
// the second group are the rule for a start whose components one thread holds.
#pragma once
#include <math.h>

#ifndef GPRHIP_REFINE_FN
#define GPRHIP_REFINE_FN __host__ __device__ __forceinline__
#endif

namespace gprhip {

enum { REFINE_ACTIVE = -1, REFINE_CONVERGED = 0, REFINE_MAX_EVALS = 1, REFINE_NAN = 2 };  // GPRHIP_REFINE_*

struct RefineOpts {
  int max_evals;
  double step0, c1, shrink, grow, xtol;
};

// ---- the arithmetic, per component
GPRHIP_REFINE_FN double refine_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
GPRHIP_REFINE_FN double refine_dir(double g, double scale, double x, double lo, double hi) {
  const double dk = scale * g;
  if (dk != dk) return 0.0;
  if (x <= lo && dk < 0.0) return 0.0;
  if (x >= hi && dk > 0.0) return 0.0;
  return dk;
}
GPRHIP_REFINE_FN double refine_max(double m, double v) { return v > m ? v : m; }
GPRHIP_REFINE_FN double refine_min(double m, double v) { return v < m ? v : m; }
GPRHIP_REFINE_FN double refine_alpha0(double step0, double wmin, double dmax) { return (step0 * wmin) / dmax; }
// (no contraction into an FMA in the two sums of the rule: x + alpha dir cancels where a step crosses most of the box, and the
//  host, the device and the Python reference of the tests round it alike)
GPRHIP_REFINE_FN double refine_trial(double x, double alpha, double dir, double lo, double hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return dir == 0.0 ? x : refine_clip(x + alpha * dir, lo, hi);  // (alpha may be infinite under a tiny gradient)
}
GPRHIP_REFINE_FN double refine_rel(double delta, double w) { return fabs(delta) / w; }
GPRHIP_REFINE_FN bool refine_armijo(double a, double ay, double c1, double gd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ay >= a + c1 * gd;
}

// ---- a start whose D components one thread holds
struct RefineStart {
  double a, alpha;
  int evals, accepted, status;
};

// dir of (x, g) -> its largest magnitude; dir itself is not stored: refine_dir is evaluated again where it is needed
GPRHIP_REFINE_FN double refine_dir_max(int D, const double* x, const double* g, const double* lo, const double* hi,
                                       const double* scale) {
  double dmax = 0.0;
  for (int k = 0; k < D; ++k) dmax = refine_max(dmax, fabs(refine_dir(g[k], scale ? scale[k] : 1.0, x[k], lo[k], hi[k])));
  return dmax;
}

// step 3's head: the next trial point into y, or the end of the start (status).  st.status must be REFINE_ACTIVE.
GPRHIP_REFINE_FN void refine_propose(int D, const double* x, const double* g, const double* lo, const double* hi,
                                     const double* scale, const RefineOpts& o, RefineStart& st, double* y) {
  if (st.evals >= o.max_evals) {
    st.status = REFINE_MAX_EVALS;
    return;
  }
  double rel = 0.0;
  for (int k = 0; k < D; ++k) {
    const double dk = refine_dir(g[k], scale ? scale[k] : 1.0, x[k], lo[k], hi[k]);
    y[k] = refine_trial(x[k], st.alpha, dk, lo[k], hi[k]);
    rel = refine_max(rel, refine_rel(y[k] - x[k], hi[k] - lo[k]));
  }
  if (rel <= o.xtol) st.status = REFINE_CONVERGED;
}

// steps 1 and 2: x holds the clipped start, (a, g) the evaluation there
GPRHIP_REFINE_FN void refine_begin(int D, const double* x, const double* g, double a, const double* lo, const double* hi,
                                   const double* scale, const RefineOpts& o, RefineStart& st, double* y) {
  st.a = a;
  st.alpha = 0.0;
  st.evals = 1;
  st.accepted = 0;
  st.status = REFINE_ACTIVE;
  if (a != a) {
    st.status = REFINE_NAN;
    return;
  }
  const double dmax = refine_dir_max(D, x, g, lo, hi, scale);
  if (dmax == 0.0) {
    st.status = REFINE_CONVERGED;
    return;
  }
  double wmin = hi[0] - lo[0];
  for (int k = 1; k < D; ++k) wmin = refine_min(wmin, hi[k] - lo[k]);
  st.alpha = refine_alpha0(o.step0, wmin, dmax);
  refine_propose(D, x, g, lo, hi, scale, o, st, y);
}

// step 3's tail: (ay, gy) is the evaluation at the trial point y.  Returns whether y was accepted (x, g updated); y
// receives the next trial point unless the start ends.
GPRHIP_REFINE_FN bool refine_advance(int D, double* x, double* g, double* y, const double* gy, double ay, const double* lo,
                                     const double* hi, const double* scale, const RefineOpts& o, RefineStart& st) {
  ++st.evals;
  double gd = 0.0;
  for (int k = 0; k < D; ++k) gd += g[k] * (y[k] - x[k]);
  const bool acc = refine_armijo(st.a, ay, o.c1, gd);
  if (acc) {
    for (int k = 0; k < D; ++k) {
      x[k] = y[k];
      g[k] = gy[k];
    }
    st.a = ay;
    ++st.accepted;
    if (refine_dir_max(D, x, g, lo, hi, scale) == 0.0) {
      st.status = REFINE_CONVERGED;
      return true;
    }
    st.alpha *= o.grow;
  } else {
    st.alpha *= o.shrink;
  }
  refine_propose(D, x, g, lo, hi, scale, o, st, y);
  return acc;
}

}  // namespace gprhip
