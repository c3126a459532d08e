// The step rule of gprhip_acquire_refine: projected gradient ascent with Armijo backtracking on one start inside a box
// (include/gprhip.h has the contract).  One copy for the host and the device: the persistent kernel of refine.hip (a start's
// components spread over 16 lanes) calls the arithmetic; refine_step_kernel (one start per thread), path_refine_kernel (one
// lane per start) and tests/cpp/refine_step_check.cpp on analytic objectives call refine_step_start, the step of one start on
// [ns][D] arrays.  The objective is any "larger is better" function with a gradient: nothing here knows of the acquisition
// criteria (gprhip_sample_paths_refine climbs drawn sample paths with it).
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
// the second group are the rule for a start whose components one thread holds; RefineStepArgs and refine_step_start are that
// rule driven on the arrays that hold the starts of a call between two evaluations.
#pragma once
#include <math.h>
#include <stdint.h>

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

// ---- the starts of a call as [ns][D] arrays (device memory on the device): the state between two evaluations
// first: (ay, gy) is the evaluation at the clipped starts in y (x, g and the per-start state are initialised from it), else at
// the trial points y.  y receives the next trial points.  The trace is [ns][max_evals][2 D + 3] records (y, g_y, a_y, alpha,
// accepted), one per evaluation.  `first` and `active` belong to refine_step_kernel: *active (pinned host memory,
// device-visible) receives the number of starts that go on.
struct RefineStepArgs {
  int ns, D, first;
  const double *lower, *upper, *scale;  // [D]; scale may be null
  RefineOpts o;
  double *x, *g, *y;                    // [ns][D]
  const double *gy, *ay;                // [ns][D], [ns]
  double *a, *alpha;                    // [ns]
  int *evals, *accepted, *status;       // [ns]
  double* trace;                        // or null
  int* active;
};

// One step of the rule for start i after an evaluation: its state is loaded from the arrays, refine_begin or refine_advance
// runs on it, the trace record of the evaluation is written and the state is stored back.  Returns whether the start goes on;
// y then holds its next trial point.  A frozen start (status not REFINE_ACTIVE after the first evaluation) is left untouched.
// AY_LATE: where the load of a_y stands -- straight after the status read, or inside each branch behind the other loads.  The
// results are the same; the compiler's register allocation is not (profiles/refine_regs.txt, profiles/path_refine_regs.txt):
// refine_step_kernel takes true, path_refine_kernel false.
template <bool AY_LATE>
GPRHIP_REFINE_FN bool refine_step_start(const RefineStepArgs& a, int i, bool first) {
  const int D = a.D;
  const int64_t rec = 2 * D + 3;
  double *const x = a.x + (int64_t)i * D, *const g = a.g + (int64_t)i * D, *const y = a.y + (int64_t)i * D;
  const double* const gy = a.gy + (int64_t)i * D;
  RefineStart st;
  bool acc = true;
  double alpha = 0.0;
  int at = 0;
  if (!first) {  // the status alone first: a frozen start costs one load
    st.status = a.status[i];
    if (st.status != REFINE_ACTIVE) return false;
  }
  double ay;  // (no initialiser: path_refine_kernel keeps the instructions it had)
  if (!AY_LATE) ay = a.ay[i];
  if (first) {
    if (AY_LATE) ay = a.ay[i];
    for (int k = 0; k < D; ++k) {  // y holds the clipped start
      x[k] = y[k];
      g[k] = gy[k];
    }
    refine_begin(D, x, g, ay, a.lower, a.upper, a.scale, a.o, st, y);
  } else {
    st.a = a.a[i]; st.alpha = a.alpha[i]; st.evals = a.evals[i]; st.accepted = a.accepted[i];
    if (AY_LATE) ay = a.ay[i];
    alpha = st.alpha;
    at = st.evals;
    if (a.trace) {
      double* const tr = a.trace + ((int64_t)i * a.o.max_evals + at) * rec;
      for (int k = 0; k < D; ++k) tr[k] = y[k];
    }
    acc = refine_advance(D, x, g, y, gy, ay, a.lower, a.upper, a.scale, a.o, st);
  }
  if (a.trace) {
    double* const tr = a.trace + ((int64_t)i * a.o.max_evals + at) * rec;
    for (int k = 0; k < D; ++k) {
      if (first) tr[k] = x[k];
      tr[D + k] = gy[k];
    }
    tr[2 * D] = ay;
    tr[2 * D + 1] = alpha;
    tr[2 * D + 2] = acc ? 1.0 : 0.0;
  }
  a.a[i] = st.a; a.alpha[i] = st.alpha; a.evals[i] = st.evals; a.accepted[i] = st.accepted; a.status[i] = st.status;
  return st.status == REFINE_ACTIVE;
}

}  // namespace gprhip
