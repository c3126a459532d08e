// What the kernels that compile small_predict_grad_body.inc share (predict_grad.hip: small_predict_grad_kernel and
// small_acquire_grad_kernel, small_max_value_grad_kernel; refine.hip: small_refine_kernel): the LDS shapes, the 64 x 64 products on
// v_mfma_f64_16x16x4_f64, and the refinement step of gprhip_acquire_refine on the body's lane layout.
#pragma once
#include "kernels.h"
#include "exp_fast.h"
#include "acq_math.h"
#include "mv_math.h"
#include "refine_step.h"

namespace gprhip {

namespace {

typedef double pd4 __attribute__((ext_vector_type(4)));
typedef double pd2 __attribute__((ext_vector_type(2)));
// lane supplies A[lane&15][lane>>4] and B[lane>>4][lane&15]; accumulator element r is D[(lane>>4) + 4r][lane&15]
__device__ __forceinline__ pd4 pmfma4(double a, double b, pd4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ---- at most 64 inducing points of at most 16 dimensions: a block of 64 test points in one kernel
constexpr int SM = 64;    // inducing points (padded)
constexpr int SLD = 66;   // leading dimension of the 64 x 64 LDS matrices
constexpr int SRB = 64;   // test points per workgroup
constexpr int LDZ = 20;   // leading dimension of the staged Z - s (16 dimensions)

// rows [16 wv, 16 wv + 16) of  A (LDS, [64][SLD]) times  B (LDS, [64][SLD]; TRANS: times B^T)  -> acc[ct], ct = column tile
// (the fully unrolled form of small.hip's rows_times: all fragments of a half of the k-range loaded before its 32 MFMAs)
template <bool TRANS>
__device__ __forceinline__ void rows_times(const double* A, const double* B, int wv, int l15, int lq, pd4 (&acc)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = pd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double af[8], bf[8][4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kk = 8 * h + j;
      af[j] = A[(16 * wv + l15) * SLD + 4 * kk + lq];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        bf[j][ct] = TRANS ? B[(16 * ct + l15) * SLD + 4 * kk + lq] : B[(4 * kk + lq) * SLD + 16 * ct + l15];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = pmfma4(af[j], bf[j][ct], acc[ct]);
  }
}

// 64 x 64 corner of a row-major mp x mp matrix -> LDS
__device__ __forceinline__ void load_corner(const double* __restrict__ M, int mp, double* L, int tid) {
  double2 v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = tid + 256 * j, r = idx >> 5, c2 = (idx & 31) * 2;
    v[j] = *reinterpret_cast<const double2*>(M + (int64_t)r * mp + c2);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = tid + 256 * j, r = idx >> 5, c2 = (idx & 31) * 2;
    *reinterpret_cast<double2*>(L + r * SLD + c2) = v[j];
  }
}

// rows of this wavefront: accumulator tiles -> LDS (in place of an operand the wavefront alone reads)
__device__ __forceinline__ void store_rows(double* W, const pd4 (&acc)[4], int wv, int l15, int lq) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) W[(16 * wv + lq + 4 * r) * SLD + 16 * ct + l15] = acc[ct][r];
}

inline size_t small_pg_lds(int DT) { return (size_t)(4 * SM * SLD + SM * LDZ + SRB * DT + SM + 16) * sizeof(double); }

// ---- the refinement loop around the body (REFINE; refine_step.h is the rule).  The body leaves the gradient spread over
// lanes -- lane (lq, l15) holds component l15 of the rows lq + 4 r of its wavefront, r = 0 .. 3 -- so a lane carries one
// component of four starts, and what the rule sums or maximises over the components of a start is a butterfly over the 16
// lanes of equal lq: every one of them ends with the same bits, whatever the other rows of the wavefront hold.
struct RefineRows {
  double x[4], g[4], y[4], a[4], alpha[4];  // the start's state (x, g, y: this lane's component); y: the trial point
  double gy[4], ay[4];                      // the evaluation at y as the body leaves it
  int evals[4], accepted[4], status[4];
  double lo, hi, w, sc;                     // this lane's component of the box (lanes >= d: lo = hi = 0, w = inf)
};

__device__ __forceinline__ double rf_sum16(double v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double rf_max16(double v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v = refine_max(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ double rf_min16(double v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v = refine_min(v, __shfl_xor(v, off));
  return v;
}

// rf_step is the lane-spread twin of refine_begin / refine_advance / refine_propose (refine_step.h), which the host check and
// refine_step_kernel run: it must mirror them line for line -- the NaN test, the zero-direction test after an acceptance, grow /
// shrink, then MAX_EVALS before the xtol test -- and calls the same per-component functions.  Only the GPU trace tests hold
// this copy; an edit of the one belongs in the other.
// One step of the rule for the four starts of a lane after an evaluation (first: the one at the clipped start): the trial
// points of the starts that go on are written to xs.  Returns whether one of them does.  A finished start is frozen: nothing
// of it is written again.  Every shuffle is executed by all lanes.
template <int DT>
__device__ __forceinline__ bool rf_step(const SmallPredictGradArgs& a, const SmallRefineArgs& rf, RefineRows& rr, double* xs,
                                        int r0, int wv, int lq, int l15, bool first) {
  bool any = false;
  const bool comp = l15 < a.d;
  const int64_t rec = 2 * a.d + 3;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lrow = 16 * wv + lq + 4 * r;
    const int64_t orow = (int64_t)r0 + lrow;
    const bool live = orow < a.rows;
    const double ay = rr.ay[r], gy = comp ? rr.gy[r] : 0.0;
    double* const tr = (rf.trace && live) ? rf.trace + (orow * rf.o.max_evals + (first ? 0 : rr.evals[r])) * rec : nullptr;
    if (first) {
      rr.x[r] = comp ? xs[lrow * DT + l15] : 0.0;
      rr.y[r] = rr.x[r];
      rr.g[r] = gy;
      rr.a[r] = ay;
      rr.alpha[r] = 0.0;
      rr.evals[r] = 1;
      rr.accepted[r] = 0;
      rr.status[r] = live ? (ay != ay ? REFINE_NAN : REFINE_ACTIVE) : REFINE_CONVERGED;
      if (tr) {
        if (comp) {
          tr[l15] = rr.x[r];
          tr[a.d + l15] = gy;
        }
        if (l15 == 0) {
          tr[2 * a.d] = ay;
          tr[2 * a.d + 1] = 0.0;
          tr[2 * a.d + 2] = 1.0;
        }
      }
      const double dmax = rf_max16(fabs(refine_dir(gy, rr.sc, rr.x[r], rr.lo, rr.hi)));
      const double wmin = rf_min16(rr.w);
      if (rr.status[r] == REFINE_ACTIVE) {
        if (dmax == 0.0) rr.status[r] = REFINE_CONVERGED;
        else rr.alpha[r] = refine_alpha0(rf.o.step0, wmin, dmax);
      }
    } else {
      const bool act = rr.status[r] == REFINE_ACTIVE;
      const double gd = rf_sum16(rr.g[r] * (rr.y[r] - rr.x[r]));
      const bool acc = refine_armijo(rr.a[r], ay, rf.o.c1, gd);
      if (act) {
        if (tr) {
          if (comp) {
            tr[l15] = rr.y[r];
            tr[a.d + l15] = gy;
          }
          if (l15 == 0) {
            tr[2 * a.d] = ay;
            tr[2 * a.d + 1] = rr.alpha[r];
            tr[2 * a.d + 2] = acc ? 1.0 : 0.0;
          }
        }
        ++rr.evals[r];
        if (acc) {
          rr.x[r] = rr.y[r];
          rr.g[r] = gy;
          rr.a[r] = ay;
          ++rr.accepted[r];
        }
      }
      const double dmax = rf_max16(fabs(refine_dir(rr.g[r], rr.sc, rr.x[r], rr.lo, rr.hi)));
      if (act) {
        if (acc && dmax == 0.0) rr.status[r] = REFINE_CONVERGED;
        else rr.alpha[r] *= acc ? rf.o.grow : rf.o.shrink;
      }
    }
    // step 3's head: the next trial point, or the end of the start
    const double dk = refine_dir(rr.g[r], rr.sc, rr.x[r], rr.lo, rr.hi);
    const double yn = refine_trial(rr.x[r], rr.alpha[r], dk, rr.lo, rr.hi);
    const double rel = rf_max16(comp ? refine_rel(yn - rr.x[r], rr.w) : 0.0);
    if (rr.status[r] == REFINE_ACTIVE) {
      if (rr.evals[r] >= rf.o.max_evals) {
        rr.status[r] = REFINE_MAX_EVALS;
      } else if (rel <= rf.o.xtol) {
        rr.status[r] = REFINE_CONVERGED;
      } else {
        rr.y[r] = yn;
        if (comp) xs[lrow * DT + l15] = yn;
        any = true;
      }
    }
  }
  return any;
}

// the results of the four starts of a lane (every output may be null)
__device__ __forceinline__ void rf_store(const SmallPredictGradArgs& a, const SmallRefineArgs& rf, const RefineRows& rr, int r0,
                                         int wv, int lq, int l15) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t orow = (int64_t)r0 + 16 * wv + lq + 4 * r;
    if (orow >= a.rows) continue;
    if (l15 < a.d) {
      if (rf.x_out) rf.x_out[orow * a.d + l15] = rr.x[r];
      if (rf.dvalues) rf.dvalues[orow * a.d + l15] = rr.g[r];
    }
    if (l15 == 0) {
      if (rf.values) rf.values[orow] = rr.a[r];
      if (rf.evals) rf.evals[orow] = rr.evals[r];
      if (rf.accepted) rf.accepted[orow] = rr.accepted[r];
      if (rf.status) rf.status[orow] = rr.status[r];
    }
  }
}

}  // namespace

}  // namespace gprhip
