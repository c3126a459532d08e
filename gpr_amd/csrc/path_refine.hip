// gprhip_sample_paths_refine on the device: the ascent of refine_step.h on drawn sample paths.  Start i climbs
//   o(x) = s f_j(x),  f_j(x) = sum_c k(x, z_c) A[c][j],  j = draw_of[i],
// with the weights A of launch_sp_weights (sample_paths.hip), s = +1 / -1.
//   * path_eval: ONE device function, the evaluator of both routes.  The wavefront layout of predict_grad_kernel and
//     sample_paths_kernel -- 16 points per wavefront, the columns walked in order, panels of Z - s and of A staged in LDS, the
//     distance product as a first MFMA chain whose A rows are permuted so that a lane ends with four adjacent columns, one
//     exp per (row, column), K never in memory.  The weight is per ROW: E_rc = K_rc A[c][draw_of[r]], a gather from the staged
//     panel; the value is the row sum of E and E is the A operand of the second MFMA chain E (Z - s) -- the E_mean arithmetic
//     of predict_grad_body.inc with t replaced by a gathered column.  A row of either chain depends on its own point and its
//     own draw only: a start's bits do not depend on what shares its wavefront or workgroup, nor on the width of the panel.
//   * path_refine_kernel (no projection, any m, d <= 64): one persistent kernel, 64 starts per workgroup.  The state of a
//     start is the [ns][D] arrays of the library-side loop (RefineStepArgs), in device memory and touched by one workgroup
//     only; after an evaluation one lane per start runs refine_step_start of refine_step.h on it -- neither the rule nor its
//     driver is written again: refine_step_kernel calls the same function -- and the loop goes on until __syncthreads_or
//     says that no start of the workgroup does.
//     The panels are staged again for every evaluation (from L2 once m exceeds a panel).  A finished start is frozen: its
//     rows are not evaluated, nothing of it is written again, its lanes only take part in the barriers.
//   * path_eval_kernel (with a projection): one evaluation of the library-side loop, the same device function over the ns
//     projected trial points; launch_input_grad_project and refine_step_kernel (refine.hip) follow it.
// No atomics: two runs give the same bits.
#include <type_traits>

#include "kernels.h"
#include "exp_fast.h"

namespace gprhip {

namespace {

typedef double pd4 __attribute__((ext_vector_type(4)));
// lane supplies A[lane&15][lane>>4] and B[lane>>4][lane&15]; accumulator element r is D[(lane>>4) + 4r][lane&15]
__device__ __forceinline__ pd4 pmfma4(double a, double b, pd4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

constexpr int PR_ROWS = 64;               // starts per workgroup
constexpr int PR_LDA = SP_MAX_DRAWS + 4;  // leading dimension of the staged panel of A
// inducing columns per staged panel: 64 up to 16 point dimensions, else 32 (the two panels take 45 KB at most)
template <int DT>
struct PathLds {
  static constexpr int DP = DT * 16, LDP = DP + 4, CP = DT == 1 ? 64 : 32;
  double zs[CP * LDP];     // Z - s
  double ap[CP * PR_LDA];  // A, columns < nd
  double zn[CP];           // |z_c - s|^2
  double sh[DP];           // s
};

// o and do/dp at the 16 points row0 .. row0 + 15 of e.pts, by one wavefront of a workgroup of 256 threads; the whole workgroup
// must call it (the panels are staged between barriers).  L.sh must hold the shift.  use_status: rows whose status is not
// REFINE_ACTIVE are not evaluated and nothing is stored for them.
template <int KS4, int DT>
__device__ __forceinline__ void path_eval(const PathEvalArgs& e, PathLds<DT>& L, int row0, bool use_status) {
  constexpr int DP = PathLds<DT>::DP, LDP = PathLds<DT>::LDP, CP = PathLds<DT>::CP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int prow = row0 + l15;  // the point of this lane's elements of E
  bool live_r = prow < e.rows;
  if (live_r && use_status) live_r = e.status[prow] == REFINE_ACTIVE;
  const bool wave_live = __ballot(live_r) != 0;
  const int dr = live_r ? e.draw_of[prow] : 0;
  const int mc = (e.m + 15) & ~15;  // columns walked
  const ExpK ek = exp_consts();

  double pb[KS4], pn = 0.0;
#pragma unroll
  for (int s = 0; s < KS4; ++s) {
    const int k = 4 * s + lq;
    const double v = (live_r && k < e.d) ? e.pts[(int64_t)prow * e.d + k] - L.sh[k] : 0.0;
    pb[s] = v;
    pn += v * v;
  }
  pn += __shfl_xor(pn, 16);
  pn += __shfl_xor(pn, 32);
  pd4 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) acc[t] = (pd4){0, 0, 0, 0};
  double rs = 0.0;
  const int pcol = 4 * (l15 & 3) + (l15 >> 2);  // A rows of the distance product: 0 4 8 12 1 5 ...

  for (int c0 = 0; c0 < mc; c0 += CP) {
    __syncthreads();
    for (int idx = tid; idx < CP * DP; idx += 256) {
      const int c = idx / DP, k = idx % DP, col = c0 + c;
      L.zs[c * LDP + k] = (col < e.m && k < e.d) ? e.Z[(int64_t)col * e.d + k] - L.sh[k] : 0.0;
    }
    for (int idx = tid; idx < CP * e.nd; idx += 256) {
      const int c = idx / e.nd, j = idx % e.nd, col = c0 + c;
      L.ap[c * PR_LDA + j] = col < e.m ? e.W[(int64_t)col * SP_MAX_DRAWS + j] : 0.0;
    }
    __syncthreads();
    {
      const int c = tid >> 2, q = tid & 3;  // (c < CP: whole wavefronts)
      if (c < CP) {
        double s2 = 0.0;
        for (int k = q; k < DP; k += 4) s2 += L.zs[c * LDP + k] * L.zs[c * LDP + k];
        s2 += __shfl_xor(s2, 1);
        s2 += __shfl_xor(s2, 2);
        if (q == 0) L.zn[c] = s2;
      }
      __syncthreads();
    }
    if (!wave_live) continue;
#pragma unroll 1
    for (int j = 0; j < CP / 16; ++j) {
      const int cb = c0 + 16 * j;
      if (cb >= mc) break;
      pd4 s4 = (pd4){0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < KS4; ++s) s4 = pmfma4(L.zs[(16 * j + pcol) * LDP + 4 * s + lq], pb[s], s4);
      double em[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * j + 4 * lq + r;
        const double dist = fmax(pn + L.zn[c] - 2.0 * s4[r], 0.0);
        em[r] = (live_r && c0 + c < e.m) ? exp_fast(e.log_sf2 + e.inv_ell2_05 * dist, ek) * L.ap[c * PR_LDA + dr] : 0.0;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        rs += em[r];
#pragma unroll
        for (int t = 0; t < DT; ++t) acc[t] = pmfma4(em[r], L.zs[(16 * j + 4 * lq + r) * LDP + 16 * t + l15], acc[t]);
      }
    }
  }
  rs += __shfl_xor(rs, 16);
  rs += __shfl_xor(rs, 32);  // every lane: rowsum(E) of point l15 = f at it
  if (lq == 0 && live_r) e.val[prow] = e.sign * rs;
  const double inv_ell2 = -2.0 * e.inv_ell2_05;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = row0 + lq + 4 * r;
    const double rm = __shfl(rs, lq + 4 * r);
    const bool live_o = __shfl(live_r ? 1 : 0, lq + 4 * r) != 0;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int dim = 16 * t + l15;
      if (live_o && dim < e.d) {
        const double pc = e.pts[(int64_t)orow * e.d + dim] - L.sh[dim];
        e.grad[(int64_t)orow * e.ldg + dim] = e.sign * (-inv_ell2 * (pc * rm - acc[t][r]));
      }
    }
  }
}

template <int KS4, int DT>
__global__ __launch_bounds__(256) void path_eval_kernel(PathEvalArgs e, int use_status) {
  __shared__ PathLds<DT> L;
  const int tid = threadIdx.x;
  if (tid < PathLds<DT>::DP) L.sh[tid] = tid < e.d ? e.shift[tid] : 0.0;
  __syncthreads();
  path_eval<KS4, DT>(e, L, blockIdx.x * PR_ROWS + (tid >> 6) * 16, use_status != 0);
}

// e.pts / e.val / e.grad / e.status are st.y / st.ay / st.gy / st.status (e.ldg = e.d = st.D): an evaluation, a barrier (the
// workgroup's own stores are visible to it then), the step of the workgroup's 64 starts by its first wavefront, and the
// vote.  The trip count is the same for the whole workgroup.
template <int KS4, int DT>
__global__ __launch_bounds__(256) void path_refine_kernel(PathEvalArgs e, RefineStepArgs st) {
  __shared__ PathLds<DT> L;
  const int tid = threadIdx.x;
  // (said once more for the compiler: one set of scalar registers holds what the two structs share)
  e.pts = st.y; e.val = const_cast<double*>(st.ay); e.grad = const_cast<double*>(st.gy); e.status = st.status; e.rows = st.ns; e.d = st.D; e.ldg = st.D;
  if (tid < PathLds<DT>::DP) L.sh[tid] = tid < e.d ? e.shift[tid] : 0.0;
  __syncthreads();
  const int r0 = blockIdx.x * PR_ROWS;
  bool first = true;
  for (;;) {
    path_eval<KS4, DT>(e, L, r0 + (tid >> 6) * 16, !first);
    __syncthreads();
    int more = 0;
    if (tid < PR_ROWS && r0 + tid < st.ns) more = refine_step_start<false>(st, r0 + tid, first) ? 1 : 0;
    first = false;
    if (!__syncthreads_or(more)) break;
  }
}

template <typename F>
void by_width(int d, F&& go) {
  if (d <= 4) go(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
  else if (d <= 8) go(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{});
  else if (d <= 16) go(std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{});
  else if (d <= 32) go(std::integral_constant<int, 8>{}, std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, 16>{}, std::integral_constant<int, 4>{});
}

void check_path_eval(const PathEvalArgs& e) {
  if (e.d > 64 || e.nd < 1 || e.nd > SP_MAX_DRAWS || !e.val || !e.grad || !e.draw_of) {
    set_error("gprhip: the refinement of sample paths takes 1 .. 64 draws of at most 64 point dimensions");
    throw HipFail{ST_BAD_ARG};
  }
}

}  // namespace

void launch_path_eval(const PathEvalArgs& e, hipStream_t s) {
  if (e.rows <= 0) return;
  check_path_eval(e);
  const dim3 grid((e.rows + PR_ROWS - 1) / PR_ROWS);
  const int use_status = e.status ? 1 : 0;
  by_width(e.d, [&](auto ks4, auto dt) {
    hipLaunchKernelGGL((path_eval_kernel<decltype(ks4)::value, decltype(dt)::value>), grid, dim3(256), 0, s, e, use_status);
  });
  GPR_HIP(hipGetLastError());
}

void launch_path_refine(const PathEvalArgs& e, const RefineStepArgs& st, hipStream_t s) {
  if (e.rows <= 0) return;
  check_path_eval(e);
  if (e.rows != st.ns || e.d != st.D || e.ldg != st.D || e.pts != st.y || e.val != st.ay || e.grad != st.gy ||
      e.status != st.status) {
    set_error("gprhip: the one-kernel refinement of sample paths evaluates the loop's own arrays (no projection)");
    throw HipFail{ST_BAD_ARG};
  }
  const dim3 grid((e.rows + PR_ROWS - 1) / PR_ROWS);
  by_width(e.d, [&](auto ks4, auto dt) {
    hipLaunchKernelGGL((path_refine_kernel<decltype(ks4)::value, decltype(dt)::value>), grid, dim3(256), 0, s, e, st);
  });
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
