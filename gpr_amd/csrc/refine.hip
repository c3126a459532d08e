// gprhip_acquire_refine on the device: projected gradient ascent with Armijo backtracking from ns starts inside a box, by the
// rule of refine_step.h.
//   * small_refine_kernel (m <= 64, d <= 16, no projection -- the shapes of small_acquire_grad_kernel): one persistent kernel,
//     64 starts per workgroup, 16 per wavefront.  It compiles small_predict_grad_body.inc once more as the evaluator (REFINE):
//     U^-1, R~^-1, Z - s and t are staged in LDS once, the trial points live in the body's xs, the state of a start in the
//     registers of the 16 lanes that hold its gradient, and the evaluation loop runs inside the kernel until
//     __syncthreads_or says that no start of the workgroup goes on.  A row of the 64 x 64 products depends on its own trial
//     point only, and the sums and maxima of the rule are butterflies over a start's 16 lanes: a start's result does not
//     depend on what shares its wavefront or workgroup.  No atomics.
//   * refine_step_kernel (every other shape): the step between two evaluations of the library-side loop, one start per
//     thread on [ns][D] arrays: refine_step_start of refine_step.h, which path_refine_kernel (path_refine.hip) and the host
//     check call too.  One workgroup counts the starts that go on through LDS and writes the count where the host reads it.
#include <type_traits>

#include "small_pg.h"

namespace gprhip {

namespace {

template <int DT>
__global__ __launch_bounds__(256) void small_refine_kernel(SmallPredictGradArgs a, AcqArgs q, SmallRefineArgs rf) {
  constexpr bool ACQ = true, MV = false, REFINE = true;
  const MvArgs mv{};
#include "small_predict_grad_body.inc"
}
// the same loop around the epilogue of gprhip_acquire_max_value (mv_math.h): gprhip_acquire_max_value_refine
template <int DT>
__global__ __launch_bounds__(256) void small_max_value_refine_kernel(SmallPredictGradArgs a, MvArgs mv, SmallRefineArgs rf) {
  constexpr bool ACQ = false, MV = true, REFINE = true;
  const AcqArgs q{};
#include "small_predict_grad_body.inc"
}

void small_refine_attrs() {
  static uint64_t done = 0;
  once_per_device(done, [] {
    auto set = [](const void* f, size_t bytes) {
      GPR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    };
    set(reinterpret_cast<const void*>(&small_refine_kernel<4>), small_pg_lds(4));
    set(reinterpret_cast<const void*>(&small_refine_kernel<8>), small_pg_lds(8));
    set(reinterpret_cast<const void*>(&small_refine_kernel<16>), small_pg_lds(16));
    set(reinterpret_cast<const void*>(&small_max_value_refine_kernel<4>), small_pg_lds(4));
    set(reinterpret_cast<const void*>(&small_max_value_refine_kernel<8>), small_pg_lds(8));
    set(reinterpret_cast<const void*>(&small_max_value_refine_kernel<16>), small_pg_lds(16));
  });
}

__global__ __launch_bounds__(256) void refine_step_kernel(RefineStepArgs a) {
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  int mine = 0;
  for (int i = tid; i < a.ns; i += 256) mine += refine_step_start<true>(a, i, a.first != 0) ? 1 : 0;
  cnt[tid] = mine;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) cnt[tid] += cnt[tid + off];
    __syncthreads();
  }
  if (tid == 0) *a.active = cnt[0];
}

}  // namespace

void launch_small_refine(const SmallPredictGradArgs& a, const AcqArgs& q, const SmallRefineArgs& rf, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.m > SM || a.d > 16) {
    set_error("gprhip: the one-kernel refinement takes at most 64 inducing points of at most 16 dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  small_refine_attrs();
  auto go = [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL((small_refine_kernel<DT>), dim3((a.rows + SRB - 1) / SRB), dim3(256), small_pg_lds(DT), s, a, q, rf);
  };
  if (a.d <= 4) go(std::integral_constant<int, 4>{});
  else if (a.d <= 8) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 16>{});
  GPR_HIP(hipGetLastError());
}

void launch_small_max_value_refine(const SmallPredictGradArgs& a, const MvArgs& mv, const SmallRefineArgs& rf, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.m > SM || a.d > 16) {
    set_error("gprhip: the one-kernel refinement takes at most 64 inducing points of at most 16 dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  if (mv.n < 1 || mv.n > MV_MAX_EXTREMES || !mv.extremes || !a.want_var) {
    set_error("gprhip: the max-value epilogue takes 1 .. 64 extremes and the variance part");
    throw HipFail{ST_BAD_ARG};
  }
  small_refine_attrs();
  auto go = [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL((small_max_value_refine_kernel<DT>), dim3((a.rows + SRB - 1) / SRB), dim3(256), small_pg_lds(DT), s, a, mv,
                       rf);
  };
  if (a.d <= 4) go(std::integral_constant<int, 4>{});
  else if (a.d <= 8) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 16>{});
  GPR_HIP(hipGetLastError());
}

void launch_refine_step(const RefineStepArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(refine_step_kernel, dim3(1), dim3(256), 0, s, a);
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
