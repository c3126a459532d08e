// Gradients of the predictive mean and variance with respect to the test inputs (Cov_se_iso, Cov_se_fat without multiscales).
//
// With p_r the point the kernel sees, K_rc = k(p_r, z_c), t the mean coefficients and
//   M = U^-1 (I - R~^-1 R~^-T) U^-T   (= (K_m + jitter)^-1 - B^-1),   G = K M:
//   mu_r      = sum_c K_rc t_c                     dmu_r / dp_rk      = -inv_ell2 sum_c K_rc t_c  (p_rk - z_ck)
//   sigma2_r  = sf2 - sum_c K_rc G_rc (+ sigma2)   dsigma2_r / dp_rk  = 2 inv_ell2 sum_c K_rc G_rc (p_rk - z_ck)
// Both gradients are the row sums of input_grad.hip with two weight sets over one K -- E_mean = K .* (1 t^T) and E_var = K .* G --
// evaluated as (p_rk - s_k) rowsum(E)_r - (E (Z - s))_rk with the common offset s (the centroid of the inducing points); the two
// row sums are the mean and the reduction of the variance themselves.
//   * predict_grad_kernel (any m, d <= 64): the wavefront layout of input_grad_kernel -- 16 test points per wavefront, the
//     columns walked in order, Z - s panels (and t) in LDS, the distance product as a first MFMA chain whose A rows are permuted
//     so that a lane ends with four adjacent columns, K and its exp shared by the two accumulator sets, G read 32 contiguous
//     bytes per lane.  VAR = false: the mean part alone, no G is read.  No atomics: two runs give the same bits.
//   * small_predict_grad_kernel (m <= 64, d <= 16): one kernel per chunk as small_predict_kernel -- the K tile in LDS,
//     V = K U^-1, Q = V R~^-1, H = V - Q R~^-T, G = H U^-T on the 64 x 64 corners, then both E products against Z - s.
#include <type_traits>

#include "small_pg.h"

namespace gprhip {

namespace {

constexpr int PG_CP = 64;    // inducing columns per staged panel
constexpr int PG_ROWS = 64;  // test points per workgroup

// KS4 = ceil(d / 4) k-steps of the distance product, DT = ceil(d / 16) tiles of point dimensions, VAR: the variance part
// The plain kernel and the one with the criterion epilogue of gprhip_acquire compile the same body text (predict_grad_body.inc,
// included as small.hip includes its bodies): up to the epilogue they are the same instructions.  ACQ: a.dmeans receives
// c_mu dmeans + c_v dvars, q.values the criterion; a.dvars is not used.  MV: the same with the coefficients of max-value entropy
// search (mv.values the criterion).
template <int KS4, int DT, bool VAR>
__global__ __launch_bounds__(256) void predict_grad_kernel(PredictGradArgs a) {
  constexpr bool ACQ = false, MV = false;
  const AcqArgs q{};
  const MvArgs mv{};
#include "predict_grad_body.inc"
}
template <int KS4, int DT, bool VAR>
__global__ __launch_bounds__(256) void acquire_grad_kernel(PredictGradArgs a, AcqArgs q) {
  constexpr bool ACQ = true, MV = false;
  const MvArgs mv{};
#include "predict_grad_body.inc"
}
// MV: the epilogue of gprhip_acquire_max_value (mv_math.h) in place of the criterion of gprhip_acquire; it needs the variance part
template <int KS4, int DT>
__global__ __launch_bounds__(256) void max_value_grad_kernel(PredictGradArgs a, MvArgs mv) {
  constexpr bool ACQ = false, MV = true, VAR = true;
  const AcqArgs q{};
#include "predict_grad_body.inc"
}

template <int KS4, int DT>
void launch_one(const PredictGradArgs& a, hipStream_t s) {
  const dim3 grid((a.rows + PG_ROWS - 1) / PG_ROWS);
  if (a.G) hipLaunchKernelGGL((predict_grad_kernel<KS4, DT, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((predict_grad_kernel<KS4, DT, false>), grid, dim3(256), 0, s, a);
}
template <int KS4, int DT>
void launch_one_acq(const PredictGradArgs& a, const AcqArgs& q, hipStream_t s) {
  const dim3 grid((a.rows + PG_ROWS - 1) / PG_ROWS);
  if (a.G) hipLaunchKernelGGL((acquire_grad_kernel<KS4, DT, true>), grid, dim3(256), 0, s, a, q);
  else hipLaunchKernelGGL((acquire_grad_kernel<KS4, DT, false>), grid, dim3(256), 0, s, a, q);
}

// ---- at most 64 inducing points of at most 16 dimensions: a block of 64 test points in one kernel (small_pg.h has the
// LDS shapes and the 64 x 64 products; REFINE: the body inside the loop of small_refine_kernel, refine.hip)
// DT: padded point dimension of the direct-difference covariance (d <= DT)
template <int DT>
__global__ __launch_bounds__(256) void small_predict_grad_kernel(SmallPredictGradArgs a) {
  constexpr bool ACQ = false, MV = false, REFINE = false;
  const AcqArgs q{};
  const MvArgs mv{};
  const SmallRefineArgs rf{};
#include "small_predict_grad_body.inc"
}
template <int DT>
__global__ __launch_bounds__(256) void small_acquire_grad_kernel(SmallPredictGradArgs a, AcqArgs q) {
  constexpr bool ACQ = true, MV = false, REFINE = false;
  const MvArgs mv{};
  const SmallRefineArgs rf{};
#include "small_predict_grad_body.inc"
}
template <int DT>
__global__ __launch_bounds__(256) void small_max_value_grad_kernel(SmallPredictGradArgs a, MvArgs mv) {
  constexpr bool ACQ = false, MV = true, REFINE = false;
  const AcqArgs q{};
  const SmallRefineArgs rf{};
#include "small_predict_grad_body.inc"
}

void small_pg_attrs() {
  static uint64_t done = 0;
  once_per_device(done, [] {
    auto set = [](const void* f, size_t bytes) {
      GPR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    };
    set(reinterpret_cast<const void*>(&small_predict_grad_kernel<4>), small_pg_lds(4));
    set(reinterpret_cast<const void*>(&small_predict_grad_kernel<8>), small_pg_lds(8));
    set(reinterpret_cast<const void*>(&small_predict_grad_kernel<16>), small_pg_lds(16));
    set(reinterpret_cast<const void*>(&small_acquire_grad_kernel<4>), small_pg_lds(4));
    set(reinterpret_cast<const void*>(&small_acquire_grad_kernel<8>), small_pg_lds(8));
    set(reinterpret_cast<const void*>(&small_acquire_grad_kernel<16>), small_pg_lds(16));
    set(reinterpret_cast<const void*>(&small_max_value_grad_kernel<4>), small_pg_lds(4));
    set(reinterpret_cast<const void*>(&small_max_value_grad_kernel<8>), small_pg_lds(8));
    set(reinterpret_cast<const void*>(&small_max_value_grad_kernel<16>), small_pg_lds(16));
  });
}

// out (full, symmetric) = I - B with B valid on its upper tiles
__global__ __launch_bounds__(256) void identity_minus_sym_kernel(const double* __restrict__ B, int mp, double* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (c >= mp) return;
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  out[(int64_t)r * mp + c] = (r == c ? 1.0 : 0.0) - B[(int64_t)lo * mp + hi];
}

}  // namespace

void launch_predict_grad(const PredictGradArgs& a, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.d > 64) {
    set_error("gprhip: the prediction gradient takes at most 64 point dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  if (a.d <= 4) launch_one<1, 1>(a, s);
  else if (a.d <= 8) launch_one<2, 1>(a, s);
  else if (a.d <= 16) launch_one<4, 1>(a, s);
  else if (a.d <= 32) launch_one<8, 2>(a, s);
  else launch_one<16, 4>(a, s);
  GPR_HIP(hipGetLastError());
}

void launch_small_predict_grad(const SmallPredictGradArgs& a, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.m > SM || a.d > 16) {
    set_error("gprhip: the one-kernel prediction gradient takes at most 64 inducing points of at most 16 dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  small_pg_attrs();
  auto go = [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL((small_predict_grad_kernel<DT>), dim3((a.rows + SRB - 1) / SRB), dim3(256), small_pg_lds(DT), s, a);
  };
  if (a.d <= 4) go(std::integral_constant<int, 4>{});
  else if (a.d <= 8) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 16>{});
  GPR_HIP(hipGetLastError());
}

void launch_acquire_grad(const PredictGradArgs& a, const AcqArgs& q, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.d > 64) {
    set_error("gprhip: the prediction gradient takes at most 64 point dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  if (a.d <= 4) launch_one_acq<1, 1>(a, q, s);
  else if (a.d <= 8) launch_one_acq<2, 1>(a, q, s);
  else if (a.d <= 16) launch_one_acq<4, 1>(a, q, s);
  else if (a.d <= 32) launch_one_acq<8, 2>(a, q, s);
  else launch_one_acq<16, 4>(a, q, s);
  GPR_HIP(hipGetLastError());
}

void launch_small_acquire_grad(const SmallPredictGradArgs& a, const AcqArgs& q, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.m > SM || a.d > 16) {
    set_error("gprhip: the one-kernel prediction gradient takes at most 64 inducing points of at most 16 dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  small_pg_attrs();
  auto go = [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL((small_acquire_grad_kernel<DT>), dim3((a.rows + SRB - 1) / SRB), dim3(256), small_pg_lds(DT), s, a, q);
  };
  if (a.d <= 4) go(std::integral_constant<int, 4>{});
  else if (a.d <= 8) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 16>{});
  GPR_HIP(hipGetLastError());
}

static void check_mv_args(const MvArgs& mv, bool with_var) {
  if (mv.n < 1 || mv.n > MV_MAX_EXTREMES || !mv.extremes || !with_var) {
    set_error("gprhip: the max-value epilogue takes 1 .. 64 extremes and the variance part");
    throw HipFail{ST_BAD_ARG};
  }
}

void launch_max_value_grad(const PredictGradArgs& a, const MvArgs& mv, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.d > 64) {
    set_error("gprhip: the prediction gradient takes at most 64 point dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  check_mv_args(mv, a.G != nullptr);
  const dim3 grid((a.rows + PG_ROWS - 1) / PG_ROWS);
  if (a.d <= 4) hipLaunchKernelGGL((max_value_grad_kernel<1, 1>), grid, dim3(256), 0, s, a, mv);
  else if (a.d <= 8) hipLaunchKernelGGL((max_value_grad_kernel<2, 1>), grid, dim3(256), 0, s, a, mv);
  else if (a.d <= 16) hipLaunchKernelGGL((max_value_grad_kernel<4, 1>), grid, dim3(256), 0, s, a, mv);
  else if (a.d <= 32) hipLaunchKernelGGL((max_value_grad_kernel<8, 2>), grid, dim3(256), 0, s, a, mv);
  else hipLaunchKernelGGL((max_value_grad_kernel<16, 4>), grid, dim3(256), 0, s, a, mv);
  GPR_HIP(hipGetLastError());
}

void launch_small_max_value_grad(const SmallPredictGradArgs& a, const MvArgs& mv, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.m > SM || a.d > 16) {
    set_error("gprhip: the one-kernel prediction gradient takes at most 64 inducing points of at most 16 dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  check_mv_args(mv, a.want_var != 0);
  small_pg_attrs();
  auto go = [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL((small_max_value_grad_kernel<DT>), dim3((a.rows + SRB - 1) / SRB), dim3(256), small_pg_lds(DT), s, a, mv);
  };
  if (a.d <= 4) go(std::integral_constant<int, 4>{});
  else if (a.d <= 8) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 16>{});
  GPR_HIP(hipGetLastError());
}

void launch_identity_minus_sym(const double* B, int mp, double* out, hipStream_t s) {
  hipLaunchKernelGGL(identity_minus_sym_kernel, dim3((mp + 255) / 256, mp), dim3(256), 0, s, B, mp, out);
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
