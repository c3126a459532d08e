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

#include "kernels.h"
#include "exp_fast.h"

namespace gprhip {

namespace {

typedef double pd4 __attribute__((ext_vector_type(4)));
typedef double pd2 __attribute__((ext_vector_type(2)));
// lane supplies A[lane&15][lane>>4] and B[lane>>4][lane&15]; accumulator element r is D[(lane>>4) + 4r][lane&15]
__device__ __forceinline__ pd4 pmfma4(double a, double b, pd4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

constexpr int PG_CP = 64;    // inducing columns per staged panel
constexpr int PG_ROWS = 64;  // test points per workgroup

// KS4 = ceil(d / 4) k-steps of the distance product, DT = ceil(d / 16) tiles of point dimensions, VAR: the variance part
template <int KS4, int DT, bool VAR>
__global__ __launch_bounds__(256) void predict_grad_kernel(PredictGradArgs a) {
  constexpr int DP = DT * 16, LDP = DP + 4;
  __shared__ double zs[PG_CP * LDP];
  __shared__ double zn[PG_CP];
  __shared__ double ts[PG_CP];
  __shared__ double sh[DP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  if (tid < DP) sh[tid] = tid < a.d ? a.shift[tid] : 0.0;
  __syncthreads();
  const int row0 = blockIdx.x * PG_ROWS + wv * 16;
  const int prow = row0 + l15;  // the test point of this lane's elements of E
  const bool live_r = prow < a.rows;
  const int mc = (a.m + 15) & ~15;  // columns walked (<= mp)
  const ExpK ek = exp_consts();

  double pb[KS4], pn = 0.0;
#pragma unroll
  for (int s = 0; s < KS4; ++s) {
    const int k = 4 * s + lq;
    const double v = (live_r && k < a.d) ? a.pts[(int64_t)prow * a.d + k] - sh[k] : 0.0;
    pb[s] = v;
    pn += v * v;
  }
  pn += __shfl_xor(pn, 16);
  pn += __shfl_xor(pn, 32);
  pd4 accm[DT], accv[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) accm[t] = accv[t] = (pd4){0, 0, 0, 0};
  double rsm = 0.0, rsv = 0.0;
  const int pcol = 4 * (l15 & 3) + (l15 >> 2);  // A rows of the distance product: 0 4 8 12 1 5 ...

  // columns cb + 4 lq .. + 3 of row prow of G
  auto load_g = [&](int cb, double (&o)[4]) {
    if (VAR && live_r && cb < mc) {
      const pd2* q = reinterpret_cast<const pd2*>(a.G + (int64_t)prow * a.mp + cb + 4 * lq);
      const pd2 u = q[0], w = q[1];
      o[0] = u.x; o[1] = u.y; o[2] = w.x; o[3] = w.y;
    } else {
      o[0] = o[1] = o[2] = o[3] = 0.0;
    }
  };
  double gv[4], gn[4];
  load_g(0, gv);
  for (int c0 = 0; c0 < mc; c0 += PG_CP) {
    __syncthreads();
    for (int idx = tid; idx < PG_CP * DP; idx += 256) {
      const int c = idx / DP, k = idx % DP, col = c0 + c;
      zs[c * LDP + k] = (col < a.m && k < a.d) ? a.Z[(int64_t)col * a.d + k] - sh[k] : 0.0;
    }
    if (tid < PG_CP) ts[tid] = c0 + tid < a.m ? a.tvec[c0 + tid] : 0.0;
    __syncthreads();
    {
      const int c = tid >> 2, q = tid & 3;
      double s2 = 0.0;
      for (int k = q; k < DP; k += 4) s2 += zs[c * LDP + k] * zs[c * LDP + k];
      s2 += __shfl_xor(s2, 1);
      s2 += __shfl_xor(s2, 2);
      if (q == 0) zn[c] = s2;
      __syncthreads();
    }
#pragma unroll 1
    for (int j = 0; j < PG_CP / 16; ++j) {
      const int cb = c0 + 16 * j;
      if (cb >= mc) break;
      load_g(cb + 16, gn);  // (beyond the last column block: nothing)
      pd4 s4 = (pd4){0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < KS4; ++s) s4 = pmfma4(zs[(16 * j + pcol) * LDP + 4 * s + lq], pb[s], s4);
      double em[4], ev[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * j + 4 * lq + r;
        const double dist = fmax(pn + zn[c] - 2.0 * s4[r], 0.0);
        const double kv = (live_r && c0 + c < a.m) ? exp_fast(a.log_sf2 + a.inv_ell2_05 * dist, ek) : 0.0;
        em[r] = kv * ts[c];
        ev[r] = kv * gv[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        rsm += em[r];
        if constexpr (VAR) rsv += ev[r];
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          const double zv = zs[(16 * j + 4 * lq + r) * LDP + 16 * t + l15];
          accm[t] = pmfma4(em[r], zv, accm[t]);
          if constexpr (VAR) accv[t] = pmfma4(ev[r], zv, accv[t]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) gv[r] = gn[r];
    }
  }
  rsm += __shfl_xor(rsm, 16);
  rsm += __shfl_xor(rsm, 32);  // every lane: rowsum(E_mean) of test point l15 = its mean
  rsv += __shfl_xor(rsv, 16);
  rsv += __shfl_xor(rsv, 32);
  if (lq == 0 && live_r) {
    if (a.means) a.means[prow] = rsm;
    if (VAR && a.vars) a.vars[prow] = (a.sf2 - rsv) + a.add;
  }
  const double inv_ell2 = -2.0 * a.inv_ell2_05;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = row0 + lq + 4 * r;
    const double rm = __shfl(rsm, lq + 4 * r), rv = __shfl(rsv, lq + 4 * r);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int dim = 16 * t + l15;
      if (orow < a.rows && dim < a.d) {
        const double pc = a.pts[(int64_t)orow * a.d + dim] - sh[dim];
        if (a.dmeans) a.dmeans[(int64_t)orow * a.ldg + dim] = -inv_ell2 * (pc * rm - accm[t][r]);
        if (VAR && a.dvars) a.dvars[(int64_t)orow * a.ldg + dim] = 2.0 * inv_ell2 * (pc * rv - accv[t][r]);
      }
    }
  }
}

template <int KS4, int DT>
void launch_one(const PredictGradArgs& a, hipStream_t s) {
  const dim3 grid((a.rows + PG_ROWS - 1) / PG_ROWS);
  if (a.G) hipLaunchKernelGGL((predict_grad_kernel<KS4, DT, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((predict_grad_kernel<KS4, DT, false>), grid, dim3(256), 0, s, a);
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

// DT: padded point dimension of the direct-difference covariance (d <= DT)
template <int DT>
__global__ __launch_bounds__(256) void small_predict_grad_kernel(SmallPredictGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pg_lds[];
  double* const Ui = pg_lds;            // [SM][SLD]
  double* const Ri = Ui + SM * SLD;     // [SM][SLD]
  double* const Kt = Ri + SM * SLD;     // [SRB][SLD] K
  double* const Wk = Kt + SRB * SLD;    // [SRB][SLD] V, Q, H, then E_var
  double* const zs = Wk + SRB * SLD;    // [SM][LDZ] Z - s (dimensions >= d zero)
  double* const xs = zs + SM * LDZ;     // [SRB][DT] test points
  double* const tv = xs + SRB * DT;     // [SM] mean coefficients
  double* const sh = tv + SM;           // [16] s
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const ExpK ek = exp_consts();
  const bool var = a.want_var != 0;
  if (var) {
    load_corner(a.uinv, a.mp, Ui, tid);
    load_corner(a.rinv, a.mp, Ri, tid);
  }
  if (tid < SM) tv[tid] = tid < a.m ? a.tvec[tid] : 0.0;
  if (tid >= 64 && tid < 80) sh[tid - 64] = tid - 64 < a.d ? a.shift[tid - 64] : 0.0;
  const int col = lane;
  const bool live_c = col < a.m;
  double z[DT];
#pragma unroll
  for (int k = 0; k < DT; ++k) z[k] = (k < a.d && live_c) ? a.Z[(int64_t)col * a.d + k] : 0.0;
  const int r0 = blockIdx.x * SRB;
  for (int idx = tid; idx < SRB * DT; idx += 256) {
    const int r = idx / DT, k = idx % DT;
    xs[idx] = (k < a.d && r0 + r < a.rows) ? a.pts[(int64_t)(r0 + r) * a.d + k] : 0.0;
  }
  __syncthreads();
  for (int idx = tid; idx < SM * 16; idx += 256) {
    const int c = idx >> 4, k = idx & 15;
    zs[c * LDZ + k] = (c < a.m && k < a.d) ? a.Z[(int64_t)c * a.d + k] - sh[k] : 0.0;
  }
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int r = wv * 16 + i;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DT; ++k) {
      const double diff = xs[r * DT + k] - z[k];
      acc = acc + diff * diff;
    }
    Kt[r * SLD + col] = (r0 + r < a.rows && live_c) ? exp_fast(a.cp.log_sf2 + a.cp.inv_ell2_05 * acc, ek) : 0.0;
  }
  __syncthreads();
  // mean part: E_mean = K .* (1 t^T) formed as the A operand
  pd4 am = pd4{0.0, 0.0, 0.0, 0.0}, av = pd4{0.0, 0.0, 0.0, 0.0};
  double rsm = 0.0, rsv = 0.0;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int c = 4 * kk + lq;
    const double e = Kt[(16 * wv + l15) * SLD + c] * tv[c];
    rsm += e;
    am = pmfma4(e, zs[c * LDZ + l15], am);
  }
  if (var) {
    pd4 accv[4], acc[4];
    rows_times<false>(Kt, Ui, wv, l15, lq, accv);  // V = K U^-1
    store_rows(Wk, accv, wv, l15, lq);
    rows_times<false>(Wk, Ri, wv, l15, lq, acc);   // Q = V R~^-1
    store_rows(Wk, acc, wv, l15, lq);
    rows_times<true>(Wk, Ri, wv, l15, lq, acc);    // Q R~^-T
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = accv[ct] - acc[ct];  // H = V - Q R~^-T
    store_rows(Wk, acc, wv, l15, lq);
    rows_times<true>(Wk, Ui, wv, l15, lq, acc);    // G = H U^-T
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int o = (16 * wv + lq + 4 * r) * SLD + 16 * ct + l15;
        Wk[o] = Kt[o] * acc[ct][r];  // E_var = K .* G
      }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int c = 4 * kk + lq;
      const double e = Wk[(16 * wv + l15) * SLD + c];
      rsv += e;
      av = pmfma4(e, zs[c * LDZ + l15], av);
    }
  }
  rsm += __shfl_xor(rsm, 16);
  rsm += __shfl_xor(rsm, 32);  // every lane: the row sum of test point 16 wv + l15
  rsv += __shfl_xor(rsv, 16);
  rsv += __shfl_xor(rsv, 32);
  const int prow = r0 + 16 * wv + l15;
  if (lq == 0 && prow < a.rows) {
    if (a.means) a.means[prow] = rsm;
    if (var && a.vars) a.vars[prow] = (a.cp.sf2 - rsv) + a.add;
  }
  const double inv_ell2 = -2.0 * a.cp.inv_ell2_05;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lrow = 16 * wv + lq + 4 * r, orow = r0 + lrow;
    const double rm = __shfl(rsm, lq + 4 * r), rv = __shfl(rsv, lq + 4 * r);
    if (orow < a.rows && l15 < a.d) {
      const double pc = xs[lrow * DT + l15] - sh[l15];
      if (a.dmeans) a.dmeans[(int64_t)orow * a.ldg + l15] = -inv_ell2 * (pc * rm - am[r]);
      if (var && a.dvars) a.dvars[(int64_t)orow * a.ldg + l15] = 2.0 * inv_ell2 * (pc * rv - av[r]);
    }
  }
}

size_t small_pg_lds(int DT) { return (size_t)(4 * SM * SLD + SM * LDZ + SRB * DT + SM + 16) * sizeof(double); }

void small_pg_attrs() {
  static uint64_t done = 0;
  once_per_device(done, [] {
    auto set = [](const void* f, size_t bytes) {
      GPR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    };
    set(reinterpret_cast<const void*>(&small_predict_grad_kernel<4>), small_pg_lds(4));
    set(reinterpret_cast<const void*>(&small_predict_grad_kernel<8>), small_pg_lds(8));
    set(reinterpret_cast<const void*>(&small_predict_grad_kernel<16>), small_pg_lds(16));
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

void launch_identity_minus_sym(const double* B, int mp, double* out, hipStream_t s) {
  hipLaunchKernelGGL(identity_minus_sym_kernel, dim3((mp + 255) / 256, mp), dim3(256), 0, s, B, mp, out);
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
