// Row passes and finish stage of problems with few inducing points (m <= 64, d <= 16 point dimensions -- D <= 64 input
// dimensions in front of a projection --, any number of rows).  The reference's own shapes (n = 1000..2000, m = 10..50,
// test/save_data.ml, test/gen_data.ml) spend their time in launches, not in arithmetic -- through the engine a gradient
// evaluation is 9 contraction launches of 16-22 us each plus ~20 small kernels, 0.40 ms; and with many rows the engine
// pads m to its 128-wide tile (6.5x the flops of m = 50).  Here each pass is ONE kernel per 64-row block that keeps the block's rows of K, V, Q' and X in LDS and the 64 x 64 corners of U^-1 / R~^-1 beside
// them, plus one fixed-order reduction of the per-workgroup partial sums into the exchange buffers -- same buffers, same
// layout as the engine path writes (do_pass1 / do_pass2), so everything around the two passes is shared.
//   pass 1: K (lib/cov_se_iso.ml:128-159, lib/cov_se_fat.ml:224-240), V = K U^-1 (lib/fitc_gp.ml:226-227), r, s, 1/s
//           (:155-166, :222-223), B~ part = V^T diag(is) V, c~ part = V^T (is y)
//   pass 2: Q' = V R~^-1, q_diag, w, v (:1048, :1092-1108, :1158-1181), X~ = diag(is) Q' R~^-T - diag(v) V - w t~^T,
//           X = X~ U^-T (:931-939, :1204-1206), E = X .* K column sums (:975-1003), G~ part = V^T diag(v) V (:1198-1203)
// All products run as v_mfma_f64_16x16x4_f64 tiles on LDS operands: wavefront w owns rows 16w..16w+15 of the block.
#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "exp_fast.h"

namespace gprhip {

namespace {

constexpr int SM = 64;    // inducing points (padded) the small path handles
constexpr int SLD = 66;   // leading dimension of the 64 x 64 LDS matrices
constexpr int SRB = 64;   // training points per block iteration
constexpr int P1LEN = SM * SM + SM + 4;  // pass-1 partial of a workgroup: B~ part | c~ part | sum log s, sum y^2/s, sum r/s, -
// pass-2 partial: G~ part | column sums: E, p_k E (d), x_big E (D), with multiscales p_k^2 E (d) | `Proj term (D d) | 8 scalars
__host__ __device__ constexpr int p2len(int d, int D, int ms = 0) {
  return SM * SM + (1 + d + D + (ms ? d : 0)) * SM + D * d + 8;
}

typedef double sd4 __attribute__((ext_vector_type(4)));
// lane supplies A[lane&15][lane>>4] and B[lane>>4][lane&15]; accumulator element r is D[(lane>>4) + 4r][lane&15]
__device__ __forceinline__ sd4 mfma_f64(double a, double b, sd4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ double sum16(double v) {  // over the 16 lanes that share lane >> 4
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}
__device__ __forceinline__ double sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// rows [16 wv, 16 wv + 16) of  A (LDS, [64][SLD]) times  B (LDS, [64][SLD]; TRANS: times B^T)  -> acc[ct], ct = column tile.
// Fully unrolled, all fragments of a half of the k-range loaded before its 32 MFMAs: with the loop left rolled every
// step waits for its own LDS reads and a product takes 2.5-4.5 us instead of ~2.
// (NB = k-steps per batch: 8, or 4 where registers are short)
template <bool TRANS, int NB = 8>
__device__ __forceinline__ void rows_times(const double* A, const double* B, int wv, int l15, int lq, sd4 (&acc)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = sd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int h = 0; h < 16 / NB; ++h) {
    double af[NB], bf[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int kk = NB * h + j;
      af[j] = A[(16 * wv + l15) * SLD + 4 * kk + lq];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        bf[j][ct] = TRANS ? B[(16 * ct + l15) * SLD + 4 * kk + lq] : B[(4 * kk + lq) * SLD + 16 * ct + l15];
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f64(af[j], bf[j][ct], acc[ct]);
  }
}

// acc[ct] += (T^T diag(wt) T) tile (wv, ct) over the 64 rows of T (LDS)
__device__ __forceinline__ void gram_update(const double* T, const double* wt, int wv, int l15, int lq, sd4 (&acc)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double af[8], bf[8][4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 4 * (8 * h + j) + lq;
      af[j] = T[k * SLD + 16 * wv + l15] * wt[k];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) bf[j][ct] = T[k * SLD + 16 * ct + l15];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f64(af[j], bf[j][ct], acc[ct]);
  }
}

// sum_g part[g * stride] over the workgroups' partials, in order; sixty-four loads in flight at a time from 64 partials on
// (a batch is one memory round trip: with sixteen per batch 256 partials were sixteen dependent round trips, 26 us of a
// reduction whose ten workgroups do nothing else -- timeline at n = 10 000, m = 256), sixteen below that.  Same order of
// additions either way.
__device__ __forceinline__ double sum_parts(const double* __restrict__ part, int64_t stride, int ng) {
  double acc = 0.0;
  int g0 = 0;
  for (; g0 + 64 <= ng; g0 += 64) {
    double v[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) v[j] = part[(int64_t)(g0 + j) * stride];
#pragma unroll
    for (int j = 0; j < 64; ++j) acc += v[j];
  }
  for (; g0 < ng; g0 += 16) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (g0 + j < ng) ? part[(int64_t)(g0 + j) * stride] : 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc += v[j];
  }
  return acc;
}

// 64 x 64 corner of a row-major mp x mp matrix -> LDS; eight 16-byte loads per thread, all issued before the first store
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

}  // namespace

// workgroups of a pass at most (each walks blocks b, b + groups, ...): what the chip holds at once -- two per CU for
// pass 1 (77 KB of LDS each), one per CU for pass 2 (150 KB)
constexpr int SMALL_GROUPS1 = 512, SMALL_GROUPS2 = 256;
int64_t small_part_len(int d, int D) {
  return std::max((int64_t)SMALL_GROUPS1 * P1LEN, (int64_t)SMALL_GROUPS2 * p2len(d, D, 1));
}
static int small_groups(int rows_p, int cap) { return std::min(cap, rows_p / SRB); }

// MS: Cov_se_fat multiscales (lib/cov_se_fat.ml:241-251; a.cp.ms = exp(log_multiscales_m05) + 1/2 as [mp][d]): the exponent
// accumulates diff * (diff / scale) + log(scale) per dimension, as cov_cross_ms_kernel
// The kernels of an evaluation chain come in pairs ("Batched evaluation"): the single one takes its
// argument struct by value; the batched one runs one lane per blockIdx.y and reads that lane's struct from a device
// array -- a uniform read, so it stays in scalar registers as the kernel arguments do.  Both compile the same body text
// (small_*_body.inc) with the same blockIdx.x / gridDim.x, so a lane's numbers are those of the single launch; the
// body is included, not called: behind a by-reference call the single pass-2 kernels came out 60-100 registers heavier.
template <int DT, bool MS>
__global__ __launch_bounds__(256) void small_pass1_kernel(SmallPass1Args a) {
#include "small_pass1_body.inc"
}
template <int DT, bool MS>
__global__ __launch_bounds__(256) void small_pass1_batch_kernel(const SmallPass1Args* __restrict__ lanes, int64_t stride) {
  const SmallPass1Args a = lane_args(lanes, stride);
#include "small_pass1_body.inc"
}


// exchange-1 buffer from the pass-1 partials, workgroups summed in order: the (0,0) upper tile (128 x 128; zero outside
// the 64 x 64 corner), c~ (mp entries) and the scalar tail
__device__ __forceinline__ void small_reduce1_body(const double* __restrict__ part, int ng, int mp,
                                                   double* __restrict__ tile, double* __restrict__ cvec,
                                                   double* __restrict__ tail) {
  const int tid = threadIdx.x;
  if (blockIdx.x < TILE * TILE / 256) {
    const int idx = blockIdx.x * 256 + tid, r = idx / TILE, c = idx % TILE;
    tile[idx] = (r < SM && c < SM) ? sum_parts(part + r * SM + c, P1LEN, ng) : 0.0;
    return;
  }
  if (tid < mp) cvec[tid] = (tid < SM) ? sum_parts(part + SM * SM + tid, P1LEN, ng) : 0.0;
  else if (tid >= 192 && tid < 196) tail[tid - 192] = sum_parts(part + SM * SM + SM + (tid - 192), P1LEN, ng);
}
__global__ __launch_bounds__(256) void small_reduce1_kernel(const double* __restrict__ part, int ng, int mp,
                                                            double* __restrict__ tile, double* __restrict__ cvec,
                                                            double* __restrict__ tail) {
  small_reduce1_body(part, ng, mp, tile, cvec, tail);
}
__global__ __launch_bounds__(256) void small_reduce1_batch_kernel(const SmallReduce1Args* __restrict__ lanes, int64_t stride) {
  const SmallReduce1Args a = lane_args(lanes, stride);
  small_reduce1_body(a.part, a.ng, a.mp, a.tile, a.cvec, a.tail);
}

// DT: padded point dimension (d <= DT); DBT: padded dimension of the original inputs of a projected kernel (D <= DBT)
// MS (multiscales, d <= 8): K as grad_fused_ms_kernel forms it, the extra column sums of p_k^2 E (`Log_multiscale_m05,
// lib/cov_se_fat.ml:598-622), and for the `Proj derivative one weight per (row, dimension), sum_c E_rc / ms_kc (:585-595),
// formed from the E tile in LDS.  MS instantiations take the staged-inputs (WIDE) route for any D.
// KR: K_nm of pass 1 is read back (a.Kin, [rows_p][64]: requested at the top of a block, parked in V's tile once V is done
// with) instead of recomputed -- the sixteen exp per thread and block are a fifth of this kernel otherwise; instantiated
// for d <= 8, D <= 16, no multiscales.
template <int DT, int DBT, bool MS, bool KR = false>
__global__ __launch_bounds__(256) void small_pass2_kernel(SmallPass2Args a) {
#include "small_pass2_body.inc"
}
template <int DT, int DBT, bool MS, bool KR = false>
__global__ __launch_bounds__(256) void small_pass2_batch_kernel(const SmallPass2Args* __restrict__ lanes, int64_t stride) {
  const SmallPass2Args a = lane_args(lanes, stride);
#include "small_pass2_body.inc"
}

// exchange-2 buffer from the pass-2 partials, every entry written: the (0,0) tile (zero outside its 64 x 64 corner), the
// column block (col_rows x mp; rows 0..d+D, columns < 64 carry sums), the `Proj second term and the scalar tail
__device__ __forceinline__ void small_reduce2_body(const double* __restrict__ part, int ng, int mp, int d, int D,
                                                   int ms, int col_rows, double* __restrict__ tile,
                                                   double* __restrict__ colblk, double* __restrict__ proj,
                                                   double* __restrict__ tail) {
  const int plen = p2len(d, D, ms), ncq = 1 + d + D + (ms ? d : 0);
  int idx = blockIdx.x * 256 + threadIdx.x;
  // nproj: the partials' `Proj entries (none without a projection); nprojbuf: the buffer's, which a Cov_se_fat layout has
  // with or without one -- all of them are written
  const int ntile = TILE * TILE, ncol = col_rows * mp, nproj = D * d, nprojbuf = (int)(tail - proj);
  int src = -1;
  double* dst;
  if (idx < ntile) {
    const int r = idx / TILE, c = idx % TILE;
    dst = tile + idx;
    if (r < SM && c < SM) src = r * SM + c;
  } else if ((idx -= ntile) < ncol) {
    const int q = idx / mp, c = idx % mp;
    dst = colblk + idx;
    if (q < ncq && c < SM) src = SM * SM + q * SM + c;
  } else if ((idx -= ncol) < nprojbuf) {
    dst = proj + idx;
    if (idx < nproj) src = SM * SM + ncq * SM + idx;
  } else if ((idx -= nprojbuf) < 8) {
    dst = tail + idx;
    src = SM * SM + ncq * SM + nproj + idx;
  } else {
    return;
  }
  *dst = (src >= 0) ? sum_parts(part + src, plen, ng) : 0.0;
}
__global__ __launch_bounds__(256) void small_reduce2_kernel(const double* __restrict__ part, int ng, int mp, int d, int D,
                                                            int ms, int col_rows, double* __restrict__ tile,
                                                            double* __restrict__ colblk, double* __restrict__ proj,
                                                            double* __restrict__ tail) {
  small_reduce2_body(part, ng, mp, d, D, ms, col_rows, tile, colblk, proj, tail);
}
__global__ __launch_bounds__(256) void small_reduce2_batch_kernel(const SmallReduce2Args* __restrict__ lanes, int64_t stride) {
  const SmallReduce2Args a = lane_args(lanes, stride);
  small_reduce2_body(a.part, a.ng, a.mp, a.d, a.D, a.ms, a.col_rows, a.tile, a.colblk, a.proj, a.tail);
}

// Finish stage of a small gradient evaluation in one workgroup (the m x m work of do_finish_enqueue on 64 x 64 corners):
//   B~^-1 = R~^-1 R~^-T (Utils.ichol, lib/utils.ml:110-113),  W~ = I - B~^-1 - t~ t~^T - G~,  W = U^-1 W~ U^-T
//   (lib/fitc_gp.ml:1196-1203), the trace terms of W against K_m and its derivatives (km_traces_kernel: :956-973,
//   lib/utils.ml:196-220), diag W, and the tails of both exchange buffers gathered behind the result block.
// MS: the multiscale trace terms of km_traces_ms_kernel (lib/cov_se_fat.ml:441-516)
template <int DT, bool MS>
__global__ __launch_bounds__(256) void small_finish_kernel(SmallFinishArgs a) {
#include "small_finish_body.inc"
}
template <int DT, bool MS>
__global__ __launch_bounds__(256) void small_finish_batch_kernel(const SmallFinishArgs* __restrict__ lanes, int64_t stride) {
  const SmallFinishArgs a = lane_args(lanes, stride);
#include "small_finish_body.inc"
}

// Means.calc / Variances.calc (lib/fitc_gp.ml:418-425, :498-518) for a block of 64 test points in one kernel: K tile,
// mean = K t, V = K U^-1, Q = V R~^-1, var = (sf2 - (|V_i|^2 - |Q_i|^2)) + add -- what do_predict otherwise does with seven
// launches per chunk (covariance, two triangular products, three row kernels, the combination).
template <int DT>
__global__ __launch_bounds__(256) void small_predict_kernel(SmallPredictArgs a) {
  extern __shared__ __attribute__((aligned(16))) double small_lds[];
  double* const Ui = small_lds;         // [SM][SLD]
  double* const Ri = Ui + SM * SLD;     // [SM][SLD]
  double* const Kt = Ri + SM * SLD;     // [SRB][SLD] K, then V in place
  double* const xs = Kt + SRB * SLD;    // [SRB][DT]
  double* const tv = xs + SRB * DT;     // [SM] mean coefficients
  double* const rk = tv + SM;           // [SRB] |V_i|^2
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const ExpK ek = exp_consts();
  if (a.vars) {
    load_corner(a.uinv, a.mp, Ui, tid);
    load_corner(a.rinv, a.mp, Ri, tid);
  }
  if (tid < SM) tv[tid] = tid < a.m ? a.tvec[tid] : 0.0;
  const int col = lane, rg = wv;
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
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int r = rg * 16 + i;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DT; ++k) {
      const double diff = xs[r * DT + k] - z[k];
      acc = acc + diff * diff;
    }
    Kt[r * SLD + col] = (r0 + r < a.rows && live_c) ? exp_fast(a.cp.log_sf2 + a.cp.inv_ell2_05 * acc, ek) : 0.0;
  }
  __syncthreads();
  if (a.means) {  // four threads per row, sixteen columns each
    const int row = tid >> 2, part = tid & 3;
    double sum = 0.0;
#pragma unroll
    for (int c = 16 * part; c < 16 * part + 16; ++c) sum += Kt[row * SLD + c] * tv[c];
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if (part == 0 && r0 + row < a.rows) a.means[r0 + row] = sum;
  }
  if (!a.vars) return;
  __syncthreads();  // (the mean phase read rows of other wavefronts)
  sd4 acc[4];
  rows_times<false>(Kt, Ui, wv, l15, lq, acc);  // V = K U^-1
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s2 = 0.0;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) s2 += acc[ct][r] * acc[ct][r];
    s2 = sum16(s2);
    const int row = 16 * wv + lq + 4 * r;
    if (l15 == 0) rk[row] = s2;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) Kt[row * SLD + 16 * ct + l15] = acc[ct][r];  // rows of this wavefront: in place
  }
  rows_times<false>(Kt, Ri, wv, l15, lq, acc);  // Q = V R~^-1
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s2 = 0.0;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) s2 += acc[ct][r] * acc[ct][r];
    s2 = sum16(s2);
    const int row = 16 * wv + lq + 4 * r;
    // prior_variance -. (k -. b), lib/fitc_gp.ml:475 (as variance_combine_kernel)
    if (l15 == 0 && r0 + row < a.rows) a.vars[r0 + row] = (a.cp.sf2 - (rk[row] - s2)) + a.add;
  }
}

static size_t small_lds4(int DT) { return (size_t)(3 * SM * SLD + SRB * DT + SM + SRB) * sizeof(double); }

static size_t small_lds1(int DT) { return (size_t)(2 * SM * SLD + SRB * DT + 3 * SRB) * sizeof(double); }
static size_t small_lds3(int DT, bool ms = false) {
  return (size_t)(4 * SM * SLD + SM * DT + SM + 4 * SM + (ms ? SM * DT : 0)) * sizeof(double);
}
static size_t small_lds2(int DT, bool ms = false) {
  return (size_t)(4 * SM * SLD + SRB * DT + 6 * SRB + 2 * SM + 4 * SM + (ms ? 2 * SM * DT : 0)) * sizeof(double);
}

template <typename F>
static void small_dispatch(int d, F&& go) {
  if (d <= 4) go(std::integral_constant<int, 4>{});
  else if (d <= 8) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 16>{});
}

static void small_attrs() {
  static uint64_t done = 0;
  once_per_device(done, [] {
    auto set = [](const void* f, size_t bytes) {
      GPR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    };
#define GPRHIP_SMALL_SET(DT)                                                                                   \
  set(reinterpret_cast<const void*>(&small_pass1_kernel<DT, false>), small_lds1(DT));                          \
  set(reinterpret_cast<const void*>(&small_pass2_kernel<DT, 1, false>), small_lds2(DT));                       \
  set(reinterpret_cast<const void*>(&small_pass2_kernel<DT, 16, false>), small_lds2(DT));                      \
  set(reinterpret_cast<const void*>(&small_pass2_kernel<DT, 64, false>), small_lds2(DT));                      \
  set(reinterpret_cast<const void*>(&small_pass2_kernel<(DT > 8 ? 8 : DT), 1, false, true>), small_lds2(DT > 8 ? 8 : DT));  \
  set(reinterpret_cast<const void*>(&small_pass2_kernel<(DT > 8 ? 8 : DT), 16, false, true>), small_lds2(DT > 8 ? 8 : DT)); \
  set(reinterpret_cast<const void*>(&small_finish_kernel<DT, false>), small_lds3(DT));                           \
  set(reinterpret_cast<const void*>(&small_pass1_batch_kernel<DT, false>), small_lds1(DT));                    \
  set(reinterpret_cast<const void*>(&small_pass2_batch_kernel<DT, 1, false>), small_lds2(DT));                 \
  set(reinterpret_cast<const void*>(&small_pass2_batch_kernel<DT, 16, false>), small_lds2(DT));                \
  set(reinterpret_cast<const void*>(&small_pass2_batch_kernel<DT, 64, false>), small_lds2(DT));                \
  set(reinterpret_cast<const void*>(&small_pass2_batch_kernel<(DT > 8 ? 8 : DT), 1, false, true>), small_lds2(DT > 8 ? 8 : DT));  \
  set(reinterpret_cast<const void*>(&small_pass2_batch_kernel<(DT > 8 ? 8 : DT), 16, false, true>), small_lds2(DT > 8 ? 8 : DT)); \
  set(reinterpret_cast<const void*>(&small_finish_batch_kernel<DT, false>), small_lds3(DT));
    GPRHIP_SMALL_SET(4)
    GPRHIP_SMALL_SET(8)
    GPRHIP_SMALL_SET(16)
#undef GPRHIP_SMALL_SET
    set(reinterpret_cast<const void*>(&small_predict_kernel<4>), small_lds4(4));
    set(reinterpret_cast<const void*>(&small_predict_kernel<8>), small_lds4(8));
    set(reinterpret_cast<const void*>(&small_predict_kernel<16>), small_lds4(16));
#define GPRHIP_SMALL_SET_MS(DT)                                                                                \
  set(reinterpret_cast<const void*>(&small_pass1_kernel<DT, true>), small_lds1(DT));                           \
  set(reinterpret_cast<const void*>(&small_pass2_kernel<DT, 1, true>), small_lds2(DT, true));                  \
  set(reinterpret_cast<const void*>(&small_pass2_kernel<DT, 64, true>), small_lds2(DT, true));                 \
  set(reinterpret_cast<const void*>(&small_finish_kernel<DT, true>), small_lds3(DT, true));                    \
  set(reinterpret_cast<const void*>(&small_pass1_batch_kernel<DT, true>), small_lds1(DT));                     \
  set(reinterpret_cast<const void*>(&small_pass2_batch_kernel<DT, 1, true>), small_lds2(DT, true));            \
  set(reinterpret_cast<const void*>(&small_pass2_batch_kernel<DT, 64, true>), small_lds2(DT, true));           \
  set(reinterpret_cast<const void*>(&small_finish_batch_kernel<DT, true>), small_lds3(DT, true));
    GPRHIP_SMALL_SET_MS(4)
    GPRHIP_SMALL_SET_MS(8)
#undef GPRHIP_SMALL_SET_MS
  });
}

bool small_path_fits(int m, int mp, int d, int D, int64_t rows, bool ms) {
  // (rows: no structural limit -- the partial sums are per workgroup, not per block; 4M rows is where int indices of the
  //  row kernels around it were last checked.  Multiscales: d <= 8, their extra LDS arrays do not fit beside d = 16.)
  return m <= SM && mp == TILE && d <= (ms ? 8 : 16) && D <= 64 && rows <= (int64_t(1) << 22);
}

void launch_small_pass1(const SmallPass1Args& a, double* tile, double* cvec, double* tail, hipStream_t s) {
  small_attrs();
  const int ng = small_groups(a.rows_p, SMALL_GROUPS1);
  const bool ms = a.cp.ms != nullptr;
  small_dispatch(a.d, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT <= 8) {
      if (ms) {
        hipLaunchKernelGGL((small_pass1_kernel<DT, true>), dim3(ng), dim3(256), small_lds1(DT), s, a);
        return;
      }
    }
    hipLaunchKernelGGL((small_pass1_kernel<DT, false>), dim3(ng), dim3(256), small_lds1(DT), s, a);
  });
  hipLaunchKernelGGL(small_reduce1_kernel, dim3(TILE * TILE / 256 + 1), dim3(256), 0, s, a.part, ng, a.mp, tile, cvec, tail);
  GPR_HIP(hipGetLastError());
}

// ---- the batched launches: `count` lanes of one shape (rows, d, option shape: `a0` is lane 0's struct on the host, which
// chooses the instantiation and the grid exactly as the single launcher does); d_lanes / d_red: the device arrays
int small_pass1_groups(int rows_p) { return small_groups(rows_p, SMALL_GROUPS1); }
int small_pass2_groups(int rows_p) { return small_groups(rows_p, SMALL_GROUPS2); }

void launch_small_pass1_batch(const SmallPass1Args& a0, const SmallPass1Args* d_lanes, const SmallReduce1Args* d_red, int count,
                              int64_t stride, hipStream_t s) {
  small_attrs();
  const int ng = small_groups(a0.rows_p, SMALL_GROUPS1);
  const bool ms = a0.cp.ms != nullptr;
  small_dispatch(a0.d, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT <= 8) {
      if (ms) {
        hipLaunchKernelGGL((small_pass1_batch_kernel<DT, true>), dim3(ng, count), dim3(256), small_lds1(DT), s, d_lanes, stride);
        return;
      }
    }
    hipLaunchKernelGGL((small_pass1_batch_kernel<DT, false>), dim3(ng, count), dim3(256), small_lds1(DT), s, d_lanes, stride);
  });
  hipLaunchKernelGGL(small_reduce1_batch_kernel, dim3(TILE * TILE / 256 + 1, count), dim3(256), 0, s, d_red, stride);
  GPR_HIP(hipGetLastError());
}

void launch_small_pass2_batch(const SmallPass2Args& a0, int col_rows, const SmallPass2Args* d_lanes, const SmallReduce2Args* d_red,
                              int count, int64_t stride, hipStream_t s) {
  small_attrs();
  const int ng = small_groups(a0.rows_p, SMALL_GROUPS2);
  const bool ms = a0.cp.ms != nullptr;
  const dim3 grid(ng, count);
  small_dispatch(a0.d, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT <= 8) {
      if (ms) {
        if (a0.D == 0) hipLaunchKernelGGL((small_pass2_batch_kernel<DT, 1, true>), grid, dim3(256), small_lds2(DT, true), s, d_lanes, stride);
        else hipLaunchKernelGGL((small_pass2_batch_kernel<DT, 64, true>), grid, dim3(256), small_lds2(DT, true), s, d_lanes, stride);
        return;
      }
    }
    if constexpr (DT <= 8) {
      if (a0.Kin && a0.D <= 16) {
        if (a0.D == 0) hipLaunchKernelGGL((small_pass2_batch_kernel<DT, 1, false, true>), grid, dim3(256), small_lds2(DT), s, d_lanes, stride);
        else hipLaunchKernelGGL((small_pass2_batch_kernel<DT, 16, false, true>), grid, dim3(256), small_lds2(DT), s, d_lanes, stride);
        return;
      }
    }
    if (a0.D == 0) hipLaunchKernelGGL((small_pass2_batch_kernel<DT, 1, false>), grid, dim3(256), small_lds2(DT), s, d_lanes, stride);
    else if (a0.D <= 16) hipLaunchKernelGGL((small_pass2_batch_kernel<DT, 16, false>), grid, dim3(256), small_lds2(DT), s, d_lanes, stride);
    else hipLaunchKernelGGL((small_pass2_batch_kernel<DT, 64, false>), grid, dim3(256), small_lds2(DT), s, d_lanes, stride);
  });
  // the buffer's `Proj block is dbig x d, projection or not: col_rows = d + 1 (Cov_se_iso, dbig = 0) or d + 1 + dbig + d
  const int dbig = col_rows > a0.d + 1 ? col_rows - 1 - 2 * a0.d : 0;
  const int nout = TILE * TILE + col_rows * a0.mp + dbig * a0.d + 8;
  hipLaunchKernelGGL(small_reduce2_batch_kernel, dim3((nout + 255) / 256, count), dim3(256), 0, s, d_red, stride);
  GPR_HIP(hipGetLastError());
}

void launch_small_finish_batch(const SmallFinishArgs& a0, const SmallFinishArgs* d_lanes, int count, int64_t stride, hipStream_t s) {
  small_attrs();
  small_dispatch(a0.d, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT <= 8) {
      if (a0.ms) {
        hipLaunchKernelGGL((small_finish_batch_kernel<DT, true>), dim3(1, count), dim3(256), small_lds3(DT, true), s, d_lanes, stride);
        return;
      }
    }
    hipLaunchKernelGGL((small_finish_batch_kernel<DT, false>), dim3(1, count), dim3(256), small_lds3(DT), s, d_lanes, stride);
  });
  GPR_HIP(hipGetLastError());
}

void launch_small_pass2(const SmallPass2Args& a, int col_rows, double* tile, double* colblk, double* proj, double* tail,
                        hipStream_t s) {
  small_attrs();
  const int ng = small_groups(a.rows_p, SMALL_GROUPS2);
  const bool ms = a.cp.ms != nullptr;
  small_dispatch(a.d, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT <= 8) {
      if (ms) {
        if (a.D == 0) hipLaunchKernelGGL((small_pass2_kernel<DT, 1, true>), dim3(ng), dim3(256), small_lds2(DT, true), s, a);
        else hipLaunchKernelGGL((small_pass2_kernel<DT, 64, true>), dim3(ng), dim3(256), small_lds2(DT, true), s, a);
        return;
      }
    }
    if constexpr (DT <= 8) {
      if (a.Kin && a.D <= 16) {
        if (a.D == 0) hipLaunchKernelGGL((small_pass2_kernel<DT, 1, false, true>), dim3(ng), dim3(256), small_lds2(DT), s, a);
        else hipLaunchKernelGGL((small_pass2_kernel<DT, 16, false, true>), dim3(ng), dim3(256), small_lds2(DT), s, a);
        return;
      }
    }
    if (a.D == 0) hipLaunchKernelGGL((small_pass2_kernel<DT, 1, false>), dim3(ng), dim3(256), small_lds2(DT), s, a);
    else if (a.D <= 16) hipLaunchKernelGGL((small_pass2_kernel<DT, 16, false>), dim3(ng), dim3(256), small_lds2(DT), s, a);
    else hipLaunchKernelGGL((small_pass2_kernel<DT, 64, false>), dim3(ng), dim3(256), small_lds2(DT), s, a);
  });
  const int nout = TILE * TILE + col_rows * a.mp + (int)(tail - proj) + 8;  // (the buffer's `Proj block: dbig x d, projection or not)
  hipLaunchKernelGGL(small_reduce2_kernel, dim3((nout + 255) / 256), dim3(256), 0, s, a.part, ng, a.mp, a.d, a.D, ms ? 1 : 0,
                     col_rows, tile, colblk, proj, tail);
  GPR_HIP(hipGetLastError());
}

void launch_small_predict(const SmallPredictArgs& a, hipStream_t s) {
  small_attrs();
  small_dispatch(a.d, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL((small_predict_kernel<DT>), dim3((a.rows + SRB - 1) / SRB), dim3(256), small_lds4(DT), s, a);
  });
  GPR_HIP(hipGetLastError());
}

void launch_small_finish(const SmallFinishArgs& a, hipStream_t s) {
  small_attrs();
  small_dispatch(a.d, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT <= 8) {
      if (a.ms) {
        hipLaunchKernelGGL((small_finish_kernel<DT, true>), dim3(1), dim3(256), small_lds3(DT, true), s, a);
        return;
      }
    }
    hipLaunchKernelGGL((small_finish_kernel<DT, false>), dim3(1), dim3(256), small_lds3(DT), s, a);
  });
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
