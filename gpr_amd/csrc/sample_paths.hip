// Posterior sample paths over test points (gprhip_sample_paths; Cov_se_iso, Cov_se_fat without multiscales).
//
// The FITC posterior is a Gaussian over m weights: with z ~ N(0, I_m) a draw is the function
//   f(x) = sum_c k(x, z_c) a_c,   a = t + U^-1 (R~^-1 z)      (R = R~ U: Cov a = R^-1 R^-T = B^-1, mean a = t)
// and a sample at test point r adds the independent part  sqrt(max(0, sf2 - |K_r U^-1|^2 (+ sigma2))) eps_r.
//   * sp_weights_kernel: an upper-triangular m x m factor times an m x ns matrix, twice (R~^-1 Z first, then U^-1 times that,
//     plus t): the weights A, [mp][64] with padded rows and columns zero.  One wavefront per row, the k range split over the
//     lanes; one launch of one workgroup for one tile and at most 4 draws (the second product behind a barrier), else one per product.
//   * sample_paths_kernel (any m, d <= 64): the wavefront layout of predict_grad_kernel -- 16 test points per wavefront, the
//     columns walked in order, Z - s panels in LDS, the distance product as a first MFMA chain whose A rows are permuted so
//     that a lane ends with four adjacent columns, one exp per (row, column) -- and the K tile as the B operand of
//     v_mfma_f64_16x16x4 against panels of A^T staged in LDS: NB = ceil(ns / 16) accumulator tiles hold F^T, draws down the
//     registers and the 16 test points across the lanes, so F[j][r] is stored draw-major in runs of 16 points.  K is never
//     written to memory.  RESID: the same product against the m columns of U^-1 (m <= 64) with the row sums of squares |K_r U^-1|^2 as the
//     only output -- the residual variance of few inducing points without a chunk x mp matrix.
//   * sp_combine_kernel: samples = F + sqrt(max(0, (sf2 - |K_r U^-1|^2) + add)) eps, in place.
//   * path_grad_at_kernel: the gradient of draw j at its best k points, one wavefront per (draw, winner), direct differences
//     against Z - s, then times tproj where there is a projection.
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

constexpr int SP_ROWS = 64;  // test points per workgroup
constexpr int SP_LD = SP_MAX_DRAWS;

// Row i of  out = (add ? add 1^T : 0) + T B  by one wavefront: out[i][j] = sum_{k >= i} T[i][k] B[k][j] for j < ns, zero for
// ns <= j < 64 and for rows >= m.  The lanes are cw columns (cw = the power of two that holds min(ns, 16)) times 64 / cw
// interleaved parts of the k range, summed over the parts by shuffles in a fixed order: the dependent chain of a row is
// (m - i) cw / 64 long.
__device__ __forceinline__ void sp_tri_row(const double* __restrict__ T, const double* B, const double* __restrict__ add, int i,
                                           int m, int mp, int ns, int cw, double* out, int lane) {
  double* const orow = out + (int64_t)i * SP_LD;
  if (i >= m) {
    orow[lane] = 0.0;
    return;
  }
  const int jj = lane & (cw - 1), kq = lane / cw, kg = 64 / cw;
  const double* const trow = T + (int64_t)i * mp;
  for (int j0 = 0; j0 < ns; j0 += cw) {
    const int j = j0 + jj;
    double acc = 0.0;
    if (j < ns) {
#pragma unroll 4
      for (int k = i + kq; k < m; k += kg) acc = __builtin_fma(trow[k], B[(int64_t)k * SP_LD + j], acc);
    }
    for (int off = cw; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
    if (kq == 0 && j < ns) orow[j] = add ? acc + add[i] : acc;
  }
  if (lane >= ns) orow[lane] = 0.0;
}

// phase 1: w1 = Rinv Z; phase 2: out = t 1^T + Uinv w1 (both factors upper-triangular, row-major mp x mp); phases = 3: both
// in ONE workgroup (gridDim.x == 1), the second after a barrier -- the workgroup's own stores to w1 are visible to it then
__global__ __launch_bounds__(1024) void sp_weights_kernel(const double* __restrict__ Rinv, const double* __restrict__ Uinv,
                                                           const double* __restrict__ Zh, const double* __restrict__ tvec,
                                                           int m, int mp, int ns, int cw, int phases, double* w1, double* out) {
  const int lane = threadIdx.x & 63, wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * (blockDim.x >> 6);
  if (phases & 1)
    for (int i = wave; i < mp; i += nwaves) sp_tri_row(Rinv, Zh, nullptr, i, m, mp, ns, cw, w1, lane);
  if (phases == 3) __syncthreads();
  if (phases & 2)
    for (int i = wave; i < mp; i += nwaves) sp_tri_row(Uinv, w1, tvec, i, m, mp, ns, cw, out, lane);
}

// KS4 = ceil(d / 4) k-steps of the distance product, DT = ceil(d / 16) tiles of point dimensions, NB = ceil(ns / 16)
template <int KS4, int DT, int NB, bool RESID>
__global__ __launch_bounds__(256) void sample_paths_kernel(SamplePathArgs a) {
  constexpr int DP = DT * 16, LDP = DP + 4, NW = NB * 16, LDA = NW + 4;
  constexpr int CP = (DP + NW > 96) ? 32 : 64;  // inducing columns per staged panel (the two panels stay below 64 KB)
  __shared__ double zs[CP * LDP];
  __shared__ double ap[CP * LDA];
  __shared__ double zn[CP];
  __shared__ double sh[DP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  if (tid < DP) sh[tid] = tid < a.d ? a.shift[tid] : 0.0;
  __syncthreads();
  const int row0 = blockIdx.x * SP_ROWS + wv * 16;
  const int prow = row0 + l15;  // the test point of this lane's elements of K and of F^T
  const bool live_r = prow < a.rows;
  const int mc = (a.m + 15) & ~15;  // columns walked
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
  pd4 acc[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) acc[t] = (pd4){0, 0, 0, 0};
  const int pcol = 4 * (l15 & 3) + (l15 >> 2);  // A rows of the distance product: 0 4 8 12 1 5 ...

  for (int c0 = 0; c0 < mc; c0 += CP) {
    __syncthreads();
    for (int idx = tid; idx < CP * DP; idx += 256) {
      const int c = idx / DP, k = idx % DP, col = c0 + c;
      zs[c * LDP + k] = (col < a.m && k < a.d) ? a.Z[(int64_t)col * a.d + k] - sh[k] : 0.0;
    }
    for (int idx = tid; idx < CP * NW; idx += 256) {
      const int c = idx / NW, j = idx % NW, col = c0 + c;
      ap[c * LDA + j] = (col < a.m && j < a.ns) ? a.W[(int64_t)col * a.ldw + j] : 0.0;
    }
    __syncthreads();
    {
      const int c = tid >> 2, q = tid & 3;  // (c < CP: whole wavefronts)
      if (c < CP) {
        double s2 = 0.0;
        for (int k = q; k < DP; k += 4) s2 += zs[c * LDP + k] * zs[c * LDP + k];
        s2 += __shfl_xor(s2, 1);
        s2 += __shfl_xor(s2, 2);
        if (q == 0) zn[c] = s2;
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int j = 0; j < CP / 16; ++j) {
      const int cb = c0 + 16 * j;
      if (cb >= mc) break;
      pd4 s4 = (pd4){0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < KS4; ++s) s4 = pmfma4(zs[(16 * j + pcol) * LDP + 4 * s + lq], pb[s], s4);
      double kv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * j + 4 * lq + r;
        const double dist = fmax(pn + zn[c] - 2.0 * s4[r], 0.0);
        kv[r] = (live_r && c0 + c < a.m) ? exp_fast(a.log_sf2 + a.inv_ell2_05 * dist, ek) : 0.0;
      }
      // F^T += A^T K^T: the lane's K entry (point l15, column 4 lq + r) is B[k = lq][col = l15] of k-step r
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < NB; ++t) acc[t] = pmfma4(ap[(16 * j + 4 * lq + r) * LDA + 16 * t + l15], kv[r], acc[t]);
    }
  }
  if constexpr (RESID) {
    double q = 0.0;
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) q += acc[t][r] * acc[t][r];
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    if (lq == 0 && live_r) a.sumsq[prow] = q;
  } else {
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int draw = 16 * t + lq + 4 * r;
        if (live_r && draw < a.ns) a.F[(int64_t)draw * a.ldf + prow] = acc[t][r];
      }
  }
}

template <int KS4, int DT, bool RESID>
void launch_width(const SamplePathArgs& a, hipStream_t s) {
  const dim3 grid((a.rows + SP_ROWS - 1) / SP_ROWS);
  const int nb = (a.ns + 15) / 16;
  if (nb == 1) hipLaunchKernelGGL((sample_paths_kernel<KS4, DT, 1, RESID>), grid, dim3(256), 0, s, a);
  else if (nb == 2) hipLaunchKernelGGL((sample_paths_kernel<KS4, DT, 2, RESID>), grid, dim3(256), 0, s, a);
  else if (nb == 3) hipLaunchKernelGGL((sample_paths_kernel<KS4, DT, 3, RESID>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((sample_paths_kernel<KS4, DT, 4, RESID>), grid, dim3(256), 0, s, a);
}

// samples[j][r] = F[j][r] + sqrt(max(0, (sf2 - sumsq[r]) + add)) eps[j][r], in place of F
__global__ __launch_bounds__(256) void sp_combine_kernel(double* __restrict__ F, int64_t ldf, const double* __restrict__ eps,
                                                          int64_t lde, const double* __restrict__ sumsq, double sf2, double add,
                                                          int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (r >= rows) return;
  const double sd = sqrt(fmax((sf2 - sumsq[r]) + add, 0.0));
  F[(int64_t)j * ldf + r] = F[(int64_t)j * ldf + r] + sd * eps[(int64_t)j * lde + r];
}

// one wavefront per (winner w = blockIdx.x, draw j = blockIdx.y); the block of draw j: [k] indices (as doubles) | [k] values |
// [k][D] gradients (written here; zero where the index is -1)
__global__ __launch_bounds__(64) void path_grad_at_kernel(PathGradAtArgs a) {
  __shared__ double ps[64], ws[64], gs[64];
  const int lane = threadIdx.x, w = blockIdx.x, j = blockIdx.y;
  double* const blk = a.out + (int64_t)j * a.out_stride;
  double* const g = blk + 2 * a.k + (int64_t)w * a.D;
  const int idx = (int)blk[w];
  if (idx < 0 || idx >= a.rows) {
    for (int b = lane; b < a.D; b += 64) g[b] = 0.0;
    return;
  }
  const ExpK ek = exp_consts();
  const double sk = lane < a.d ? a.shift[lane] : 0.0;
  ps[lane] = lane < a.d ? a.pts[(int64_t)idx * a.d + lane] - sk : 0.0;
  gs[lane] = sk;
  __syncthreads();
  double acc = 0.0;
  for (int c0 = 0; c0 < a.m; c0 += 64) {
    const int c = c0 + lane;
    double wv = 0.0;
    if (c < a.m) {
      double dist = 0.0;
      for (int k = 0; k < a.d; ++k) {
        const double diff = ps[k] - (a.Z[(int64_t)c * a.d + k] - gs[k]);
        dist += diff * diff;
      }
      wv = exp_fast(a.log_sf2 + a.inv_ell2_05 * dist, ek) * a.W[(int64_t)c * SP_LD + j];
    }
    __syncthreads();  // the reads of ws of the block before
    ws[lane] = wv;
    __syncthreads();
    if (lane < a.d) {
      const int ce = a.m - c0 < 64 ? a.m - c0 : 64;
      for (int cc = 0; cc < ce; ++cc) acc += ws[cc] * (ps[lane] - (a.Z[(int64_t)(c0 + cc) * a.d + lane] - sk));
    }
  }
  acc *= 2.0 * a.inv_ell2_05;  // -inv_ell2
  if (!a.tproj) {
    if (lane < a.d) g[lane] = acc;
    return;
  }
  __syncthreads();
  ps[lane] = lane < a.d ? acc : 0.0;
  __syncthreads();
  for (int b = lane; b < a.D; b += 64) {
    double o = 0.0;
    for (int k = 0; k < a.d; ++k) o += a.tproj[(int64_t)k * a.D + b] * ps[k];
    g[b] = o;
  }
}

template <bool RESID>
void launch_any(const SamplePathArgs& a, hipStream_t s) {
  if (a.d <= 4) launch_width<1, 1, RESID>(a, s);
  else if (a.d <= 8) launch_width<2, 1, RESID>(a, s);
  else if (a.d <= 16) launch_width<4, 1, RESID>(a, s);
  else if constexpr (!RESID) {  // (the one-kernel residual serves at most 16 dimensions)
    if (a.d <= 32) launch_width<8, 2, RESID>(a, s);
    else launch_width<16, 4, RESID>(a, s);
  }
  GPR_HIP(hipGetLastError());
}

}  // namespace

void launch_sp_weights(const double* Rinv, const double* Uinv, const double* Zh, const double* tvec, int m, int mp, int ns,
                       double* w1, double* out, hipStream_t s) {
  int cw = 1;
  while (cw < ns && cw < 16) cw <<= 1;
  // one tile of inducing points and at most 4 draws: one workgroup, one launch -- the second product waits at a barrier (a
  // wavefront walks its rows one after the other, each a few load latencies long: beyond this the rows are better spread
  // over the chip, one wavefront each, at the price of the second launch)
  if (mp <= 128 && ns <= 4) {
    hipLaunchKernelGGL(sp_weights_kernel, dim3(1), dim3(1024), 0, s, Rinv, Uinv, Zh, tvec, m, mp, ns, cw, 3, w1, out);
  } else {
    const dim3 grid((mp + 3) / 4);
    hipLaunchKernelGGL(sp_weights_kernel, grid, dim3(256), 0, s, Rinv, Uinv, Zh, tvec, m, mp, ns, cw, 1, w1, out);
    hipLaunchKernelGGL(sp_weights_kernel, grid, dim3(256), 0, s, Rinv, Uinv, Zh, tvec, m, mp, ns, cw, 2, w1, out);
  }
  GPR_HIP(hipGetLastError());
}

void launch_sample_paths(const SamplePathArgs& a, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.d > 64 || a.ns < 1 || a.ns > SP_MAX_DRAWS || !a.F) {
    set_error("gprhip: the sample paths take 1 .. 64 draws of at most 64 point dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  launch_any<false>(a, s);
}

void launch_sp_row_sumsq(const SamplePathArgs& a, hipStream_t s) {
  if (a.rows <= 0) return;
  if (a.d > 16 || a.m > 64 || a.ns != a.m || !a.sumsq) {
    set_error("gprhip: the one-kernel residual takes at most 64 inducing points of at most 16 dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  launch_any<true>(a, s);
}

void launch_sp_combine(double* F, int64_t ldf, const double* eps, int64_t lde, const double* sumsq, double sf2, double add,
                       int rows, int ns, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(sp_combine_kernel, dim3((rows + 255) / 256, ns), dim3(256), 0, s, F, ldf, eps, lde, sumsq, sf2, add, rows);
  GPR_HIP(hipGetLastError());
}

void launch_path_grad_at(const PathGradAtArgs& a, hipStream_t s) {
  if (a.k < 1 || a.ns < 1) return;
  if (a.d > 64) {
    set_error("gprhip: the gradient of a sample path takes at most 64 point dimensions");
    throw HipFail{ST_BAD_ARG};
  }
  hipLaunchKernelGGL(path_grad_at_kernel, dim3(a.k, a.ns), dim3(64), 0, s, a);
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
