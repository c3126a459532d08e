// Gradient of the log evidence with respect to the training inputs (Cov_se_iso, Cov_se_fat without multiscales).
//
// diag K_n = sf2 and K_m do not depend on the training inputs, so of a gradient entry -1/2 (v . diag K'_n - tr(W K'_m)) - tr(X^T K'_nm)
// only the last term is left.  With E = X .* K_nm and p_r the point the kernel sees
//   dl/dp_rk = inv_ell2 sum_c E_rc (p_rk - z_ck)
// -- the row-direction twin of the column sums sum_r E_rc (p_rk - z_ck) of grad_mfma.hip.  It is evaluated as
//   inv_ell2 ((p_rk - s_k) rowsum(E)_r - (E (Z - s))_rk)
// with a common offset s near the data (so that a far-away origin costs no digits), and the rows x m by m x d product runs as
// v_mfma_f64_16x16x4_f64 with E formed on the fly as the A operand:
//   * a wavefront owns 16 training points and walks the inducing columns 16 at a time, in order (no atomics; the bits of two
//     runs agree);
//   * K recomputed (d <= 64): S^T = (Z - s)(P - s)^T of the 16 x 16 tile is a first MFMA chain whose A rows are loaded in the
//     order 0 4 8 12 1 5 ..., so that the accumulator layout (lane: rows lq + 4 r of column l15) leaves lane (l15, lq) with
//     the four ADJACENT columns 4 lq + r of training point l15: |p - z|^2 = |p|^2 + |z|^2 - 2 S, exp_fast, times the 32
//     contiguous bytes of X the lane loaded -- which is exactly the A operand (k = lq) of the four output MFMAs against the
//     rows 4 lq + r of Z - s.  E never leaves the registers;
//   * K given (the resident store of Cov_se_fat with projection hypers, or the chunk rebuilt for d > 64): E = X .* K is
//     read the same way; more than 64 dimensions take one launch per block of 64;
//   * rowsum(E) is summed by the lanes beside the MFMAs (four adds per tile) and reduced over lq at the end.
// Workgroup: 4 wavefronts x 16 rows; the 64-column panels of Z - s are staged through LDS and shared by the four.
#include "kernels.h"
#include "exp_fast.h"

namespace gprhip {

namespace {

typedef double xd4 __attribute__((ext_vector_type(4)));
typedef double xd2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ xd4 xmfma4(double a, double b, xd4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

constexpr int XG_CP = 64;    // inducing columns per staged panel
constexpr int XG_ROWS = 64;  // training points per workgroup

struct InputGradBlock {
  InputGradArgs a;
  int d0, dw;  // the dimensions [d0, d0 + dw) of this launch
};

// KS4 = ceil(d / 4) k-steps of the distance product (0 with K given), DT = ceil(dw / 16) tiles of point dimensions
template <int KS4, int DT, bool KR>
__global__ __launch_bounds__(256) void input_grad_kernel(InputGradBlock g) {
  const InputGradArgs& a = g.a;
  constexpr int DP = DT * 16, LDP = DP + 4;
  __shared__ double zs[XG_CP * LDP];
  __shared__ double zn[XG_CP];
  __shared__ double sh[DP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  if (tid < DP) sh[tid] = tid < g.dw ? a.shift[g.d0 + tid] : 0.0;
  __syncthreads();
  const int row0 = blockIdx.x * XG_ROWS + wv * 16;
  const int prow = row0 + l15;  // the training point of this lane's elements of E
  const bool live_r = prow < a.rows;
  const int mc = (a.m + 15) & ~15;  // columns walked (<= mp)
  const ExpK ek = exp_consts();

  double pb[KS4 > 0 ? KS4 : 1], pn = 0.0;
  if constexpr (!KR) {
#pragma unroll
    for (int s = 0; s < KS4; ++s) {
      const int k = 4 * s + lq;
      const double v = (live_r && k < a.d) ? a.pts[(int64_t)prow * a.d + k] - sh[k] : 0.0;
      pb[s] = v;
      pn += v * v;
    }
    pn += __shfl_xor(pn, 16);
    pn += __shfl_xor(pn, 32);
  }
  xd4 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) acc[t] = (xd4){0, 0, 0, 0};
  double rs = 0.0;
  const int pcol = 4 * (l15 & 3) + (l15 >> 2);  // A rows of the distance product: 0 4 8 12 1 5 ...

  // columns cb + 4 lq .. + 3 of row prow: X (times K when it is given)
  auto load_e = [&](int cb, double (&o)[4]) {
    if (live_r && cb < mc) {
      const int64_t off = (int64_t)prow * a.mp + cb + 4 * lq;
      const xd2* q = reinterpret_cast<const xd2*>(a.X + off);
      const xd2 u = q[0], w = q[1];
      o[0] = u.x; o[1] = u.y; o[2] = w.x; o[3] = w.y;
      if constexpr (KR) {
        const xd2* qk = reinterpret_cast<const xd2*>(a.K + off);
        const xd2 uk = qk[0], wk = qk[1];
        o[0] *= uk.x; o[1] *= uk.y; o[2] *= wk.x; o[3] *= wk.y;
      }
    } else {
      o[0] = o[1] = o[2] = o[3] = 0.0;
    }
  };
  double xv[4], xn[4];
  load_e(0, xv);
  for (int c0 = 0; c0 < mc; c0 += XG_CP) {
    __syncthreads();
    for (int idx = tid; idx < XG_CP * DP; idx += 256) {
      const int c = idx / DP, k = idx % DP, col = c0 + c;
      zs[c * LDP + k] = (col < a.m && k < g.dw) ? a.Z[(int64_t)col * a.d + g.d0 + k] - sh[k] : 0.0;
    }
    __syncthreads();
    if constexpr (!KR) {
      const int c = tid >> 2, q = tid & 3;
      double s2 = 0.0;
      for (int k = q; k < DP; k += 4) s2 += zs[c * LDP + k] * zs[c * LDP + k];
      s2 += __shfl_xor(s2, 1);
      s2 += __shfl_xor(s2, 2);
      if (q == 0) zn[c] = s2;
      __syncthreads();
    }
#pragma unroll 1
    for (int j = 0; j < XG_CP / 16; ++j) {
      const int cb = c0 + 16 * j;
      if (cb >= mc) break;
      load_e(cb + 16, xn);  // (beyond the last column block: nothing)
      double ev[4];
      if constexpr (KR) {
#pragma unroll
        for (int r = 0; r < 4; ++r) ev[r] = (cb + 4 * lq + r < a.m) ? xv[r] : 0.0;
      } else {
        xd4 s4 = (xd4){0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < KS4; ++s) s4 = xmfma4(zs[(16 * j + pcol) * LDP + 4 * s + lq], pb[s], s4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 16 * j + 4 * lq + r;
          const double dist = fmax(pn + zn[c] - 2.0 * s4[r], 0.0);
          const double kv = exp_fast(a.log_sf2 + a.inv_ell2_05 * dist, ek);
          ev[r] = (live_r && c0 + c < a.m) ? xv[r] * kv : 0.0;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        rs += ev[r];
#pragma unroll
        for (int t = 0; t < DT; ++t) acc[t] = xmfma4(ev[r], zs[(16 * j + 4 * lq + r) * LDP + 16 * t + l15], acc[t]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = xn[r];
    }
  }
  rs += __shfl_xor(rs, 16);
  rs += __shfl_xor(rs, 32);  // every lane: rowsum(E) of training point l15
  const double inv_ell2 = -2.0 * a.inv_ell2_05;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = row0 + lq + 4 * r;
    const double rsum = __shfl(rs, lq + 4 * r);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int dim = 16 * t + l15;
      if (orow < a.rows && dim < g.dw) {
        const double pc = a.pts[(int64_t)orow * a.d + g.d0 + dim] - sh[dim];
        a.G[(int64_t)orow * a.ldg + g.d0 + dim] = inv_ell2 * (pc * rsum - acc[t][r]);
      }
    }
  }
}

template <int KS4, int DT, bool KR>
void launch_one(const InputGradBlock& g, hipStream_t s) {
  hipLaunchKernelGGL((input_grad_kernel<KS4, DT, KR>), dim3((g.a.rows + XG_ROWS - 1) / XG_ROWS), dim3(256), 0, s, g);
}

__global__ __launch_bounds__(256) void input_grad_project_kernel(const double* __restrict__ G, int64_t rows, int d, int D,
                                                                 const double* __restrict__ tproj, double* __restrict__ out,
                                                                 int64_t ldo) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * D) return;
  const int64_t r = idx / D;
  const int b = (int)(idx % D);
  double s = 0.0;
  for (int k = 0; k < d; ++k) s += tproj[(int64_t)k * D + b] * G[r * d + k];
  out[r * ldo + b] = s;
}

}  // namespace

void launch_input_grad(const InputGradArgs& a, hipStream_t s) {
  if (a.rows <= 0) return;
  InputGradBlock g{a, 0, a.d};
  if (a.d > 64 && !a.K) {
    set_error("gprhip: input gradient with more than 64 point dimensions needs K_nm of the chunk in memory");
    throw HipFail{ST_BAD_ARG};
  }
  if (a.K) {
    for (g.d0 = 0; g.d0 < a.d; g.d0 += 64) {
      g.dw = a.d - g.d0 < 64 ? a.d - g.d0 : 64;
      if (g.dw <= 16) launch_one<0, 1, true>(g, s);
      else if (g.dw <= 32) launch_one<0, 2, true>(g, s);
      else launch_one<0, 4, true>(g, s);
    }
  } else if (a.d <= 4) launch_one<1, 1, false>(g, s);
  else if (a.d <= 8) launch_one<2, 1, false>(g, s);
  else if (a.d <= 16) launch_one<4, 1, false>(g, s);
  else if (a.d <= 32) launch_one<8, 2, false>(g, s);
  else launch_one<16, 4, false>(g, s);
  GPR_HIP(hipGetLastError());
}

void launch_input_grad_project(const double* G, int64_t rows, int d, int D, const double* tproj, double* out, int64_t ldo,
                               hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(input_grad_project_kernel, dim3((unsigned)((rows * D + 255) / 256)), dim3(256), 0, s, G, rows, d, D, tproj,
                     out, ldo);
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
