// Several target vectors on one model (gprhip_eval_targets): the target-dependent pieces of an evaluation, each the
// k-column form of a single-vector step of the engine row path.  Everything expensive -- K_nm, V = K_nm U^-1, both
// factorisations, Q', the X launch, both SYRK-shaped launches, the gradient kernel -- depends on the model only and runs
// once; what is here is tall-skinny (n x m against m x k, k <= 16) and HBM-bound: one read of V, one of Q', one
// read-modify-write of X per gradient evaluation.
//   tg_vty_kernel   : C (m x k) = A^T diag(w) Y over the rows of A       (c~ = V^T diag(1/s) Y;  B = R~^-T c~)
//   tg_rows_kernel  : S (rows x k) = A Bm                                (Q' B per row chunk;  T~ = R~^-1 B;  T = U^-1 T~;
//                                                                         K_tm T of the prediction)
//   tg_p2_rows      : w_k = (y_k - (Q' b_k)) / s, v = v1 - mean_k w_k^2, es = q - v (sf2 - r) - mean_k w_k (Q' b_k)
//   tg_xcorr        : X -= (1/k) W_mat T^T                               (the ger of lib/fitc_gp.ml:1204-1206, rank k)
//   tg_w_rankk      : W~ -= (1/k) T~ T~^T                                (lib/fitc_gp.ml:1196-1203)
// Small m x k matrices are row-major with a fixed leading dimension of TG_LD = 16 (columns >= k are zero).  Every
// cross-workgroup sum goes through per-workgroup partials summed in workgroup order: results repeat bit for bit.
#include "kernels.h"

namespace gprhip {

namespace {

__device__ __forceinline__ double tg_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One wavefront per workgroup: 128 columns of A (two per lane, 16-byte loads) against a block of `rpb` rows; the row
// weights times the k target values of 64 rows at a time are staged in LDS and read back as broadcasts.
// part[row block][column][TG_LD].  UP: A is upper triangular (entries below the diagonal are not trusted to be zero).
template <int KT, bool UP>
__global__ __launch_bounds__(64) void tg_vty_kernel(const double* __restrict__ A, int64_t lda, int64_t rows, int rpb,
                                                    const double* __restrict__ w, const double* __restrict__ Y,
                                                    int64_t y_rs, int64_t y_cs, int k, int mp,
                                                    double* __restrict__ part) {
  __shared__ double sy[KT][64];
  const int lane = threadIdx.x;
  const int c = blockIdx.x * 128 + 2 * lane;
  const int64_t r0 = (int64_t)blockIdx.y * rpb;
  int64_t r1 = min(rows, r0 + (int64_t)rpb);
  if (UP) r1 = min(r1, (int64_t)blockIdx.x * 128 + 128);  // rows below this tile's last column contribute nothing
  double a0[KT], a1[KT];
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) a0[kk] = a1[kk] = 0.0;
  for (int64_t rb = r0; rb < r1; rb += 64) {
    __syncthreads();
    const int64_t r = rb + lane;
    const bool in = r < r1;
    const double wr = in ? (w ? w[r] : 1.0) : 0.0;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) sy[kk][lane] = (in && kk < k) ? wr * Y[r * y_rs + kk * y_cs] : 0.0;
    __syncthreads();
    const int nr = (int)min((int64_t)64, r1 - rb);
    const double* ap = A + rb * lda + c;
#pragma unroll 4
    for (int i = 0; i < nr; ++i) {
      double2 x = *reinterpret_cast<const double2*>(ap + (int64_t)i * lda);
      if (UP) {
        if (rb + i > c) x.x = 0.0;
        if (rb + i > c + 1) x.y = 0.0;
      }
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) {
        const double sv = sy[kk][i];
        a0[kk] = fma(sv, x.x, a0[kk]);
        a1[kk] = fma(sv, x.y, a1[kk]);
      }
    }
  }
  double* o = part + ((int64_t)blockIdx.y * mp + c) * TG_LD;
#pragma unroll
  for (int kk = 0; kk < TG_LD; ++kk) {
    o[kk] = kk < KT ? a0[kk < KT ? kk : 0] : 0.0;
    o[TG_LD + kk] = kk < KT ? a1[kk < KT ? kk : 0] : 0.0;
  }
}

// 64 rows of A per workgroup; 64 x 64 tiles of A go through LDS (read coalesced along the rows, used one row per lane),
// the matching 64 x k tile of Bm beside them.  The four wavefronts take 16 columns of the tile each and are combined in a
// fixed order at the end.  out[row * o_rs + kk * o_cs], kk < k.
template <int KT, bool UP>
__global__ __launch_bounds__(256) void tg_rows_kernel(const double* __restrict__ A, int64_t lda, int64_t rows, int mp,
                                                      const double* __restrict__ Bm, int k, double* __restrict__ out,
                                                      int64_t o_rs, int64_t o_cs) {
  __shared__ double smem[64 * 65 + 64 * KT];
  double(*sA)[65] = reinterpret_cast<double(*)[65]>(smem);
  double(*sB)[KT] = reinterpret_cast<double(*)[KT]>(smem + 64 * 65);
  double(*sR)[KT][64] = reinterpret_cast<double(*)[KT][64]>(smem);  // (the A tile's space, after the last tile is done with)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  double acc[KT];
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) acc[kk] = 0.0;
  const int col2 = (t & 31) * 2, lrow = t >> 5;
  for (int j0 = UP ? (int)r0 : 0; j0 < mp; j0 += 64) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = lrow + 8 * q;
      const int64_t gr = r0 + row;
      double2 x = make_double2(0.0, 0.0);
      if (gr < rows) x = *reinterpret_cast<const double2*>(A + gr * lda + j0 + col2);
      if (UP) {
        if (j0 + col2 < gr) x.x = 0.0;
        if (j0 + col2 + 1 < gr) x.y = 0.0;
      }
      sA[row][col2] = x.x;
      sA[row][col2 + 1] = x.y;
    }
    for (int idx = t; idx < 64 * KT; idx += 256) {
      const int j = idx / KT, kk = idx % KT;
      sB[j][kk] = Bm[(int64_t)(j0 + j) * TG_LD + kk];
    }
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const double a = sA[lane][wv * 16 + jj];
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) acc[kk] = fma(a, sB[wv * 16 + jj][kk], acc[kk]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) sR[wv][kk][lane] = acc[kk];
  __syncthreads();
  for (int idx = t; idx < 64 * KT; idx += 256) {
    const int kk = idx / 64, row = idx % 64;
    if (r0 + row < rows && kk < k)
      out[(r0 + row) * o_rs + kk * o_cs] = (sR[0][kk][row] + sR[1][kk][row]) + (sR[2][kk][row] + sR[3][kk][row]);
  }
}

// part[block][TG_LD]: sum over the block's 256 rows of y_k^2 / s   (|y~_k|^2 of lib/fitc_gp.ml:290)
template <int KT>
__global__ __launch_bounds__(256) void tg_y2_kernel(const double* __restrict__ Y, int64_t ld, const double* __restrict__ is,
                                                    int64_t rows, int k, double* __restrict__ part) {
  __shared__ double red[4][KT];
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double wr = row < rows ? is[row] : 0.0;
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) {
    const double y = (row < rows && kk < k) ? Y[kk * ld + row] : 0.0;
    const double v = tg_wave_sum(wr * y * y);
    if (lane == 0) red[wv][kk] = v;
  }
  __syncthreads();
  if (threadIdx.x < TG_LD) {
    const int kk = threadIdx.x;
    part[(int64_t)blockIdx.x * TG_LD + kk] = kk < KT ? (red[0][kk < KT ? kk : 0] + red[1][kk < KT ? kk : 0]) +
                                                           (red[2][kk < KT ? kk : 0] + red[3][kk < KT ? kk : 0])
                                                     : 0.0;
  }
}

// out[kk] = sum_i Bm[i][kk]^2 (one workgroup; 16 row classes per column, combined in order)
__global__ __launch_bounds__(256) void tg_colsq_kernel(const double* __restrict__ Bm, int mp, double* __restrict__ out) {
  __shared__ double red[16][TG_LD];
  const int kk = threadIdx.x % TG_LD, cls = threadIdx.x / TG_LD;
  double acc = 0.0;
  for (int i = cls; i < mp; i += 16) {
    const double b = Bm[(int64_t)i * TG_LD + kk];
    acc = fma(b, b, acc);
  }
  red[cls][kk] = acc;
  __syncthreads();
  if (threadIdx.x < TG_LD) {
    double tot = 0.0;
    for (int c = 0; c < 16; ++c) tot += red[c][threadIdx.x];
    out[threadIdx.x] = tot;
  }
}

// One training point per thread.  On entry Wm[kk][row] = (Q' b_k)_row, v = v1 and es = q - v1 (sf2 - r) as the model-only
// row pass left them; on exit Wm = w_k, v = v1 - mean_k w_k^2 and es = q - v (sf2 - r) - mean_k w_k (Q' b_k) with that v
// (rowops.hip, pass2_rows_kernel: the row sum of E carries the FINAL v).  part[block] = -sum mean_k w_k^2.
template <int KT>
__global__ __launch_bounds__(256) void tg_p2_rows_kernel(const double* __restrict__ Y, double* __restrict__ Wm, int64_t ld,
                                                         const double* __restrict__ is, const double* __restrict__ r,
                                                         double sf2, int rows, int k, double inv_k,
                                                         double* __restrict__ v, double* __restrict__ es,
                                                         double* __restrict__ part) {
  __shared__ double red[4];
  const int row = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double dv = 0.0;
  if (row < rows) {
    const double isr = is[row];
    double sw2 = 0.0, swsb = 0.0;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
      if (kk < k) {
        const double sb = Wm[kk * ld + row];
        const double w = isr * (Y[kk * ld + row] - sb);
        Wm[kk * ld + row] = w;
        sw2 = fma(w, w, sw2);
        swsb = fma(w, sb, swsb);
      }
    }
    dv = -(sw2 * inv_k);
    v[row] += dv;
    if (es) es[row] -= dv * (sf2 - r[row]) + swsb * inv_k;
  }
  dv = tg_wave_sum(dv);
  if (lane == 0) red[wv] = dv;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// X[row][c] -= inv_k sum_kk Wm[kk][row] T[c][kk]: a thread keeps the k coefficients of its two columns in registers and
// walks 32 rows
template <int KT>
__global__ __launch_bounds__(128) void tg_xcorr_kernel(double* __restrict__ X, int rows, int mp, const double* __restrict__ Wm,
                                                       int64_t ld, const double* __restrict__ T, int k, double inv_k) {
  const int c = blockIdx.x * 256 + 2 * threadIdx.x;
  if (c >= mp) return;
  double t0[KT], t1[KT];
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) {
    t0[kk] = kk < k ? inv_k * T[(int64_t)c * TG_LD + kk] : 0.0;
    t1[kk] = kk < k ? inv_k * T[(int64_t)(c + 1) * TG_LD + kk] : 0.0;
  }
  const int r0 = blockIdx.y * 32, r1 = min(rows, r0 + 32);
  for (int r = r0; r < r1; ++r) {
    double2* xp = reinterpret_cast<double2*>(X + (int64_t)r * mp + c);
    double2 x = *xp;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
      const double w = kk < k ? Wm[kk * ld + r] : 0.0;
      x.x = fma(-w, t0[kk], x.x);
      x.y = fma(-w, t1[kk], x.y);
    }
    *xp = x;
  }
}

// W~[r][c] -= inv_k sum_kk Tt[r][kk] Tt[c][kk]   (W~ full symmetric, as build_w leaves it)
__global__ __launch_bounds__(256) void tg_w_rankk_kernel(double* __restrict__ W, int mp, const double* __restrict__ Tt,
                                                         int k, double inv_k) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (c >= mp) return;
  double acc = 0.0;
  for (int kk = 0; kk < k; ++kk) acc = fma(Tt[(int64_t)r * TG_LD + kk], Tt[(int64_t)c * TG_LD + kk], acc);
  W[(int64_t)r * mp + c] -= inv_k * acc;
}

int tg_kt(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

}  // namespace

#define TG_DISPATCH(k, ...)                  \
  switch (tg_kt(k)) {                        \
    case 1: { constexpr int KT = 1; __VA_ARGS__; } break;  \
    case 2: { constexpr int KT = 2; __VA_ARGS__; } break;  \
    case 4: { constexpr int KT = 4; __VA_ARGS__; } break;  \
    case 8: { constexpr int KT = 8; __VA_ARGS__; } break;  \
    default: { constexpr int KT = 16; __VA_ARGS__; } break; \
  }

int targets_vty_rows_per_block(int64_t rows) {
  return (int)std::max<int64_t>(64, round_up((rows + 255) / 256, 64));
}
int targets_vty_blocks(int64_t rows) {
  const int rpb = targets_vty_rows_per_block(rows);
  return (int)((rows + rpb - 1) / rpb);
}

void launch_targets_vty(const double* A, int64_t lda, int64_t rows, int mp, int upper, const double* w, const double* Y,
                        int64_t y_rs, int64_t y_cs, int k, double* part, double* out, hipStream_t s) {
  const int rpb = targets_vty_rows_per_block(rows), nblk = targets_vty_blocks(rows);
  const dim3 grid(mp / TILE, nblk);
  if (upper) {
    TG_DISPATCH(k, hipLaunchKernelGGL((tg_vty_kernel<KT, true>), grid, dim3(64), 0, s, A, lda, rows, rpb, w, Y, y_rs, y_cs,
                                       k, mp, part));
  } else {
    TG_DISPATCH(k, hipLaunchKernelGGL((tg_vty_kernel<KT, false>), grid, dim3(64), 0, s, A, lda, rows, rpb, w, Y, y_rs, y_cs,
                                       k, mp, part));
  }
  GPR_HIP(hipGetLastError());
  launch_reduce_rows(part, nblk, mp * TG_LD, out, 0, s);
}

void launch_targets_rows(const double* A, int64_t lda, int64_t rows, int mp, int upper, const double* Bm, int k,
                         double* out, int64_t o_rs, int64_t o_cs, hipStream_t s) {
  const dim3 grid((unsigned)((rows + 63) / 64));
  if (upper) {
    TG_DISPATCH(k, hipLaunchKernelGGL((tg_rows_kernel<KT, true>), grid, dim3(256), 0, s, A, lda, rows, mp, Bm, k, out, o_rs,
                                       o_cs));
  } else {
    TG_DISPATCH(k, hipLaunchKernelGGL((tg_rows_kernel<KT, false>), grid, dim3(256), 0, s, A, lda, rows, mp, Bm, k, out, o_rs,
                                       o_cs));
  }
  GPR_HIP(hipGetLastError());
}

void launch_targets_y2(const double* Y, int64_t ld, const double* is, int64_t rows, int k, double* part, double* out,
                       hipStream_t s) {
  const int nblk = (int)((rows + 255) / 256);
  TG_DISPATCH(k, hipLaunchKernelGGL((tg_y2_kernel<KT>), dim3(nblk), dim3(256), 0, s, Y, ld, is, rows, k, part));
  GPR_HIP(hipGetLastError());
  launch_reduce_rows(part, nblk, TG_LD, out, 0, s);
}

void launch_targets_colsq(const double* Bm, int mp, double* out, hipStream_t s) {
  hipLaunchKernelGGL(tg_colsq_kernel, dim3(1), dim3(256), 0, s, Bm, mp, out);
  GPR_HIP(hipGetLastError());
}

void launch_targets_p2_rows(const double* Y, double* Wm, int64_t ld, const double* is, const double* r, double sf2, int rows,
                            int k, double* v, double* es, double* part, double* sumv, hipStream_t s) {
  const int nblk = (rows + 255) / 256;
  const double inv_k = 1.0 / k;
  TG_DISPATCH(k, hipLaunchKernelGGL((tg_p2_rows_kernel<KT>), dim3(nblk), dim3(256), 0, s, Y, Wm, ld, is, r, sf2, rows, k, inv_k, v,
                                     es, part));
  GPR_HIP(hipGetLastError());
  launch_reduce_rows(part, nblk, 1, sumv, 1, s);
}

void launch_targets_xcorr(double* X, int rows, int mp, const double* Wm, int64_t ld, const double* T, int k, hipStream_t s) {
  const dim3 grid((mp + 255) / 256, (rows + 31) / 32);
  const double inv_k = 1.0 / k;
  TG_DISPATCH(k, hipLaunchKernelGGL((tg_xcorr_kernel<KT>), grid, dim3(128), 0, s, X, rows, mp, Wm, ld, T, k, inv_k));
  GPR_HIP(hipGetLastError());
}

void launch_targets_w_rankk(double* W, int mp, const double* Tt, int k, hipStream_t s) {
  hipLaunchKernelGGL(tg_w_rankk_kernel, dim3((mp + 255) / 256, mp), dim3(256), 0, s, W, mp, Tt, k, 1.0 / k);
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
