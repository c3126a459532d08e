// gprhip_observe: fold k <= 64 new observations into the whitened posterior factors without a refit.
//   rows    W = diag(1/sqrt(s)) V_new ([64][mp]) and eta = y / sqrt(s) from the rows of V = K U^-1 that the prediction launches built
//   update  [R~' | b'] = the triangular factor of [R~ | b] stacked on [W | eta]: a triangular-pentagonal QR in 128-column
//           blocks, ONE reflector per pivot column (tp_reflect.h).  Per block row two launches in stream order: the
//           diagonal launch (one workgroup: block of R~ in LDS, W in registers with the k entries of a column across the 64
//           lanes of a wavefront, dot products by cross-lane butterflies) and the trailing launch (one lane per column right of
//           the block and one for b | eta: its k entries of W in registers, R~ streamed row by row, the reflectors in LDS).
// No atomics; every sum has a fixed order.
#include "kernels.h"
#include "tp_reflect.h"

namespace gprhip {

namespace {

constexpr int OB = TILE;       // block of pivot columns
constexpr int OK_ROWS = OBS_MAX_ROWS;
constexpr int DIAG_THREADS = 1024, DIAG_WAVES = DIAG_THREADS / 64, DIAG_SLOTS = OB / DIAG_WAVES;  // 16 wavefronts, 8 columns each
// LDS of the diagonal launch: the block of R~ | w of the reflector in flight (two buffers) | its (v1, beta) | the block of b |
// the reduction scratch
// (138 KB: the 160 KB of LDS a gfx950 workgroup may take, as chol.hip's diagonal kernels do -- the library is built for that
//  target alone; the launch fails with a HIP error on a device with less)
constexpr int DIAG_LDS = (OB * OB + 2 * 64 + 2 * 2 + OB + DIAG_THREADS) * 8;

__device__ __forceinline__ double wave_sum(double x) {
  // butterfly: lane l and lane l ^ o add the same two numbers, so all 64 lanes end with the same bits
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// r_i = sf2 - |v_i|^2, s_i = r_i + sigma2, W[i][:] = v_i / sqrt(s_i), eta_i = y_i / sqrt(s_i); rows >= k are zero.  One
// workgroup per row of the [64][mp] block.  A row with s_i <= 0 gets zeros: the caller refuses the call from rs.
__global__ __launch_bounds__(256) void obs_rows_kernel(ObsRowsArgs a) {
  const int i = blockIdx.x;
  double inv = 0.0;
  if (i < a.k) {
    const double r = a.sf2 - a.sumsq[i];
    const double s = r + a.sigma2;
    inv = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
    if (threadIdx.x == 0) {
      a.rs[i] = r;
      a.rs[OK_ROWS + i] = s;
    }
  } else if (threadIdx.x == 0) {
    a.rs[i] = 0.0;
    a.rs[OK_ROWS + i] = 0.0;
  }
  for (int c = threadIdx.x; c < a.mp; c += 256)
    a.W[(int64_t)i * a.mp + c] = (i < a.k && c < a.m) ? a.V[(int64_t)i * a.mp + c] * inv : 0.0;
  if (threadIdx.x == 0) a.eta[i] = (i < a.k && a.y) ? a.y[i] * inv : 0.0;
}

// The diagonal launch of block row J.  rhs: this launch carries the b | eta column (the last block row of a state with targets).
__global__ __launch_bounds__(DIAG_THREADS) void obs_diag_kernel(ObsUpdateArgs a, int J, int rhs, int last) {
  extern __shared__ __attribute__((aligned(16))) double L[];
  double* const Rl = L;                    // [128][128]
  double* const sw = Rl + OB * OB;         // [2][64]
  double* const ss = sw + 2 * 64;          // [2][2]
  double* const sb = ss + 4;               // [128]
  double* const red = sb + OB;             // [1024]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int mp = a.mp;
  const int64_t o0 = (int64_t)J * OB;
  for (int idx = tid; idx < OB * OB; idx += DIAG_THREADS)  // (the upper triangle alone is read again)
    if (idx % OB >= idx / OB) Rl[idx] = a.R[(o0 + idx / OB) * mp + o0 + idx % OB];
  if (rhs && tid < OB) sb[tid] = a.b[o0 + tid];
  double W[DIAG_SLOTS];
#pragma unroll
  for (int t = 0; t < DIAG_SLOTS; ++t) W[t] = a.W[(int64_t)lane * mp + o0 + w + DIAG_WAVES * t];
  double e = (rhs && w == 0) ? a.eta[lane] : 0.0;
  __syncthreads();

  // the wavefront that owns pivot column jn forms its reflector, publishes it in LDS buffer jn & 1 and in global memory
  auto reflector = [&](int jn) {
    double x = 0.0;
#pragma unroll
    for (int t = 0; t < DIAG_SLOTS; ++t)
      if (t == jn / DIAG_WAVES) x = W[t];
    const double sigma = wave_sum(x * x);
    double mu, v1, beta;
    const double lr = tp_reflector(Rl[jn * OB + jn], sigma, mu, v1, beta);
    sw[(jn & 1) * 64 + lane] = x;
    if (!last) a.u[jn * 64 + lane] = x;  // (the trailing launch reads them; the last block row has none)
    if (lane == 0) {
      Rl[jn * OB + jn] = mu;
      ss[(jn & 1) * 2] = v1;
      ss[(jn & 1) * 2 + 1] = beta;
      if (!last) {
        a.vb[jn] = v1;
        a.vb[OB + jn] = beta;
      }
      a.ldr[o0 + jn] = lr;
    }
  };
  if (w == 0) reflector(0);
  __syncthreads();
  for (int j = 0; j < OB; ++j) {
    const int buf = j & 1;
    const double v1 = ss[buf * 2], beta = ss[buf * 2 + 1];
    if (beta != 0.0) {
      const double wl = sw[buf * 64 + lane];
#pragma unroll
      for (int t = 0; t < DIAG_SLOTS; ++t) {
        const int c = w + DIAG_WAVES * t;
        if (c > j) {
          const double rho = Rl[j * OB + c];
          const double tt = tp_factor(v1, beta, rho, wave_sum(wl * W[t]));
          W[t] -= tt * wl;
          if (lane == 0) Rl[j * OB + c] = rho - tt * v1;
        }
      }
      if (rhs && w == 0) {
        const double rho = sb[j];
        const double tt = tp_factor(v1, beta, rho, wave_sum(wl * e));
        e -= tt * wl;
        if (lane == 0) sb[j] = rho - tt * v1;
      }
    }
    if (j + 1 < OB && w == ((j + 1) & (DIAG_WAVES - 1))) reflector(j + 1);
    __syncthreads();
  }
  for (int idx = tid; idx < OB * OB; idx += DIAG_THREADS) {
    const int r = idx / OB, c = idx % OB;
    if (c >= r) a.R[(o0 + r) * mp + o0 + c] = Rl[idx];
  }
  if (rhs && tid < OB) a.b[o0 + tid] = sb[tid];
  if (!last) return;
  // the last launch: sum_j log(R~'_jj / R~_jj) over all columns and |rho|^2 (what is left of eta), each in a fixed order
  if (rhs && w == 0) {
    a.eta[lane] = e;
    const double r2 = wave_sum(e * e);
    if (lane == 0) a.out[1] = r2;
  } else if (!rhs && tid == 0) {
    a.out[1] = 0.0;
  }
  __syncthreads();  // (the ldr entries of this launch are visible to the whole workgroup)
  double s = 0.0;
  for (int c = tid; c < mp; c += DIAG_THREADS) s += a.ldr[c];
  red[tid] = s;
  __syncthreads();
  for (int o = DIAG_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) a.out[0] = red[0];
}

// The trailing launch of block row J: the 128 reflectors of the block applied to every real column right of it, one lane
// each, and to b | eta by one more lane.  KP >= k entries of W per lane in registers.
template <int KP>
__global__ __launch_bounds__(64) void obs_trail_kernel(ObsUpdateArgs a, int J, int ncols, int rhs) {
  extern __shared__ __attribute__((aligned(16))) double L[];
  double* const uL = L;              // [128][KP]
  double* const vbL = L + OB * KP;   // [2][128]
  const int lane = threadIdx.x;
  for (int idx = lane; idx < OB * KP; idx += 64) uL[idx] = a.u[(idx / KP) * 64 + idx % KP];
  for (int idx = lane; idx < 2 * OB; idx += 64) vbL[idx] = a.vb[idx];
  const int g = blockIdx.x * 64 + lane;
  const bool col = g < ncols, active = col || (rhs && g == ncols);
  const int64_t c = (int64_t)(J + 1) * OB + g;
  double* const rp = col ? a.R + (int64_t)J * OB * a.mp + c : a.b + (int64_t)J * OB;
  const int64_t rstride = col ? a.mp : 1;
  double* const wp = col ? a.W + c : a.eta;
  const int64_t wstride = col ? a.mp : 1;
  double w[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) w[i] = active ? wp[i * wstride] : 0.0;
  __syncthreads();
#pragma unroll 2
  for (int j = 0; j < OB; ++j) {
    const double v1 = vbL[j], beta = vbL[OB + j];
    if (beta == 0.0) continue;
    const double rho = active ? rp[j * rstride] : 0.0;
    const double* const u = uL + j * KP;
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < KP; ++i) dot += u[i] * w[i];
    const double tt = tp_factor(v1, beta, rho, dot);
#pragma unroll
    for (int i = 0; i < KP; ++i) w[i] -= tt * u[i];
    if (active) rp[j * rstride] = rho - tt * v1;
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < KP; ++i) wp[i * wstride] = w[i];
  }
}

template <int KP>
void launch_trail(const ObsUpdateArgs& a, int J, int ncols, int rhs, hipStream_t s) {
  constexpr int lds = (OB * KP + 2 * OB) * 8;
  static uint64_t done = 0;
  once_per_device(done, [] {
    GPR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&obs_trail_kernel<KP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  });
  hipLaunchKernelGGL(obs_trail_kernel<KP>, dim3((ncols + rhs + 63) / 64), dim3(64), lds, s, a, J, ncols, rhs);
  GPR_HIP(hipGetLastError());
}

}  // namespace

void launch_obs_rows(const ObsRowsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(obs_rows_kernel, dim3(OK_ROWS), dim3(256), 0, s, a);
  GPR_HIP(hipGetLastError());
}

void launch_obs_update(const ObsUpdateArgs& a, hipStream_t s) {
  static uint64_t done = 0;
  once_per_device(done, [] {
    GPR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&obs_diag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DIAG_LDS));
  });
  const int nb = a.mp / OB;
  const int rhs = a.b != nullptr;
  for (int J = 0; J < nb; ++J) {
    const bool last = J == nb - 1;
    hipLaunchKernelGGL(obs_diag_kernel, dim3(1), dim3(DIAG_THREADS), DIAG_LDS, s, a, J, last ? rhs : 0, last ? 1 : 0);
    GPR_HIP(hipGetLastError());
    if (last) break;
    const int ncols = a.m - (J + 1) * OB;  // real columns right of the block (the padded ones hold zeros in R~ and in W)
    if (a.k <= 4) launch_trail<4>(a, J, ncols, rhs, s);
    else if (a.k <= 16) launch_trail<16>(a, J, ncols, rhs, s);
    else launch_trail<64>(a, J, ncols, rhs, s);
  }
}

}  // namespace gprhip
