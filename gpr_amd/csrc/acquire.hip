// The best k of the criterion values of one chunk of gprhip_acquire, with their gradient rows.
//
// Order: value descending, the lower index first among equal values (bitwise equal ones, and -0 = +0); NaN is never
// selected.  A value becomes a 64-bit key that orders as the doubles do (0 = "nothing": NaN, or beyond the rows), so every
// comparison is one of integers.
//   * acq_select_slab_kernel: a slab of 2048 values in LDS per workgroup; k times the arg-max of the slab, the winner struck
//     out.  A thread keeps the best of its own eight entries in registers and looks at them again only after one of them won.
//   * acq_select_merge_kernel (one workgroup): the slabs' lists are sorted, so the best k of the chunk are k steps of a merge
//     over the list heads, one list per thread, the lower slab -- the lower index -- winning a tie; then the same workgroup
//     gathers index, value and gradient row of the k winners into one block.
// No atomics: two runs give the same bits.
#include "kernels.h"

namespace gprhip {

namespace {

constexpr int SEL_SLAB = 2048;          // values per workgroup
constexpr int SEL_PER = SEL_SLAB / 256;  // ... per thread

__device__ __forceinline__ unsigned long long sel_key(double v) {
  if (v != v) return 0ull;
  const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);  // (-0 + 0 = +0)
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// the better of two candidates (key, position): the larger key, the lower position among equal keys
__device__ __forceinline__ void sel_take(unsigned long long& k, int& i, unsigned long long ok, int oi) {
  if (ok > k || (ok == k && oi < i)) {
    k = ok;
    i = oi;
  }
}

// the workgroup's best candidate; wk / wi: one slot per wavefront.  Ends with every thread past its reads of wk / wi.
__device__ __forceinline__ void sel_block_best(unsigned long long& k, int& i, unsigned long long* wk, int* wi, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long ok = __shfl_xor(k, off);
    const int oi = __shfl_xor(i, off);
    sel_take(k, i, ok, oi);
  }
  if ((tid & 63) == 0) {
    wk[tid >> 6] = k;
    wi[tid >> 6] = i;
  }
  __syncthreads();
  k = wk[0];
  i = wi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) sel_take(k, i, wk[w], wi[w]);
  __syncthreads();
}

// (blockIdx.y: the value column -- ldv doubles apart, its candidate lists gridDim.x * k entries apart; sign: +1 the largest,
//  -1 the smallest)
__global__ __launch_bounds__(256) void acq_select_slab_kernel(const double* __restrict__ values, int64_t ldv, double sign,
                                                               int rows, int k, unsigned long long* __restrict__ ckey,
                                                               int* __restrict__ cidx) {
  __shared__ unsigned long long keys[SEL_SLAB];
  __shared__ unsigned long long wk[4];
  __shared__ int wi[4];
  const int tid = threadIdx.x, base = blockIdx.x * SEL_SLAB;
  values += (int64_t)blockIdx.y * ldv;
  ckey += (int64_t)blockIdx.y * gridDim.x * k;
  cidx += (int64_t)blockIdx.y * gridDim.x * k;
  for (int i = tid; i < SEL_SLAB; i += 256) keys[i] = base + i < rows ? sel_key(sign * values[base + i]) : 0ull;
  __syncthreads();
  unsigned long long bk;
  int bi;
  auto own = [&] {  // entries tid, tid + 256, ...: ascending, so the first of equal keys stays
    bk = 0ull;
    bi = tid;
#pragma unroll
    for (int j = 0; j < SEL_PER; ++j) {
      const unsigned long long kk = keys[tid + 256 * j];
      if (kk > bk) {
        bk = kk;
        bi = tid + 256 * j;
      }
    }
  };
  own();
  for (int it = 0; it < k; ++it) {
    unsigned long long gk = bk;
    int gi = bi;
    sel_block_best(gk, gi, wk, wi, tid);
    if (tid == 0) {
      ckey[(int64_t)blockIdx.x * k + it] = gk;
      cidx[(int64_t)blockIdx.x * k + it] = gk ? base + gi : -1;
    }
    if (gk && (gi & 255) == tid) {  // the winner's owner strikes it out (no other thread reads that entry)
      keys[gi] = 0ull;
      own();
    }
  }
}

// out: [k] indices (as doubles; -1: fewer than k values qualify) | [k] values | [k][D] gradient rows (grads null: not written)
__global__ __launch_bounds__(256) void acq_select_merge_kernel(const unsigned long long* __restrict__ ckey,
                                                                const int* __restrict__ cidx, int nslabs, int k,
                                                                const double* __restrict__ values, int64_t ldv,
                                                                const double* __restrict__ grads, int D,
                                                                double* __restrict__ out, int64_t out_stride) {
  __shared__ unsigned long long wk[4];
  __shared__ int wi[4];
  __shared__ int sel[64];
  const int tid = threadIdx.x;
  values += (int64_t)blockIdx.y * ldv;
  ckey += (int64_t)blockIdx.y * nslabs * k;
  cidx += (int64_t)blockIdx.y * nslabs * k;
  out += (int64_t)blockIdx.y * out_stride;
  int head = 0;
  unsigned long long bk = tid < nslabs ? ckey[(int64_t)tid * k] : 0ull;
  for (int it = 0; it < k; ++it) {
    unsigned long long gk = bk;
    int gs = tid;
    sel_block_best(gk, gs, wk, wi, tid);
    if (gs == tid) {
      sel[it] = gk ? cidx[(int64_t)tid * k + head] : -1;
      if (gk) {
        ++head;
        bk = head < k ? ckey[(int64_t)tid * k + head] : 0ull;
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < k; j += 256) {
    out[j] = (double)sel[j];
    out[k + j] = sel[j] >= 0 ? values[sel[j]] : 0.0;
  }
  if (grads)
    for (int e = tid; e < k * D; e += 256) {
      const int j = e / D, b = e - j * D;
      out[2 * k + e] = sel[j] >= 0 ? grads[(int64_t)sel[j] * D + b] : 0.0;
    }
}

}  // namespace

int64_t acq_select_scratch_bytes() { return (int64_t)ACQ_SELECT_MAX_SLABS * ACQ_MAX_TOP_K * 12; }

void launch_acq_select(const AcqSelectArgs& a, hipStream_t s) {
  const int nslabs = (a.rows + SEL_SLAB - 1) / SEL_SLAB;
  if (a.rows <= 0 || a.k < 1 || a.k > ACQ_MAX_TOP_K || nslabs > ACQ_SELECT_MAX_SLABS) {
    set_error("gprhip: the selection takes 1 .. 64 candidates out of at most 524288 values per launch");
    throw HipFail{ST_BAD_ARG};
  }
  unsigned long long* const ckey = static_cast<unsigned long long*>(a.scratch);
  int* const cidx = reinterpret_cast<int*>(ckey + (int64_t)ACQ_SELECT_MAX_SLABS * ACQ_MAX_TOP_K);
  hipLaunchKernelGGL(acq_select_slab_kernel, dim3(nslabs), dim3(256), 0, s, a.values, (int64_t)0, 1.0, a.rows, a.k, ckey, cidx);
  hipLaunchKernelGGL(acq_select_merge_kernel, dim3(1), dim3(256), 0, s, ckey, cidx, nslabs, a.k, a.values, (int64_t)0, a.grads,
                     a.D, a.out, (int64_t)0);
  GPR_HIP(hipGetLastError());
}

int64_t acq_select_many_scratch_bytes(int64_t rows, int k, int ncols) {
  return ((rows + SEL_SLAB - 1) / SEL_SLAB) * (int64_t)k * ncols * 12;
}

void launch_acq_select_many(const AcqSelectManyArgs& a, hipStream_t s) {
  const int nslabs = (a.rows + SEL_SLAB - 1) / SEL_SLAB;
  if (a.rows <= 0 || a.k < 1 || a.k > ACQ_MAX_TOP_K || nslabs > ACQ_SELECT_MAX_SLABS || a.ncols < 1 || a.ldv < a.rows ||
      a.out_stride < 2 * a.k) {
    set_error("gprhip: the selection takes 1 .. 64 candidates out of at most 524288 values per column and launch");
    throw HipFail{ST_BAD_ARG};
  }
  unsigned long long* const ckey = static_cast<unsigned long long*>(a.scratch);
  int* const cidx = reinterpret_cast<int*>(ckey + (int64_t)nslabs * a.k * a.ncols);
  hipLaunchKernelGGL(acq_select_slab_kernel, dim3(nslabs, a.ncols), dim3(256), 0, s, a.values, a.ldv, a.sign, a.rows, a.k, ckey,
                     cidx);
  hipLaunchKernelGGL(acq_select_merge_kernel, dim3(1, a.ncols), dim3(256), 0, s, ckey, cidx, nslabs, a.k, a.values, a.ldv,
                     static_cast<const double*>(nullptr), 0, a.out, a.out_stride);
  GPR_HIP(hipGetLastError());
}

}  // namespace gprhip
