// Host-side pieces of gprhip_sample_paths that need no device: the argument checks and the merge of two sorted best-k lists
// (the best so far and those of a new chunk).  Plain C++: gprhip.hip includes this, and so does tests/cpp/sample_paths_check.cpp,
// which runs both under the address and undefined-behaviour sanitizers on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gprhip {

constexpr int SP_HOST_MAX_DRAWS = 64;  // GPRHIP_MAX_DRAWS
constexpr int SP_HOST_MAX_TOP_K = 64;  // GPRHIP_MAX_TOP_K

// What the call is given, as far as the checks look at it (have_p = 0: the problem is NULL, D / d / m / f32 are not read)
struct SpCall {
  int have_p = 0, D = 0, d = 0, m = 0, f32 = 0;
  const void* z = nullptr;
  int64_t ldz = 0;
  int ns = 0;
  const void* test_inputs = nullptr;
  int64_t ld = 0, nt = 0;
  const void* eps = nullptr;
  int64_t lde = 0;
  const void* samples = nullptr;
  int64_t lds = 0;
  int top_k = 0;
  const void* top_index = nullptr;
  int on_device = 0;
};

// nullptr: the arguments are in order; else the reason (GPRHIP_EBADARG).  The checks that need no problem come first.
inline const char* sp_check_args(const SpCall& c) {
  if (c.ns < 1 || c.ns > SP_HOST_MAX_DRAWS) return "ns must lie in 1 .. GPRHIP_MAX_DRAWS (64)";
  if (c.top_k < 0 || c.top_k > SP_HOST_MAX_TOP_K) return "top_k must lie in 0 .. GPRHIP_MAX_TOP_K (64)";
  if (c.top_k > 0 && !c.top_index) return "top_k > 0 needs top_index";
  if (!c.samples && c.top_k == 0) return "nothing is requested (samples is NULL and top_k is 0)";
  if (!c.have_p || !c.z || !c.test_inputs || c.nt < 1) return "invalid arguments";
  if (c.f32) return "sample paths are evaluated in fp64 only (GPRHIP_F32_BULK problem)";
  if (c.d > 64) return "at most 64 point dimensions on the kernel side (d)";
  if (c.ldz < c.m) return "bad ldz (need ldz >= m)";
  if (c.on_device ? c.ld != c.D : c.ld < c.D) return "bad ld (need ld == D for device buffers, ld >= D for host buffers)";
  if (c.eps && c.lde < c.nt) return "bad lde (need lde >= nt)";
  if (c.samples && c.lds < c.nt) return "bad lds (need lds >= nt)";
  return nullptr;
}

// The best k of one draw so far: index, value and (D doubles each, or none) the gradient rows, best first.
struct SpBest {
  std::vector<int64_t> idx;
  std::vector<double> val, grad;
};

// Merges the sorted list of a chunk into `best` (both: sign * value descending, the lower index first among equal values).
// cidx[k] are the chunk's indices as doubles (-1 ends the list), cval[k] its values, cgrad [k][D] (or null); `offset` is
// added to the chunk's indices.  An earlier entry (a lower index) stays in front of an equal later one.
inline void sp_merge_topk(SpBest& best, int k, double sign, const double* cidx, const double* cval, const double* cgrad, int D,
                          int64_t offset) {
  SpBest out;
  size_t ia = 0;
  int ib = 0;
  while ((int)out.idx.size() < k) {
    const bool has_a = ia < best.idx.size(), has_b = ib < k && cidx[ib] >= 0.0;
    if (!has_a && !has_b) break;
    if (has_a && (!has_b || !(sign * cval[ib] > sign * best.val[ia]))) {
      out.idx.push_back(best.idx[ia]);
      out.val.push_back(best.val[ia]);
      if (cgrad) out.grad.insert(out.grad.end(), best.grad.begin() + ia * D, best.grad.begin() + (ia + 1) * D);
      ++ia;
    } else {
      out.idx.push_back(offset + (int64_t)cidx[ib]);
      out.val.push_back(cval[ib]);
      if (cgrad) out.grad.insert(out.grad.end(), cgrad + (int64_t)ib * D, cgrad + (int64_t)(ib + 1) * D);
      ++ib;
    }
  }
  best.idx.swap(out.idx);
  best.val.swap(out.val);
  best.grad.swap(out.grad);
}

}  // namespace gprhip
