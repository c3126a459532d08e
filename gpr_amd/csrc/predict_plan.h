// The chunk rule of every call that evaluates the model at test points (gprhip_predict, _predict_input_grad, _acquire,
// _sample_paths).  Plain C++ with no device and no problem: gprhip.hip includes this, and so does
// tests/cpp/predict_plan_check.cpp, which pins the rule to a table on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>

namespace gprhip {

constexpr int64_t PLAN_TILE = 128;            // TILE of common.h (gprhip.hip asserts it)
constexpr int64_t PLAN_MAX_CHUNK = 131072;    // most rows of a chunk in buffers of the call's own

struct ChunkPlan {
  int64_t chunk;   // test points per chunk
  bool grow_pred;  // predA / predB (K and the second matrix of a chunk) must be regrown, to `chunk` rows
  bool grow_xt;    // the xt / pt / prow scratch must be regrown, to `chunk` rows
};

// Test points go through in chunks of their own: the training chunk (at most the training set, padded) when it holds the call,
// else up to 131072 rows in buffers kept for later calls, max(want, 8 * training chunk) rows when they must grow -- a model
// trained on 2000 points predicts 100 000 test points in one pass instead of 49 (5.4 -> 0.7 ms), each of which ends in a
// stream synchronisation.  mats: K and the second matrix of a chunk live in memory (predA / predB beyond the training chunk);
// without them (one kernel per chunk, or means only) a chunk needs the row buffers only, which then set its size -- not
// two chunk x mp matrices (268 MB at 131072 rows that a cached small model would pin for nothing).
inline ChunkPlan predict_plan(int64_t train_chunk, int64_t nt, bool mats, int64_t pred_rows, int64_t xt_rows) {
  ChunkPlan c{train_chunk, false, false};
  const int64_t want = std::min(PLAN_MAX_CHUNK, (nt + PLAN_TILE - 1) / PLAN_TILE * PLAN_TILE);
  if (want > train_chunk) {
    const int64_t rows = std::min(PLAN_MAX_CHUNK, std::max(want, 8 * train_chunk));
    if (mats) {
      c.grow_pred = pred_rows < want;
      c.chunk = c.grow_pred ? rows : pred_rows;
    } else {
      c.chunk = std::max(xt_rows >= want ? xt_rows : rows, train_chunk);
    }
  }
  c.grow_xt = xt_rows < c.chunk;
  return c;
}

}  // namespace gprhip
