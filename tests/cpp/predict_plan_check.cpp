// Stand-alone check of the chunk plan of the calls at test points (gpr_amd/csrc/predict_plan.h): the rule against a table
// worked out by hand, and a randomised sweep of call sequences that carries the buffer sizes forward as the allocation step
// does.  No device, no library: built with -fsanitize=address,undefined and run on the CPU by tests/test_predict_plan_host.py.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../gpr_amd/csrc/predict_plan.h"

using namespace gprhip;

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);             \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

struct Row {
  int64_t train, nt;
  int mats;  // 0 / 1; -1: either
  int64_t pred_rows, xt_rows;  // pred_rows -1: any
  int64_t chunk;
  bool grow_pred, grow_xt;
};

static void check_table() {
  const Row rows[] = {
      {2048, 100, -1, 0, 0, 2048, false, true},
      {2048, 100, -1, 0, 2048, 2048, false, false},
      {2048, 5000, 1, 0, 0, 16384, true, true},
      {2048, 10000, 1, 16384, 16384, 16384, false, false},
      {2048, 20000, 1, 16384, 16384, 20096, true, true},
      {2048, 100000, 1, 0, 0, 100096, true, true},
      {2048, 131072 + 65, 1, 0, 0, 131072, true, true},
      {2048, 5000, 1, 16384, 100096, 16384, false, false},
      {2048, 5000, 0, -1, 0, 16384, false, true},
      {2048, 5000, 0, -1, 100096, 100096, false, false},
      {2048, 20000, 0, -1, 16384, 20096, false, true},
      {131072, 1000000, -1, 0, 0, 131072, false, true},
  };
  for (const Row& r : rows)
    for (int mats = 0; mats < 2; ++mats) {
      if (r.mats >= 0 && r.mats != mats) continue;
      for (int64_t pred : {int64_t(0), int64_t(2048), int64_t(16384), int64_t(131072)}) {
        if (r.pred_rows >= 0 && pred != r.pred_rows) continue;
        const ChunkPlan c = predict_plan(r.train, r.nt, mats != 0, pred, r.xt_rows);
        EXPECT(c.chunk == r.chunk);
        EXPECT(c.grow_pred == r.grow_pred);
        EXPECT(c.grow_xt == r.grow_xt);
        if (failures) std::fprintf(stderr, "  (nt %lld mats %d pred_rows %lld xt_rows %lld: chunk %lld)\n", (long long)r.nt, mats,
                                   (long long)pred, (long long)r.xt_rows, (long long)c.chunk);
      }
    }
  // nt = 131072 + 65 goes through in chunks of 131072 and 65 rows
  const ChunkPlan two = predict_plan(2048, 131072 + 65, true, 0, 0);
  EXPECT(131072 + 65 - two.chunk == 65);
}

// call sequences on one problem: pred_rows / xt_rows are carried forward as chunk_alloc of gprhip.hip leaves them
static void check_sweep() {
  std::mt19937_64 gen(11);
  const int64_t trains[] = {128, 256, 2048, 4096, 65536, 131072, 262144};
  for (int trial = 0; trial < 2000; ++trial) {
    const int64_t train = trains[gen() % 7];
    int64_t pred_rows = 0, xt_rows = 0;
    for (int call = 0; call < 12; ++call) {
      int64_t nt;
      switch (gen() % 4) {
        case 0: nt = 1 + (int64_t)(gen() % 300); break;
        case 1: nt = 1 + (int64_t)(gen() % (10 * train)); break;
        case 2: nt = 131072 - 200 + (int64_t)(gen() % 400); break;
        default: nt = 1 + (int64_t)(gen() % 400000); break;
      }
      const bool mats = gen() % 2;
      const ChunkPlan c = predict_plan(train, nt, mats, pred_rows, xt_rows);
      const int64_t want = std::min<int64_t>(131072, (nt + 127) / 128 * 128);
      EXPECT(c.chunk >= train && c.chunk >= 1);
      // one chunk whenever the call does not fit the training chunk and has at most 131072 points
      if (nt <= 131072 && want > train) EXPECT(c.chunk >= nt);
      // the buffers the plan says will exist hold the chunk, and none shrinks
      const int64_t pred_after = c.grow_pred ? c.chunk : pred_rows;
      const int64_t xt_after = c.grow_xt ? c.chunk : xt_rows;
      EXPECT(pred_after >= pred_rows && xt_after >= xt_rows);
      EXPECT(xt_after >= c.chunk);
      if (mats && c.chunk > train) EXPECT(pred_after >= c.chunk);  // (up to the training chunk K lives in the training buffers)
      if (!mats) EXPECT(!c.grow_pred);
      // growth only where the buffer is too small for the chunk
      EXPECT(c.grow_xt == (xt_rows < c.chunk));
      if (c.grow_pred) EXPECT(pred_rows < want);
      pred_rows = pred_after;
      xt_rows = xt_after;
    }
  }
}

int main() {
  check_table();
  check_sweep();
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("predict_plan_check: ok\n");
  return 0;
}
