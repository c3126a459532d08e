"""Latency of a batch evaluation beside `count` single evaluations (gprhip_batch_eval against gprhip_eval).

For each shape -- C1 (n = 2000, m = 50, d = 3) and n = 1000, m = 10, d = 3 -- and each count in 1, 2, 4, 8, 16, 32, 64: the
median over REPS repetitions (after warm-up) of one gradient evaluation of `count` lanes, beside count x the median latency
of a single gprhip_eval measured in the same process, the two interleaved repetition by repetition.  Wall-clock times of the
blocking calls through the Python mirror, in milliseconds.

    python tools/bench_batch.py [--reps 50] [--out profiles/batch_latency.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpr_amd  # noqa: E402

SHAPES = [("C1", 2000, 50, 3), ("n1000_m10", 1000, 10, 3)]
COUNTS = [1, 2, 4, 8, 16, 32, 64]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# batch evaluation against single evaluations, gradient evaluations, medians of %d interleaved repetitions (ms)" % a.reps,
             "# shape count batch_ms single_ms count_x_single_ms ratio"]
    for name, n, m, d in SHAPES:
        rng = np.random.default_rng(3)
        X = np.asfortranarray(rng.normal(size=(d, n)))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
        p.set_inputs(X)
        p.set_targets(y)
        hyps = [dict(log_ell=0.5 * np.log(d) + 0.01 * j, log_sf2=0.0, sigma2=0.1 + 0.001 * j,
                     inducing=np.asfortranarray(X[:, rng.permutation(n)[:m]] + 0.01 * rng.normal(size=(d, m))))
                for j in range(max(COUNTS))]
        b = p.batch(max(COUNTS))
        for count in COUNTS:
            tb, ts = [], []
            for it in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                b.eval(hyps[:count])
                t1 = time.perf_counter()
                p.eval(**hyps[it % count])
                t2 = time.perf_counter()
                if it >= a.warmup:
                    tb.append((t1 - t0) * 1e3)
                    ts.append((t2 - t1) * 1e3)
            mb, ms = statistics.median(tb), statistics.median(ts)
            lines.append("%s %d %.4f %.4f %.4f %.2f" % (name, count, mb, ms, count * ms, mb / (count * ms)))
            print(lines[-1], flush=True)
        b.close()
        p.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
