"""Cost of gprhip_observe beside the refit it replaces:  python tools/bench_observe.py [out]   (default profiles/observe_cost.txt)

Shapes n = 2000 / m = 50, n = 10 000 / m = 256, n = 16 384 / m = 2048 (d = 3), k = 1, 16, 64.  Per shape and k, interleaved in
one process (observe, yardstick, observe, ...; medians of REPS rounds after one warm-up round):
  observe      Problem.observe on the n-row state, wall clock around the call (it ends synchronised), and its four stage timers
               (HIP events, timing level 2); the state is put back by posterior_restore between rounds (not timed)
  refit        an evidence-only Problem.eval of the n + k problem, wall clock, and that evaluation's "b_chol" stage
Nothing is asserted."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: one HIP runtime serves both)
import numpy as np  # noqa: E402

import gpr_amd  # noqa: E402
from tests.util import synth  # noqa: E402

SHAPES = ((2000, 50), (10000, 256), (16384, 2048))
KS = (1, 16, 64)
REPS = 7
D = 3
STAGES = ("obs_rows", "obs_update", "obs_inverse", "obs_vectors")


def main(out_path):
    lines = ["# tools/bench_observe.py on %s; milliseconds, medians of %d interleaved rounds; d = %d, sigma2 = 0.1"
             % (torch.cuda.get_device_name(0), REPS, D),
             "# n m k | observe wall | " + " ".join(STAGES) + " | refit(n + k) wall | its b_chol | refit / observe | b_chol / observe"]
    for n, m in SHAPES:
        X, y, Z = synth(77 + m, n + 64, m, D)
        hyp = dict(log_ell=0.5 * np.log(D), log_sf2=0.0, sigma2=0.1, inducing=Z, want_grad=False)
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, D, D, m)
        p.set_inputs(np.asfortranarray(X[:, :n]))
        p.set_targets(y[:n].copy())
        p.eval(**hyp)
        p.posterior_save()
        p.set_timing(2)
        for k in KS:
            q = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n + k, D, D, m)
            q.set_inputs(np.asfortranarray(X[:, :n + k]))
            q.set_targets(y[:n + k].copy())
            q.set_timing(2)
            Xn, yn = np.asfortranarray(X[:, n:n + k]), y[n:n + k].copy()
            rec = {s: [] for s in STAGES + ("obs", "refit", "b_chol")}
            for r in range(REPS + 1):
                t0 = time.perf_counter()
                p.observe(Xn, yn)
                t1 = time.perf_counter()
                tm = p.last_timings()
                p.posterior_restore()
                t2 = time.perf_counter()
                q.eval(**hyp)
                t3 = time.perf_counter()
                tq = q.last_timings()
                if r == 0:
                    continue
                rec["obs"].append((t1 - t0) * 1e3)
                rec["refit"].append((t3 - t2) * 1e3)
                rec["b_chol"].append(tq.get("b_chol", float("nan")))
                for s in STAGES:
                    rec[s].append(tm.get(s, float("nan")))
            q.close()
            med = {s: statistics.median(v) for s, v in rec.items()}
            line = "%6d %5d %3d | %8.3f | %s | %9.3f | %8.3f | %7.1f | %6.2f" % (
                n, m, k, med["obs"], " ".join("%7.3f" % med[s] for s in STAGES), med["refit"], med["b_chol"],
                med["refit"] / med["obs"], med["b_chol"] / med["obs"])
            print(line, flush=True)
            lines.append(line)
        p.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "observe_cost.txt"))
