"""Cost of refining max-value entropy search candidates on the device: Problem.acquire_max_value_refine on device pointers
against the floor of any host-driven loop -- `evals` times one Problem.acquire_max_value call (values + gradient, device
pointers) over the same ns points -- timed INTERLEAVED in one process on one device: host wall time of the blocking calls,
median of REPS after two warm-ups.  Shapes: n = 2000 / m = 50 (d = 3; the persistent kernel), n = 10 000 / m = 256 and
n = 100 000 / m = 2048 (d = 8; the library-side loop), each with 64 and 1024 starts and S = 1, 16, 64 extremes.  `evals` of a
refine call is its largest per-start evaluation count -- the number of evaluations the loop made; the yardstick runs that many
acquire_max_value calls, the kernels of the parent commit.  Then the HIP-event stage times (timing level 2) of one refine call.
The extremes are a ladder from the largest target to that plus 0.5: values that maxima of drawn paths take.
    usage (GPU box, repo root): timeout 900 python3 tools/bench_max_value_refine.py [--out profiles/max_value_refine_cost.txt] [--skip-big]
"""
import os
import sys
import time

import numpy as np

import torch  # noqa: F401  (first: one HIP runtime serves both)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpr_amd  # noqa: E402
from bench import synth  # noqa: E402

REPS = int(os.environ.get("REPS", 7))
MAX_EVALS = 40
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
shapes = [("n=2000 m=50", 2000, 50, 3), ("n=10000 m=256", 10000, 256, 8)]
if "--skip-big" not in sys.argv:
    shapes += [("n=100000 m=2048", 100000, 2048, 8)]
lines = ["# tools/bench_max_value_refine.py: acquire_max_value_refine (max_evals %d) vs evals x acquire_max_value, device pointers," % MAX_EVALS,
         "# interleaved, host wall time in ms (median of %d after 2 warm-ups, and the least and the largest of them for the refine call);" % REPS,
         "# per eval: the call over its evaluations; stages: HIP events (timing level 2) of one refine call, summed over its evaluations",
         "%-16s %6s %3s %6s %10s %12s %10s %12s %7s %15s   %s" % ("shape", "ns", "S", "evals", "refine", "refine/eval", "loop", "mv/call", "ratio",
                                                            "refine min-max", "stages (ms)")]
dev = "cuda:0"
for name, n, m, d in shapes:
    X, y, Z = synth(1, n, m, d)
    kw = dict(log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(want_grad=False, **kw)
    lo, hi = np.full(d, -3.0), np.full(d, 3.0)
    for ns in (64, 1024):
        S0 = np.random.default_rng(2).normal(size=(ns, d))
        st = torch.tensor(np.ascontiguousarray(np.clip(S0, -3.0, 3.0)), device=dev)
        outs = {"x": torch.empty((ns, d), dtype=torch.float64, device=dev), "values": torch.empty(ns, dtype=torch.float64, device=dev),
                "dvalues": torch.empty((ns, d), dtype=torch.float64, device=dev), "evals": torch.empty(ns, dtype=torch.int32, device=dev),
                "status": torch.empty(ns, dtype=torch.int32, device=dev)}
        ptrs = {k: v.data_ptr() for k, v in outs.items()}
        aptr = {"values": ptrs["values"], "dvalues": ptrs["dvalues"]}
        torch.cuda.synchronize()
        for S in (1, 16, 64):
            ext = float(np.max(y)) + np.linspace(0.0, 0.5, S)

            def refine():
                p.acquire_max_value_refine(st.data_ptr(), ext, lower=lo, upper=hi, maximise=True, max_evals=MAX_EVALS, want=tuple(ptrs),
                                           out_device_ptrs=ptrs, ns=ns)

            refine()
            evals = int(outs["evals"].max().item())

            def loop():
                for _ in range(evals):
                    p.acquire_max_value(st.data_ptr(), ext, maximise=True, want=tuple(aptr), out_device_ptrs=aptr, nt=ns)

            times = [[], []]
            for _ in range(REPS + 2):
                for t, f in zip(times, (refine, loop)):
                    t0 = time.perf_counter()
                    f()
                    t.append(time.perf_counter() - t0)
            tr, tl = (1e3 * float(np.median(t[2:])) for t in times)
            spread = "%.3f-%.3f" % (1e3 * min(times[0][2:]), 1e3 * max(times[0][2:]))
            p.set_timing(2)
            refine()
            stg = p.last_timings()
            p.set_timing(0)
            stages = "  ".join("%s %.3f" % (k, v) for k, v in stg.items() if k.startswith(("pg_", "rf_")))
            lines.append("%-16s %6d %3d %6d %10.3f %12.4f %10.3f %12.4f %7.2f %15s   %s" % (name, ns, S, evals, tr, tr / evals, tl, tl / evals,
                                                                                      tr / tl, spread, stages))
            print(lines[-1], flush=True)
        del outs, st
    p.close()
    del X, y, Z
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
