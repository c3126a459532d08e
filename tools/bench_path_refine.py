"""Cost of refining drawn sample paths on the device: Problem.sample_paths_refine on device pointers (16 draws, max_evals 40)
against the floor of any host-driven loop -- `evals` times one Problem.predict_input_grad call asking for means + dmeans on
device pointers over the same ns points (the parent commit's kernels; the yardstick of profiles/sample_paths_cost.txt) --
timed INTERLEAVED in one process on one device: host wall time of the blocking calls, median of REPS after two warm-ups.
Shapes as tools/bench_refine.py: n = 2000 / m = 50 (d = 3), n = 10 000 / m = 256 and n = 100 000 / m = 2048 (d = 8), each with
64 and 1024 starts.  `evals` of a refine call is its largest per-start evaluation count.  Then the HIP-event stage times
(timing level 2) of one refine call.  The table is written by this tool; a comparison of runs may follow it as comment lines.
    usage (GPU box, repo root): timeout 900 python3 tools/bench_path_refine.py [--out profiles/path_refine_cost.txt] [--skip-big]
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
MAX_EVALS, ND = 40, 16
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
shapes = [("n=2000 m=50", 2000, 50, 3), ("n=10000 m=256", 10000, 256, 8)]
if "--skip-big" not in sys.argv:
    shapes += [("n=100000 m=2048", 100000, 2048, 8)]
lines = ["# tools/bench_path_refine.py: sample_paths_refine (%d draws, max_evals %d) vs evals x predict_input_grad (means + dmeans)," % (ND, MAX_EVALS),
         "# device pointers, interleaved, host wall time in ms (median of %d after 2 warm-ups, and the least and the largest of them for the refine call); per eval: the call over its" % REPS,
         "# evaluations; stages: HIP events (timing level 2) of one refine call",
         "%-16s %6s %6s %10s %12s %10s %12s %7s %15s   %s" % ("shape", "ns", "evals", "refine", "refine/eval", "loop", "grad/call", "ratio", "refine min-max",
                                                        "stages (ms)")]
dev = "cuda:0"
for name, n, m, d in shapes:
    X, y, Z = synth(1, n, m, d)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(want_grad=False, log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
    rng = np.random.default_rng(2)
    z = rng.standard_normal((m, ND))
    lo, hi = np.full(d, -3.0), np.full(d, 3.0)
    for ns in (64, 1024):
        S = rng.normal(size=(ns, d))
        dr = (np.arange(ns) % ND).astype(np.int32)
        st = torch.tensor(np.ascontiguousarray(np.clip(S, -3.0, 3.0)), device=dev)
        outs = {"x": torch.empty((ns, d), dtype=torch.float64, device=dev), "values": torch.empty(ns, dtype=torch.float64, device=dev),
                "dvalues": torch.empty((ns, d), dtype=torch.float64, device=dev), "evals": torch.empty(ns, dtype=torch.int32, device=dev),
                "status": torch.empty(ns, dtype=torch.int32, device=dev)}
        ptrs = {k: v.data_ptr() for k, v in outs.items()}
        torch.cuda.synchronize()

        def refine():
            p.sample_paths_refine(st.data_ptr(), z, dr, lower=lo, upper=hi, max_evals=MAX_EVALS, want=tuple(ptrs),
                                  out_device_ptrs=ptrs, ns=ns)

        refine()
        evals = int(outs["evals"].max().item())
        gptr = {"means": ptrs["values"], "dmeans": ptrs["dvalues"]}

        def loop():
            for _ in range(evals):
                p.predict_input_grad(st.data_ptr(), want=("means", "dmeans"), out_device_ptrs=gptr, nt=ns)

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
        stages = "  ".join("%s %.3f" % (k, v) for k, v in stg.items() if k.startswith(("sp_", "prf_", "rf_")))
        lines.append("%-16s %6d %6d %10.3f %12.4f %10.3f %12.4f %7.2f %15s   %s" % (name, ns, evals, tr, tr / evals, tl, tl / evals, tr / tl, spread, stages))
        print(lines[-1], flush=True)
        del outs, st
    p.close()
    del X, y, Z
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
