"""Cost of the acquisition criterion: Problem.predict_input_grad (all four outputs) and Problem.acquire timed INTERLEAVED in one
process on one device -- host wall time of the blocking calls, median of REPS after two warm-ups -- at n = 2000 / m = 50
(d = 3) with 1000 and 100 000 candidates, n = 10 000 / m = 256 (d = 8) with 100 000 and m = 2048 (d = 8, n = 100 000) with
1 000 000.  Columns: predict_input_grad with host buffers, twice (the spread between the two is the yardstick's own noise);
acquire (log EI) with values + dvalues to the host -- D nt + nt doubles instead of 2 D nt + 2 nt --; predict_input_grad on
device pointers; acquire with host inputs and only the best 16 candidates requested (nothing of size nt leaves the device);
then the HIP-event stage times (timing level 2) of one such top-k call, "acq_select" among them.  `predict_input_grad` is the
parent commit's, its kernels untouched: the yardstick of the same run.  Every line of the output file is written by this tool.
    usage (GPU box, repo root): timeout 900 python3 tools/bench_acquire.py [--out profiles/acquire_cost.txt] [--skip-big]
"""
import os
import sys
import time

import numpy as np

import torch  # noqa: F401  (first: one HIP runtime serves both)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpr_amd  # noqa: E402
from bench import synth  # noqa: E402

REPS = int(os.environ.get("REPS", 5))
TOP_K = 16
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
shapes = [("n=2000 m=50", 2000, 50, 3, 1000), ("n=2000 m=50", 2000, 50, 3, 100000), ("n=10000 m=256", 10000, 256, 8, 100000)]
if "--skip-big" not in sys.argv:
    shapes += [("n=100000 m=2048", 100000, 2048, 8, 1000000)]
lines = ["# tools/bench_acquire.py: predict_input_grad vs acquire (log EI), interleaved, host wall time in ms (median of %d after 2 warm-ups);" % REPS,
         "# grad host (twice): all four outputs to the host; acq host: values + dvalues to the host; grad dev: device pointers;",
         "# acq top%d: host inputs, only the best %d returned; stages: HIP events (timing level 2) of one top-k call, summed over its chunks" % (TOP_K, TOP_K),
         "%-16s %8s %10s %10s %10s %7s %10s %10s %7s   %s" % ("shape", "nt", "grad host", "grad host", "acq host", "ratio", "grad dev",
                                                            "acq top%d" % TOP_K, "ratio", "stages (ms)")]
for name, n, m, d, nt in shapes:
    X, y, Z = synth(1, n, m, d)
    kw = dict(log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(want_grad=False, **kw)
    rng = np.random.default_rng(2)
    Xt = np.asfortranarray(rng.normal(size=(d, nt)))
    xt = torch.tensor(np.ascontiguousarray(Xt.T), device="cuda:0")
    outs = {"means": torch.empty(nt, dtype=torch.float64, device="cuda:0"),
            "variances": torch.empty(nt, dtype=torch.float64, device="cuda:0"),
            "dmeans": torch.empty((nt, d), dtype=torch.float64, device="cuda:0"),
            "dvariances": torch.empty((nt, d), dtype=torch.float64, device="cuda:0")}
    ptrs = {k: v.data_ptr() for k, v in outs.items()}
    acq = dict(maximise=False, best=float(np.min(y)), xi=0.01)
    torch.cuda.synchronize()
    calls = [lambda: p.predict_input_grad(Xt),
             lambda: p.predict_input_grad(Xt),
             lambda: p.acquire(Xt, "log_ei", **acq),
             lambda: p.predict_input_grad(xt.data_ptr(), out_device_ptrs=ptrs, nt=nt),
             lambda: p.acquire(Xt, "log_ei", want=(), top_k=TOP_K, **acq)]
    times = [[] for _ in calls]
    for _ in range(REPS + 2):
        for t, f in zip(times, calls):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    g1, g2, ah, gd, at = (1e3 * float(np.median(t[2:])) for t in times)
    p.set_timing(2)
    p.acquire(Xt, "log_ei", want=(), top_k=TOP_K, **acq)
    st = p.last_timings()
    p.set_timing(0)
    stages = "  ".join("%s %.3f" % (k, v) for k, v in st.items() if k.startswith(("pg_", "acq_")))
    lines.append("%-16s %8d %10.3f %10.3f %10.3f %7.2f %10.3f %10.3f %7.2f   %s" % (name, nt, g1, g2, ah, ah / min(g1, g2), gd, at,
                                                                                 at / gd, stages))
    print(lines[-1], flush=True)
    p.close()
    del outs, xt, Xt, X, y, Z
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
