"""Cost of max-value entropy search: Problem.acquire (log EI) and Problem.acquire_max_value with S = 1, 16, 64 extremes timed
INTERLEAVED in one process on one device -- host wall time of the blocking calls, median of REPS after two warm-ups -- at the
shapes of tools/bench_acquire.py.  Two forms of each call: on device pointers (values + dvalues written in place) and with
only the best 16 candidates requested (nothing of size nt leaves the device).  The log-EI call runs the parent commit's
kernels untouched: it is the yardstick of the same run, and the ratio per shape and S is what is reported.  Then the
HIP-event stage times (timing level 2) of one S = 64 top-k call: the epilogue is part of "pg_grad".  Every line of the output
file is written by this tool.
    usage (GPU box, repo root): timeout 900 python3 tools/bench_max_value.py [--out profiles/max_value_cost.txt] [--skip-big]
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
COUNTS = (1, 16, 64)
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
shapes = [("n=2000 m=50", 2000, 50, 3, 1000), ("n=2000 m=50", 2000, 50, 3, 100000), ("n=10000 m=256", 10000, 256, 8, 100000)]
if "--skip-big" not in sys.argv:
    shapes += [("n=100000 m=2048", 100000, 2048, 8, 1000000)]
lines = ["# tools/bench_max_value.py: acquire (log EI) vs acquire_max_value with S extremes, interleaved, host wall time in ms (median of %d" % REPS,
         "# after 2 warm-ups).  dev: device pointers, values + dvalues written in place; top%d: only the best %d returned; ratio: over the" % (TOP_K, TOP_K),
         "# log-EI call of the same form; stages: HIP events (timing level 2) of one S = 64 top-k call, summed over its chunks",
         "%-16s %8s %5s %10s %10s %7s %10s %10s %7s" % ("shape", "nt", "S", "logEI dev", "MES dev", "ratio", "logEI top", "MES top", "ratio")]
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
    outs = {"values": torch.empty(nt, dtype=torch.float64, device="cuda:0"),
            "dvalues": torch.empty((nt, d), dtype=torch.float64, device="cuda:0")}
    ptrs = {k: v.data_ptr() for k, v in outs.items()}
    acq = dict(maximise=False, best=float(np.min(y)), xi=0.01)
    # minima of drawn paths lie around and below the smallest target: gamma of both signs over the candidates
    ext = {S: float(np.min(y)) + 0.3 * rng.normal(size=S) for S in COUNTS}
    torch.cuda.synchronize()
    want = ("values", "dvalues")
    calls = [lambda: p.acquire(xt.data_ptr(), "log_ei", want=want, out_device_ptrs=ptrs, nt=nt, **acq),
             lambda: p.acquire(xt.data_ptr(), "log_ei", want=(), out_device_ptrs={}, nt=nt, top_k=TOP_K, **acq)]
    for S in COUNTS:
        calls.append(lambda S=S: p.acquire_max_value(xt.data_ptr(), ext[S], maximise=False, want=want, out_device_ptrs=ptrs, nt=nt))
        calls.append(lambda S=S: p.acquire_max_value(xt.data_ptr(), ext[S], maximise=False, want=(), out_device_ptrs={}, nt=nt,
                                                     top_k=TOP_K))
    times = [[] for _ in calls]
    for _ in range(REPS + 2):
        for t, f in zip(times, calls):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    med = [1e3 * float(np.median(t[2:])) for t in times]
    for i, S in enumerate(COUNTS):
        md, mt = med[2 + 2 * i], med[3 + 2 * i]
        lines.append("%-16s %8d %5d %10.3f %10.3f %7.2f %10.3f %10.3f %7.2f" % (name, nt, S, med[0], md, md / med[0], med[1], mt,
                                                                               mt / med[1]))
        print(lines[-1], flush=True)
    p.set_timing(2)
    calls[-1]()
    st = p.last_timings()
    p.set_timing(0)
    lines.append("#   stages (ms), S = 64 top-k: " + "  ".join("%s %.3f" % (k, v) for k, v in st.items() if k.startswith(("pg_", "acq_"))))
    print(lines[-1], flush=True)
    p.close()
    del outs, xt, Xt, X, y, Z
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
