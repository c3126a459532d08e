"""Cost of the prediction gradient: Problem.predict (means + variances) and Problem.predict_input_grad (all four outputs) timed
INTERLEAVED in one process on one device -- host wall time of the blocking calls, median of REPS after two warm-ups -- at
n = 2000 / m = 50 (d = 3) with 1000 and 100 000 test points, n = 10 000 / m = 256 (d = 8) with 100 000 and m = 2048 (d = 8,
n = 100 000) with 1 000 000; then the HIP-event stage times (timing level 2) of one predict_input_grad.  Both calls take host
test inputs and return host arrays, so the new call also carries 2 D nt doubles more back to the host; the third column is the
same call with device pointers (no transfer at all).  `predict` is the parent commit's, its kernels untouched: the yardstick of
the same run.  Every line of the output file is written by this tool.
    usage (GPU box, repo root): timeout 900 python3 tools/bench_predict_grad.py [--out profiles/predict_grad_cost.txt] [--skip-big]
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
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
shapes = [("n=2000 m=50", 2000, 50, 3, 1000), ("n=2000 m=50", 2000, 50, 3, 100000), ("n=10000 m=256", 10000, 256, 8, 100000)]
if "--skip-big" not in sys.argv:
    shapes += [("n=100000 m=2048", 100000, 2048, 8, 1000000)]
lines = ["# tools/bench_predict_grad.py: predict vs predict_input_grad, interleaved, host wall time (median of %d after 2 warm-ups);" % REPS,
         "# host: test inputs and all outputs cross the PCIe link; device: the same call on device pointers;",
         "# stages: HIP events (timing level 2) of one predict_input_grad (host), summed over its chunks",
         "%-16s %8s %11s %13s %7s %13s %7s   %s" % ("shape", "nt", "predict ms", "grad host ms", "ratio", "grad dev ms", "ratio",
                                                    "stages (ms)")]
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
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(REPS + 2):
        t0 = time.perf_counter()
        p.predict(Xt)
        t1 = time.perf_counter()
        p.predict_input_grad(Xt)
        t2 = time.perf_counter()
        p.predict_input_grad(xt.data_ptr(), out_device_ptrs=ptrs, nt=nt)
        t3 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
        tc.append(t3 - t2)
    a, b, c = (1e3 * float(np.median(t[2:])) for t in (ta, tb, tc))
    p.set_timing(2)
    p.predict_input_grad(Xt)
    st = p.last_timings()
    p.set_timing(0)
    stages = "  ".join("%s %.3f" % (k, v) for k, v in st.items() if k.startswith("pg_"))
    lines.append("%-16s %8d %11.3f %13.3f %7.2f %13.3f %7.2f   %s" % (name, nt, a, b, b / a, c, c / a, stages))
    print(lines[-1], flush=True)
    p.close()
    del outs, xt, Xt, X, y, Z
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
