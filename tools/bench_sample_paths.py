"""Cost of the posterior sample paths: Problem.predict_input_grad (means + dmeans only, device pointers -- the parent commit's
kernel, untouched: the yardstick of the same run) and Problem.sample_paths timed INTERLEAVED in one process on one device --
host wall time of the blocking calls, median of REPS after two warm-ups -- at the four shapes of tools/bench_acquire.py:
n = 2000 / m = 50 (d = 3) with 1000 and 100 000 points, n = 10 000 / m = 256 (d = 8) with 100 000 and m = 2048 (d = 8,
n = 100 000) with 1 000 000.  Columns: the yardstick twice (the spread between the two is its own noise); the path part alone
with ns = 1, 16 and 64 draws on device pointers; ns = 16 with eps (device pointers); ns = 16 from host inputs with only the
best point of every draw requested (nothing of size nt leaves the device); then the HIP-event stage times (timing level 2) of
one ns = 16 call with eps and top-1, summed over its chunks.  Every line of the output file is written by this tool.
    usage (GPU box, repo root): timeout 900 python3 tools/bench_sample_paths.py [--out profiles/sample_paths_cost.txt] [--skip-big]
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
lines = ["# tools/bench_sample_paths.py: predict_input_grad (means + dmeans, device pointers) vs sample_paths, interleaved, host wall time in ms",
         "# (median of %d after 2 warm-ups); path ns=1/16/64: the path part alone on device pointers; +eps: ns = 16 with the residual part;" % REPS,
         "# top1: ns = 16, host inputs, only the best point of every draw returned; ratio = path ns=1 / the faster yardstick column;",
         "# stages: HIP events (timing level 2) of one ns = 16 call with eps and top-1, summed over its chunks",
         "%-16s %8s %9s %9s %9s %6s %9s %9s %9s %9s   %s" % ("shape", "nt", "grad dev", "grad dev", "path ns=1", "ratio", "path ns=16",
                                                            "path ns=64", "ns=16+eps", "ns=16 top1", "stages (ms)")]
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
    z = np.asfortranarray(rng.standard_normal((m, 64)))
    means = torch.empty(nt, dtype=torch.float64, device="cuda:0")
    dmeans = torch.empty((nt, d), dtype=torch.float64, device="cuda:0")
    F = torch.empty((64, nt), dtype=torch.float64, device="cuda:0")
    eps = torch.randn((16, nt), dtype=torch.float64, device="cuda:0")
    gptrs = {"means": means.data_ptr(), "dmeans": dmeans.data_ptr()}
    torch.cuda.synchronize()
    grad = lambda: p.predict_input_grad(xt.data_ptr(), want=("means", "dmeans"), out_device_ptrs=gptrs, nt=nt)
    path = lambda ns: p.sample_paths(xt.data_ptr(), z[:, :ns], out_device_ptrs={"samples": F.data_ptr()}, nt=nt)
    calls = [grad, grad, lambda: path(1), lambda: path(16), lambda: path(64),
             lambda: p.sample_paths(xt.data_ptr(), z[:, :16], eps=eps.data_ptr(), out_device_ptrs={"samples": F.data_ptr()}, nt=nt),
             lambda: p.sample_paths(Xt, z[:, :16], top_k=1, want_samples=False)]
    times = [[] for _ in calls]
    for _ in range(REPS + 2):
        for t, f in zip(times, calls):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    g1, g2, p1, p16, p64, pe, pt = (1e3 * float(np.median(t[2:])) for t in times)
    p.set_timing(2)
    p.sample_paths(xt.data_ptr(), z[:, :16], eps=eps.data_ptr(), top_k=1, out_device_ptrs={"samples": F.data_ptr()}, nt=nt)
    st = p.last_timings()
    p.set_timing(0)
    stages = "  ".join("%s %.3f" % (k, v) for k, v in st.items() if k.startswith("sp_"))
    lines.append("%-16s %8d %9.3f %9.3f %9.3f %6.2f %9.3f %9.3f %9.3f %9.3f   %s" % (name, nt, g1, g2, p1, p1 / min(g1, g2), p16, p64, pe,
                                                                                 pt, stages))
    print(lines[-1], flush=True)
    p.close()
    del F, eps, xt, Xt, X, y, Z, means, dmeans
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
