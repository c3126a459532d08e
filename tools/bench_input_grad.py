"""Cost of the input gradient: Problem.eval (gradient evaluation) and Problem.eval_input_grad timed INTERLEAVED in one
process on one device -- host wall time of the blocking calls, median of REPS after two warm-ups -- at C1 (n = 2000, m = 50,
d = 3), n = 10 000 / m = 256 (d = 8), C2 (n = 10^6, m = 2048, d = 8) and C3 (Cov_se_fat with a 32 x 32 projection, n = 10^6,
m = 4096: K_nm read from the resident store, then the G tproj^T kernel); then the HIP-event stage times (timing level 2):
"p2_xgrad" of one eval_input_grad (the new kernels, per chunk) beside "p2_grad" (the hyper-gradient kernel and its
reductions) of one plain eval in the same process -- the hyper-gradient kernels are the parent commit's, unchanged, so this
is the parent's stage on the same box -- and of the eval_input_grad itself.  On the one-kernel row paths the gradient sums
are part of "p2_small" / "p2_mid", which is then the figure printed.  The aim is p2_xgrad <= 1.5 x p2_grad.  The
device-pointer output is used, so no n x D transfer to the host is inside the figures.  Every line of the output file is
written by this tool.
    usage (GPU box, repo root): timeout 900 python3 tools/bench_input_grad.py [--out profiles/input_grad_cost.txt] [--skip-big]
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
shapes = [("C1", 2000, 50, 3), ("n=10000 m=256", 10000, 256, 8)]
if "--skip-big" not in sys.argv:
    shapes += [("C2", 1000000, 2048, 8), ("C3 (projection)", 1000000, 4096, 32)]
lines = ["# tools/bench_input_grad.py: eval vs eval_input_grad, interleaved, host wall time (median of %d after 2 warm-ups);" % REPS,
         "# stages: HIP events (timing level 2); p2_xgrad of one eval_input_grad; p2_grad of one plain eval in the same process",
         "# (the parent commit's kernels, unchanged) and, last column, of the eval_input_grad itself; X bytes = 8 n mp",
         "%-16s %10s %14s %8s %12s %12s %8s %10s %14s" % ("shape", "eval ms", "input_grad ms", "ratio", "p2_xgrad ms", "p2_grad ms",
                                                          "ratio", "X GB/s", "p2_grad (own)")]
ratios = {}
for name, n, m, d in shapes:
    if name.startswith("C3"):  # bench.py's C3: ARD as a diagonal projection
        rng = np.random.default_rng(3)
        X = np.asfortranarray(rng.normal(size=(d, n)))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        P = np.asfortranarray(np.diag(np.exp(-rng.uniform(-0.5, 0.5, size=d))) / np.sqrt(d))
        Z = np.asfortranarray((P.T @ X[:, rng.permutation(n)[:m]]) + 0.01 * rng.normal(size=(d, m)))
        kw = dict(log_sf2=0.0, sigma2=0.1, inducing=Z, tproj=P)
        p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, d, d, m)
    else:
        X, y, Z = synth(1, n, m, d)
        kw = dict(log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    out = torch.empty((n, d), dtype=torch.float64, device="cuda:0")
    ta, tb = [], []
    for _ in range(REPS + 2):
        t0 = time.perf_counter()
        p.eval(**kw)
        t1 = time.perf_counter()
        p.eval_input_grad(out_device_ptr=out.data_ptr(), **kw)
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    a, b = 1e3 * float(np.median(ta[2:])), 1e3 * float(np.median(tb[2:]))
    p.set_timing(2)
    p.eval(**kw)
    p.eval(**kw)
    st0 = p.last_timings()
    p.eval_input_grad(out_device_ptr=out.data_ptr(), **kw)
    p.eval_input_grad(out_device_ptr=out.data_ptr(), **kw)
    st = p.last_timings()
    gname = "p2_grad" if "p2_grad" in st else ("p2_small" if "p2_small" in st else "p2_mid")
    xg, gr = st["p2_xgrad"], st0[gname]
    mp = -(-m // 128) * 128
    ratios[name] = (xg / gr, 8.0 * n * mp / xg / 1e9, b / a)
    line = "%-16s %10.3f %14.3f %8.3f %12.4f %12.4f %8.3f %10.0f %14.4f" % (name, a, b, b / a, xg, gr, xg / gr,
                                                                            8.0 * n * mp / xg / 1e6, st[gname])
    lines.append(line + ("" if gname == "p2_grad" else "   (%s: the whole one-kernel pass 2)" % gname))
    print(lines[-1], flush=True)
    p.close()
    del out, X, y, Z
for name, (r, tbs, ev) in ratios.items():
    if name.startswith("C2") or name.startswith("C3"):
        lines.append("# %s: p2_xgrad / p2_grad = %.2f (aim: <= 1.5), %.2f TB/s over the one read of X, evaluation x %.3f"
                     % (name, r, tbs, ev))
        print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
