"""Cost of evaluating K target vectors on one model in one evaluation (Problem.eval_targets) beside the single-target
evaluation (Problem.eval), same process, same device: HOST WALL TIME of the blocking calls (as tools/latency.py: the host-side
argument copies and the result transfer are inside the figure, on both sides of the ratio), median of REPS after two
warm-ups, gradient and evidence-only, K in {1, 2, 4, 8, 16}; then the per-stage HIP-event times (timing level 2) of one K = 8
gradient evaluation.  A stage is not one kernel: "p1_targets" = the V^T diag(1/s) Y product, its partial-sum reduction and the
y^2 sums; "p2_targets" = the Q' B product and the row kernel; "p2_xcorr" = the X correction alone.  The rates derived from them
count only the n x m matrix each stage reads (and, for p2_xcorr, writes) and are therefore lower bounds of the kernels' own.
    usage (GPU box, repo root): timeout 600 python3 tools/bench_targets.py [n m d] [--out profiles/targets_c2.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpr_amd  # noqa: E402
from bench import synth  # noqa: E402

REPS = int(os.environ.get("REPS", 5))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out_path:
    args = [a for a in args if a != out_path]
n, m, d = (int(v) for v in args[:3]) if len(args) >= 3 else (1000000, 2048, 8)


def median_ms(f):
    ts = []
    for _ in range(REPS + 2):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts[2:]))


X, y, Z = synth(1, n, m, d)
rng = np.random.default_rng(2)
s = X.sum(0)
Y = np.asfortranarray(np.stack([np.sin((0.5 + 0.1 * k) * s + k) + (0.05 + 0.01 * k) * rng.normal(size=n) for k in range(16)], axis=1))
kw = dict(log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
p.set_inputs(X)
p.set_targets(y)
res = dict(n=n, m=m, d=d, reps=REPS, single=dict(
    grad_ms=median_ms(lambda: p.eval(**kw)), evidence_ms=median_ms(lambda: p.eval(want_grad=False, **kw))), targets={})
print("single target: gradient %.2f ms, evidence only %.2f ms" % (res["single"]["grad_ms"], res["single"]["evidence_ms"]), flush=True)
for K in (1, 2, 4, 8, 16):
    p.set_targets_many(Y[:, :K])
    g = median_ms(lambda: p.eval_targets(**kw))
    e = median_ms(lambda: p.eval_targets(want_grad=False, **kw))
    res["targets"][str(K)] = dict(grad_ms=g, evidence_ms=e, grad_ratio=g / res["single"]["grad_ms"],
                                  evidence_ratio=e / res["single"]["evidence_ms"])
    print("K = %2d: gradient %.2f ms (%.3f x single), evidence only %.2f ms (%.3f x)" % (
        K, g, g / res["single"]["grad_ms"], e, e / res["single"]["evidence_ms"]), flush=True)
p.set_targets_many(Y[:, :8])
p.set_timing(2)
p.eval_targets(**kw)
p.eval_targets(**kw)
st = p.last_timings()
nm8 = 8.0 * n * (-(-m // 128) * 128)
res["stages_ms_K8"] = {k: round(v, 3) for k, v in st.items()}
res["timing"] = "host wall time of the blocking call, median of %d after 2 warm-ups; stages: HIP events (level 2)" % REPS
res["stage_GBps_K8"] = {  # n x m bytes moved per stage: V once; Q' once; X read and written
    "p1_targets": nm8 / st["p1_targets"] / 1e6, "p2_targets": nm8 / st["p2_targets"] / 1e6, "p2_xcorr": 2 * nm8 / st["p2_xcorr"] / 1e6}
print("stages (K = 8, gradient):", res["stages_ms_K8"])
print("stages of the new kernels, GB/s of their n x m traffic:", {k: round(v) for k, v in res["stage_GBps_K8"].items()}, flush=True)
p.close()
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
