"""profiles/max_value_refine_margins.txt from the GPR_MARGINS_LOG of a GPU run of tests/test_gpu_max_value_refine.py: per route
(r1 the persistent kernel, r2 the library-side loop; clamped / far / observed: the edges) and output the worst achieved ratio
of tests/test_gpu_max_value.py's _hold on the trace records, and how many calls had a trace bit for bit equal to
Problem.acquire_max_value at the traced points.
    usage: GPR_MARGINS_LOG=run.jsonl python3 -m pytest tests/test_gpu_max_value_refine.py -m gpu
           python3 tools/max_value_refine_margins.py run.jsonl [--out profiles/max_value_refine_margins.txt]
"""
import collections
import json
import sys

rows = [json.loads(ln) for ln in open(sys.argv[1])]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
worst, tol, bits = collections.defaultdict(float), {}, collections.Counter()
for r in rows:
    w = r["what"]
    if not w.startswith("mvrefine."):
        continue
    parts = w.split(".")
    route = parts[1] if parts[1] in ("r1", "r2") else "%s (m = %s)" % (parts[1], r.get("m", "?"))
    if w.endswith(".bitwise_max_value"):
        bits[(route, r["err"] == 0.0)] += 1
    elif parts[-1] in ("values", "dvalues", "coefficients"):
        key = (route, parts[-1], bool(r.get("proj", False)))
        worst[key] = max(worst[key], r["err"])
        tol[key] = r["tol"]
lines = ["# tools/max_value_refine_margins.py over the GPR_MARGINS_LOG of tests/test_gpu_max_value_refine.py on the MI355X: every trace",
         "# record of gprhip_acquire_max_value_refine held to the bounds of tests/test_gpu_max_value.py (_hold: mpmath at the device's own",
         "# posterior at the traced points; values: the ratio c against C_a = 20 of tests/max_value_ref.py; dvalues and the recovered",
         "# coefficients: error over bound, at most 1).  r1: the persistent kernel, r2: the library-side loop.  Worst achieved:"]
for k in sorted(worst):
    lines.append("%-22s %-13s proj=%d worst %.4g (bound %g)" % (k[0], k[1], k[2], worst[k], tol[k]))
lines.append("# calls whose trace equals Problem.acquire_max_value at the traced points bit for bit (asserted on r2, where the same")
lines.append("# kernel binary runs; on r1 asserted if ROUTE_1_BITWISE of the test file is set, which needs it to hold in every call here):")
for k in sorted(bits):
    lines.append("%-22s bitwise_equal=%s calls %d" % (k[0], k[1], bits[k]))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
