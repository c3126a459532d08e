"""profiles/refine_margins.txt from the GPR_MARGINS_LOG of a GPU run of tests/test_gpu_refine.py: per route (r1 the persistent
kernel, r2 the library-side loop, clamped the clamped-variance edge), criterion and output the worst achieved ratio of the
layer-A check of tests/test_gpu_acquire.py on the trace records, and how many calls had a trace bit for bit equal to
Problem.acquire at the traced points.
    usage: GPR_MARGINS_LOG=run.jsonl python3 -m pytest tests/test_gpu_refine.py -m gpu
           python3 tools/refine_margins.py run.jsonl [--out profiles/refine_margins.txt]
"""
import collections
import json
import sys

rows = [json.loads(ln) for ln in open(sys.argv[1])]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
worst, bits = collections.defaultdict(float), collections.Counter()
for r in rows:
    w = r["what"]
    if not w.startswith("refine."):
        continue
    route = w.split(".")[1]
    if w.endswith(".bitwise_acquire"):
        bits[(route, r["err"] == 0.0)] += 1
    else:
        key = (route, r.get("acq", "?"), w.rsplit(".", 1)[1], bool(r.get("proj", False)))
        worst[key] = max(worst[key], r["err"])
lines = ["# tools/refine_margins.py over the GPR_MARGINS_LOG of tests/test_gpu_refine.py on the MI355X: every trace record of",
         "# gprhip_acquire_refine held to the layer-A bounds of tests/test_gpu_acquire.py (c 2^-53 (1 + u^2); constants 40 / 35 / 30 / 8",
         "# for ei / log_ei / pi / bound) at the device's own posterior at the traced points.  r1: the persistent kernel, r2: the",
         "# library-side loop, clamped: the clamped-variance edge.  Worst achieved ratio c (proj=1: error over TOL_GRAD's scale):"]
for k in sorted(worst):
    lines.append("%-8s %-7s %-8s proj=%d worst %.4g" % (k[0], k[1], k[2], k[3], worst[k]))
lines.append("# calls whose trace equals Problem.acquire at the traced points bit for bit (the test asserts it):")
for k in sorted(bits):
    lines.append("%-8s bitwise_equal=%s calls %d" % (k[0], k[1], bits[k]))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
