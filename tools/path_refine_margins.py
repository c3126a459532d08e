"""profiles/path_refine_margins.txt from the GPR_MARGINS_LOG of a GPU run of tests/test_gpu_path_refine.py: per route (r1 the
persistent kernel, r2 the library-side loop) and shape the worst achieved error of the traced values / gradients against the
80-bit reference, relative to the draw's largest entry, beside TOL_POST / TOL_GRAD; the z = 0 check against Problem.acquire;
and how many calls had values bit for bit equal to Problem.sample_paths at the traced points (recorded, not asserted).
    usage: GPR_MARGINS_LOG=run.jsonl python3 -m pytest tests/test_gpu_path_refine.py -m gpu
           python3 tools/path_refine_margins.py run.jsonl [--out profiles/path_refine_margins.txt]
"""
import collections
import json
import sys

rows = [json.loads(ln) for ln in open(sys.argv[1])]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
worst, tol, bits = collections.defaultdict(float), {}, collections.Counter()
for r in rows:
    w = r["what"]
    if not w.startswith("path_refine."):
        continue
    parts = w.split(".")
    if w.endswith(".bitwise_sample_paths"):
        bits[(parts[1], r["err"] == 0.0)] += 1
        continue
    key = (parts[1], parts[2] if parts[1] != "zero_z" else "m%d_d%d" % (r.get("m", 0), r.get("d", 0)), parts[-1])
    worst[key] = max(worst[key], r["err"])
    tol[key] = r["tol"]
lines = ["# tools/path_refine_margins.py over the GPR_MARGINS_LOG of tests/test_gpu_path_refine.py on the MI355X: every trace record of",
         "# gprhip_sample_paths_refine against the 80-bit reference at the traced point, largest error over the draw's largest entry;",
         "# worst over the draws and the four calls (maximise x scale) of a shape.  zero_z: z = 0 against Problem.acquire (bound, kappa 0)."]
for k in sorted(worst):
    lines.append("%-8s %-28s %-8s worst %.3e  bound %.0e" % (k[0], k[1], k[2], worst[k], tol[k]))
lines.append("# calls whose values equal Problem.sample_paths at the traced points bit for bit (not asserted: another summation order):")
for k in sorted(bits):
    lines.append("%-8s bitwise_equal=%s calls %d" % (k[0], k[1], bits[k]))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
