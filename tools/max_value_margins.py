"""profiles/max_value_margins.txt from the GPR_MARGINS_LOG of tests/test_max_value_host.py (the CPU grid that pins the
constants) and of a GPU run of tests/test_gpu_max_value.py: the worst achieved ratio per output on the CPU and per case on the
device, beside the constant it is held to.
    usage: GPR_MARGINS_LOG=cpu.jsonl python3 -m pytest tests/test_max_value_host.py
           GPR_MARGINS_LOG=gpu.jsonl python3 -m pytest tests/test_gpu_max_value.py -m gpu
           python3 tools/max_value_margins.py cpu.jsonl gpu.jsonl [--out profiles/max_value_margins.txt]
"""
import collections
import json
import sys

args = [a for a in sys.argv[1:]]
out_path = None
if "--out" in args:
    out_path = args[args.index("--out") + 1]
    del args[args.index("--out"):args.index("--out") + 2]
rows = [json.loads(ln) for path in args for ln in open(path)]
worst, tol = collections.defaultdict(float), {}
for r in rows:
    w = r["what"]
    if not w.startswith("mv."):
        continue
    worst[w] = max(worst[w], r["err"])
    tol[w] = r["tol"]
lines = ["# tools/max_value_margins.py: gprhip_acquire_max_value against mpmath at 50 digits (tests/max_value_ref.py).",
         "# mv.cpu.*: the point function on the host over the grid of tests/test_max_value_host.py -- the worst c in",
         "#   c 2^-53 (1 + gamma_max^2) per output; the constants (tol) are at most 10 x these.",
         "# every other line: the device at its own posterior -- .values: the worst c of the values (held to the CPU-pinned constant),",
         "#   .dvalues: the worst entry error of the gradient over its bound (4 2^-53 of the two products plus the coefficient bounds),",
         "#   .coefficients: c_mu, c_v recovered from a gradient row by least squares, worst error over the CPU-pinned coefficient",
         "#   bound with the entries' rounding carried through the recovery"]
for k in sorted(worst, key=lambda k: (not k.startswith("mv.cpu."), k)):
    lines.append("%-58s worst %-10.4g tol %g" % (k, worst[k], tol[k]))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
