"""The seeds of tests/test_gpu_path_refine.py's trace cases, checked on the CPU before the device sees them:
tests/refine_ref.py over the 80-bit evaluator of tests/path_refine_cases.py (longdouble weights, K a_j and its gradient; the
projection cases through tproj) with the cases' own boxes, scales, starts, draws and options, counting the records whose Armijo
inequality lies inside the band the GPU test may skip, 8 2^-53 (|a| + |a_y| + c1 sum |g_k delta_k|).  The GPU test allows 2 %
per shape; the seeds are kept where the reference stays at or below 1 %.
    usage (repo root, no GPU): python3 tools/path_refine_precheck.py [--out profiles/path_refine_precheck.txt]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import path_refine_cases as PC  # noqa: E402
from tests.test_gpu_refine import OPTS  # noqa: E402
from tests.test_path_refine_host import reference_ties  # noqa: E402

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
shapes = [(1, m, d, None, nd, ns, f) for m, d, nd, ns, f in PC.ROUTE_1] + [(2, m, d, D, nd, ns, f) for m, d, D, nd, ns, f in PC.ROUTE_2]
lines = ["# tools/path_refine_precheck.py: tests/refine_ref.py over the 80-bit evaluator on the trace cases of",
         "# tests/test_gpu_path_refine.py; ties: records whose Armijo inequality lies inside the band the GPU test may skip",
         "# (cap there: 2 % per shape; here: at most 1 %)",
         "%-6s %4s %3s %3s %3s %4s %-5s %8s %6s %7s" % ("route", "m", "d", "D", "nd", "ns", "form", "records", "ties", "share")]
worst = 0.0
for route, m, d, D, nd, ns, form in shapes:
    records, ties = reference_ties(PC.key_of(m, d, D), nd, ns, form, OPTS)
    share = 100.0 * ties / max(records, 1)
    worst = max(worst, share)
    lines.append("%-6d %4d %3d %3d %3d %4d %-5s %8d %6d %6.2f%%" % (route, m, d, D or d, nd, ns, form, records, ties, share))
    print(lines[-1], flush=True)
lines.append("# worst share %.2f%%" % worst)
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text)
sys.exit(0 if worst <= 1.0 else 1)
