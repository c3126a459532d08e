"""The seeds of tests/test_gpu_max_value_refine.py's trace cases, checked on the CPU before the device sees them:
tests/refine_ref.py over the 80-bit evaluator of tests/max_value_refine_cases.py (longdouble posterior, mpmath criterion) with
the cases' own boxes, scales, starts, extremes and options, counting the records whose Armijo inequality lies inside the band
the GPU test may skip, 8 2^-53 (|a| + |a_y| + c1 sum |g_k delta_k|).  The GPU test allows 2 % per shape.  Cov_se_iso shapes
only: the evaluator does not cover the projection case (m = 20, 5 -> 2), which is reported as not checked.
    usage (repo root, no GPU): python3 tools/max_value_refine_precheck.py [--out profiles/max_value_refine_precheck.txt]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import max_value_refine_cases as MC  # noqa: E402
from tests import refine_cases as RC  # noqa: E402
from tests import refine_ref as RR  # noqa: E402
from tests import test_gpu_max_value_refine as T  # noqa: E402

EPS = 2.0 ** -53
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
shapes = [(1, m, d, None, ns, S) for m, d, ns, S in T.ROUTE_1] + [(2, m, d, D, ns, S) for m, d, D, ns, S in T.ROUTE_2]
lines = ["# tools/max_value_refine_precheck.py: tests/refine_ref.py over the 80-bit evaluator on the trace cases of",
         "# tests/test_gpu_max_value_refine.py; ties: records whose Armijo inequality lies inside the band the GPU test may skip",
         "# (cap: 2 % per shape)",
         "%-6s %4s %3s %3s %-22s %8s %6s %7s" % ("route", "m", "d", "S", "ns", "records", "ties", "share")]
worst = 0.0
for route, m, d, D, ns_list, S in shapes:
    if D:
        lines.append("%-6d %4d %3d %3d %-22s not checked (projection: outside the CPU evaluator)" % (route, m, d, S, ns_list))
        continue
    X, y, Z, args = RC.data(m, d)
    post = RC.posterior(X, y, Z, args)
    lo, hi = MC.box(d)
    q = post(MC.box_points(lo, hi))
    ext = {mx: MC.extremes(q["means"], q["variances"], S, mx) for mx in (True, False)}
    opts = T.OPTS_64 if S == 64 else T.OPTS
    records = ties = 0
    for ci, (ns, maximise, scaled) in enumerate(T._calls(ns_list, S)):
        scale = np.linspace(0.5, 1.5, d) if scaled else None
        St = T.TR._starts(d, ns, lo, hi, 7 * ns + ci)
        f = MC.evaluator(post, ext[maximise], maximise)
        for i in range(ns):
            r = RR.refine(f, St[:, i], lo, hi, scale, **opts)
            x, g, a = (np.array(r["trace"][0][0]), np.array(r["trace"][0][1]), r["trace"][0][2])
            for yy, gy, ay, alpha, acc in r["trace"][1:]:
                delta = np.array(yy) - x
                records += 1
                band = 8 * EPS * (abs(a) + abs(ay) + opts["c1"] * float(np.sum(np.abs(g * delta))))
                ties += abs(ay - (a + opts["c1"] * float(np.dot(g, delta)))) < band
                if acc:
                    x, g, a = np.array(yy), np.array(gy), ay
    share = 100.0 * ties / max(records, 1)
    worst = max(worst, share)
    lines.append("%-6d %4d %3d %3d %-22s %8d %6d %6.2f%%" % (route, m, d, S, ns_list, records, ties, share))
    print(lines[-1], flush=True)
lines.append("# worst share %.2f %%: %s the cap of 2 %%" % (worst, "inside" if worst <= 2.0 else "BEYOND"))
text = "\n".join(lines) + "\n"
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text)
sys.exit(0 if worst <= 2.0 else 1)
