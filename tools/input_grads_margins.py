#!/usr/bin/env python3
"""Turns the GPR_MARGINS_LOG of one run of tests/test_input_grads_host.py and tests/test_gpu_input_grads.py into the table
profiles/input_grads_margins.txt: the worst |got - ref| / bound on the device per kernel instantiation and output
(tests/input_grads_ref.py), then case by case, and under their own heading the host file's worst ratios and the planted
defects' miss factors.

    GPR_MARGINS_LOG=host.jsonl python -m pytest tests/test_input_grads_host.py
    GPR_MARGINS_LOG=gpu.jsonl python -m pytest tests/test_gpu_input_grads.py
    python tools/input_grads_margins.py host.jsonl gpu.jsonl > profiles/input_grads_margins.txt
"""
import collections
import json
import sys


def main(paths):
    recs = [json.loads(line) for p in paths for line in open(p) if line.strip()]
    dev = collections.OrderedDict()
    host, defects, other = collections.defaultdict(float), [], []
    for r in recs:
        what, case = r["what"], r.get("case", "")
        if what.startswith("igrads."):
            key = (case, what[7:])
            if key not in dev or r["err"] > dev[key]["err"]:
                dev[key] = r
        elif what.startswith("host.igrads.defect.") or what.startswith("host.igrads.old_check_misses."):
            defects.append(r)
        elif what.startswith("host.igrads.restated."):
            host[what[21:]] = max(host[what[21:]], r["err"])
        else:
            other.append(r)
    print("# |got - ref| / bound (tests/input_grads_ref.py; u = 2^-53, C_E = 9, C_D = 16, C_M = 4): gprhip_predict_input_grad,")
    print("# gprhip_eval_input_grad and M (\"pg_m\") against the 80-bit contraction of the device's own t, U^-1, R~^-1, M and X.")
    print("# A ratio above 1 is a miss.  Worst ratio per kernel instantiation and output, and the case it occurred in:")
    worst = collections.OrderedDict()
    for (case, what), r in dev.items():
        if what not in worst or r["err"] > worst[what]["err"]:
            worst[what] = r
    for what in sorted(worst):
        r = worst[what]
        print("worst  %-34s %10.3g   %s%s" % (what, r["err"], r.get("case", ""), "   MISS" if r["err"] > r["tol"] else ""))
    print()
    print("# case by case.  scale: the largest reference entry; bound: the largest bound of the output.")
    print("%-58s %-30s %10s %10s %10s" % ("case", "output", "ratio", "scale", "bound"))
    for (case, what), r in dev.items():
        print("%-58s %-30s %10.3g %10.3g %10.3g%s" % (case, what, r["err"], r.get("scale", float("nan")), r.get("bound", r["tol"]),
                                                     "   MISS" if r["err"] > r["tol"] else ""))
    print()
    print("# ---- the CPU half (tests/test_input_grads_host.py) ----")
    print("# worst ratio of the float64 restatements over all cases and both summation orders, per path and output:")
    for k, v in sorted(host.items()):
        print("host   %-34s %10.3g" % (k, v))
    print("# planted defects: ratio by which the bound of the touched entry is missed (at least 100 asked); old_check_misses: the")
    print("# same defect on a far row, where the max-norm check at 1e-8 passes:")
    for r in defects:
        print("defect %-40s %-44s %10.3g" % (r["what"][12:], r.get("case", ""), r["err"]))
    print("# the references against tests/predict_grad_ref.py and tests/input_grad_ref.py, and the max-norm check on the planted rows:")
    agg = collections.defaultdict(float)
    for r in other:
        agg[(r["what"], r["tol"])] = max(agg[(r["what"], r["tol"])], r["err"])
    for (what, tol), v in sorted(agg.items()):
        print("%-40s %10.3g (asked %.0e)" % (what, v, tol))


if __name__ == "__main__":
    main(sys.argv[1:])
