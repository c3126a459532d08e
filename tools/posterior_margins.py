#!/usr/bin/env python3
"""Turns the GPR_MARGINS_LOG of one run of tests/test_posterior_host.py and tests/test_gpu_posterior.py into the table
profiles/posterior_margins.txt: per case and output the worst |got - ref| / bound on the device (tests/posterior_ref.py), and
under their own heading the host file's worst ratios, the size of each bound and the planted defects' miss factors.

    GPR_MARGINS_LOG=host.jsonl python -m pytest tests/test_posterior_host.py
    GPR_MARGINS_LOG=gpu.jsonl python -m pytest tests/test_gpu_posterior.py
    python tools/posterior_margins.py host.jsonl gpu.jsonl > profiles/posterior_margins.txt
"""
import collections
import json
import sys


def main(paths):
    recs = [json.loads(line) for p in paths for line in open(p) if line.strip()]
    dev = collections.OrderedDict()
    host, size, defects, other = collections.defaultdict(float), {}, [], []
    for r in recs:
        what, case = r["what"], r.get("case", "")
        if what.startswith("post."):
            key = (case, what[5:])
            if key not in dev or r["err"] > dev[key]["err"]:
                dev[key] = r
        elif what.startswith("host.defect."):
            defects.append(r)
        elif what.startswith("host.bound_over_scale."):
            size[(case, what[22:])] = r
        elif what.startswith("host.") and what.count(".") == 2:
            host[what[5:]] = max(host[what[5:]], r["err"])
        else:
            other.append(r)
    print("# |got - ref| / bound per case and output (tests/posterior_ref.py; u = 2^-53, C = 8): the device's posterior calls against")
    print("# the 80-bit contraction of its own t, U^-1, R~^-1.  A ratio above 1 is a miss.  scale: the largest reference entry;")
    print("# bound: the largest bound of the output.")
    print("%-62s %-22s %10s %10s %10s" % ("case", "output", "ratio", "scale", "bound"))
    worst = collections.defaultdict(float)
    for (case, what), r in dev.items():
        worst[what.split(".")[0]] = max(worst[what.split(".")[0]], r["err"] / r["tol"])
        print("%-62s %-22s %10.3g %10.3g %10.3g%s" % (case, what, r["err"], r.get("scale", float("nan")), r.get("bound", r["tol"]),
                                                     "   MISS" if r["err"] > r["tol"] else ""))
    print("# worst device ratio over its bound, per output: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    print()
    print("# ---- the CPU half (tests/test_posterior_host.py) ----")
    print("# worst ratio of the float64 / float32 restatements over all models, per output and summation order:")
    for k, v in sorted(host.items()):
        print("host   %-34s %10.3g" % (k, v))
    print("# planted defects: ratio by which the bound of the output is missed (at least 100 asked):")
    for r in defects:
        print("defect %-34s %-30s %10.3g" % (r["what"][12:], r.get("case", ""), r["err"]))
    print("# largest bound over the largest reference entry, and over sf2, per model and output (a record, not a condition):")
    for (case, what), r in sorted(size.items()):
        print("size   %-50s %-10s %10.3g %10.3g" % (case, what, r["err"], r["over_sf2"]))
    print("# the reference against the oracle (relative to the largest entry), and the gap test:")
    agg = collections.defaultdict(float)
    for r in other:
        agg[(r["what"], r["tol"])] = max(agg[(r["what"], r["tol"])], r["err"])
    for (what, tol), v in sorted(agg.items()):
        print("%-24s %10.3g (asked %.0e)" % (what, v, tol))


if __name__ == "__main__":
    main(sys.argv[1:])
