#!/usr/bin/env python3
"""Turns the GPR_MARGINS_LOG of one run of tests/test_sample_paths_pin_host.py and tests/test_gpu_sample_paths_pin.py into the
table profiles/sample_paths_pin_margins.txt: the worst |got - ref| / bound on the device per group (weights per cw and route,
paths per kernel instantiation, samples per residual route, the gradient at every row, the refinement evaluator per route), the
case it occurred in, and under their own heading the host file's worst restatement ratios and the planted defects.

    GPR_MARGINS_LOG=host.jsonl python -m pytest tests/test_sample_paths_pin_host.py
    GPR_MARGINS_LOG=gpu.jsonl python -m pytest tests/test_gpu_sample_paths_pin.py -m gpu
    python tools/sample_paths_pin_margins.py host.jsonl gpu.jsonl > profiles/sample_paths_pin_margins.txt
"""
import collections
import json
import sys


def main(paths):
    recs = [json.loads(line) for p in paths for line in open(p) if line.strip()]
    dev, count = {}, collections.Counter()
    host, defects = collections.defaultdict(float), []
    for r in recs:
        what = r["what"]
        if what.startswith("sp_pin."):
            count[what[7:]] += 1
            if what[7:] not in dev or r["err"] > dev[what[7:]]["err"]:
                dev[what[7:]] = r
        elif what.startswith("host.sp_pin.defect"):
            defects.append(r)
        elif what.startswith("host.sp_pin."):
            host[what[12:]] = max(host[what[12:]], r["err"])
    print("# |got - ref| / bound (tests/sample_paths_pin_ref.py; u = 2^-53, C_W = 2, C_E = 9, C_D = 16, C_DIRECT = 17): every entry of")
    print("# gprhip_sample_paths and gprhip_sample_paths_refine against the 80-bit contraction of the device's own t, U^-1, R~^-1 and")
    print("# weights (\"sp_a\").  A ratio above 1 is a miss.  Worst ratio per group, the checks behind it, and the case it occurred in:")
    print("%-34s %10s %7s   %s" % ("group", "ratio", "checks", "case"))
    for what in sorted(dev):
        r = dev[what]
        print("%-34s %10.3g %7d   %s%s" % (what, r["err"], count[what], r.get("case", ""),
                                           "   MISS" if r["err"] > r["tol"] else "   (loose: below 1e-3)" if r["err"] < 1e-3 else ""))
    fam = collections.defaultdict(float)
    for what, r in dev.items():
        fam[what.split(".")[0]] = max(fam[what.split(".")[0]], r["err"])
    print()
    print("# worst ratio per family:")
    for k in sorted(fam):
        print("family %-27s %10.3g%s" % (k, fam[k], "   (below 1e-3: the bound is loose here; see the planted defects)" if fam[k] < 1e-3 else ""))
    print()
    print("# ---- the CPU half (tests/test_sample_paths_pin_host.py) ----")
    print("# worst ratio of the float64 restatements over all cases and both summation orders:")
    for k, v in sorted(host.items()):
        print("host   %-34s %10.3g" % (k, v))
    print("# planted defects: the ratio by which the entry check is missed, and the max-norm check of tests/test_gpu_sample_paths.py")
    print("# (a column's largest deviation over its largest entry) beside its tolerance:")
    print("# (group: the device group above whose bound the defect is held against; defect 8 is a predicate -- every padded entry")
    print("# == 0.0 -- with no bound and no ratio: \"fails\")")
    for r in sorted(defects, key=lambda r: int(r["what"][18:])):
        entry = "     fails" if r.get("predicate") else "%10.3g" % r["err"]
        print("%-8s %-40s %-24s %-18s entry %s   max-norm %10.3g / %.0e  %s" % (
            r["what"][12:], r.get("case", ""), r.get("on", ""), r.get("group", ""), entry, r["old_check"], r["old_tol"],
            "sees it" if r["old_sees"] else "PASSES"))


if __name__ == "__main__":
    main(sys.argv[1:])
