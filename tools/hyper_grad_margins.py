#!/usr/bin/env python3
"""Turns the GPR_MARGINS_LOG of one run of tests/test_hyper_grad_host.py and tests/test_gpu_hyper_grad.py into the table
profiles/hyper_grad_margins.txt: per case and family the worst |g_dev - g_ref| / ((L + C) u A) on the device, the same ratio of
the float64 CPU restatements (the oracle's gradient; the device's form), L and C, and the oracle_* lines of the host file.

    GPR_MARGINS_LOG=host.jsonl python -m pytest tests/test_hyper_grad_host.py
    GPR_MARGINS_LOG=gpu.jsonl python -m pytest tests/test_gpu_hyper_grad.py
    python tools/hyper_grad_margins.py host.jsonl gpu.jsonl > profiles/hyper_grad_margins.txt
"""
import collections
import json
import sys


def main(paths):
    recs = [json.loads(line) for p in paths for line in open(p) if line.strip()]
    dev = collections.OrderedDict()
    host = collections.defaultdict(dict)
    oracle, power, head = [], [], collections.defaultdict(float)
    for r in recs:
        what, case = r["what"], r.get("case", "?")
        kind, _, fam = what.partition(".")
        if kind in ("dev", "chunks"):
            dev[(case, kind, fam)] = r
        elif kind.startswith("host_"):
            key = (case, fam)      # the host file labels a case by its host key (tests/test_gpu_hyper_grad.py::host_key)
            host[key][kind[5:]] = max(host[key].get(kind[5:], 0.0), r["err"])
        elif what.startswith("oracle_"):
            oracle.append(r)
        elif what.startswith("power_"):
            power.append(r)
        elif kind.startswith("headroom_"):
            head[kind[9:]] = max(head[kind[9:]], r["err"])
    print("# |g - g_ref| / ((L + C) u A) per case and family; u = 2^-53 (tests/hyper_grad_ref.py).  dev: the device; oracle64,")
    print("# raw64, shifted64: the oracle's float64 gradient and the float64 restatements of the device's forms on the oracle's")
    print("# operands (tests/test_hyper_grad_host.py).  A ratio above 1 is a miss.")
    print("%-58s %-10s %9s %4s %10s %10s %10s %10s" % ("case", "family", "L", "C", "dev", "oracle64", "raw64", "shifted64"))
    worst = 0.0
    for (case, kind, fam), r in dev.items():
        h = host.get((r.get("key"), fam), {})
        worst = max(worst, r["err"])
        f = lambda x: "%10.3g" % x if x is not None else "%10s" % "-"
        print("%-58s %-10s %9d %4d %s %s %s %s%s" % (case + ("" if kind == "dev" else " [chunks/2]"), fam, r["L"], r["C"], f(r["err"]),
                                                  f(h.get("oracle")), f(h.get("raw")), f(h.get("shifted", h.get("shifted_once"))),
                                                  "   MISS" if r["err"] > 1 else ""))
    print("# worst device ratio: %.3g" % worst)
    print("# worst host ratios: " + ", ".join("%s %.3g" % (k, max(v.get(k, 0.0) for v in host.values()))
                                              for k in ("oracle", "raw", "shifted", "shifted_once")))
    print("# headroom max A / max |g| over the inducing family: " + ", ".join("%s %.3g" % kv for kv in sorted(head.items())))
    print("# planted defects, ratio by which the bound is missed (at least 100 asked):")
    for r in power:
        print("power  %-40s %-12s %10.3g" % (r["case"], r["what"][6:], r["err"]))
    print("# the oracle's float64 gradient against the 80-bit reference, relative to the family's largest entry:")
    for r in oracle:
        print("%-18s %-44s %10.3g (asked %.0e)" % (r["what"], r["case"], r["err"], r["tol"]))


if __name__ == "__main__":
    main(sys.argv[1:])
