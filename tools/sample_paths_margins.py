"""Table of the achieved errors of tests/test_gpu_sample_paths.py from the log of one run of the module:
    GPR_MARGINS_LOG=log.jsonl python3 -m pytest -m gpu tests/test_gpu_sample_paths.py
    python3 tools/sample_paths_margins.py log.jsonl > profiles/sample_paths_margins.txt
One line per quantity (the last component of the record's name): checks, the worst error, its bound, their ratio and where."""
import collections
import json
import sys

recs = [r for r in (json.loads(line) for line in open(sys.argv[1])) if r["what"].startswith("paths.")]  # (a log of the whole suite serves)
groups = collections.defaultdict(list)
for r in recs:
    parts = r["what"].split(".")
    key = ".".join(parts[1:3]) if parts[1] == "structure" else parts[-1]
    groups[key].append(r)
print("# worst achieved errors of tests/test_gpu_sample_paths.py on an MI355X (GPR_MARGINS_LOG of one run of the whole module, %d records)"
      % len(recs))
print("# error: largest absolute deviation over the largest absolute entry of the column (values: TOL_POST) or of the matrix of the")
print("# winners' gradients (dvalues: TOL_GRAD), against the 80-bit reference of tests/sample_paths_ref.py; no conditioning allowance")
print("%-28s %7s %12s %9s %8s   %s" % ("quantity", "checks", "worst", "bound", "ratio", "where"))
for key in sorted(groups):
    rs = groups[key]
    w = max(rs, key=lambda r: r["err"] / r["tol"])
    print("%-28s %7d %12.3e %9.0e %8.4f   %s (%s)" % (key, len(rs), w["err"], w["tol"], w["err"] / w["tol"], w["what"],
                                                    w["test"].split("::")[-1]))
