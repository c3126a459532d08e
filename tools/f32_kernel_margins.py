"""profiles/f32_kernel_margins.txt from the log of one run of tests/test_gpu_f32_kernels.py:

    GPR_MARGINS_LOG=log.jsonl python -m pytest tests/test_gpu_f32_kernels.py -m gpu
    python tools/f32_kernel_margins.py log.jsonl "<one line about the run>" > profiles/f32_kernel_margins.txt
"""
import json
import sys


def main(path, header):
    recs = [json.loads(line) for line in open(path)]
    knm = [r for r in recs if r["what"] == "knm_f32"]
    print("# tests/test_gpu_f32_kernels.py, %s" % header)
    print("# K_nm of an fp32-bulk problem (all rows x m entries of debug_fetch_matrix(\"knm_rows\")) against the direct-difference")
    print("# cross covariance in 80-bit arithmetic.  asserted = worst |K_dev - K_ref| / bound of the builder that serves the width")
    print("# (matrix-core expansion for 16 <= d <= 64 without multiscales, else direct differences); direct = the same against the")
    print("# tighter direct-difference bound; both bounds are 1.01 (2^-24 + fp64 terms of some 1e-14) |K_ref|, so the worst entry of")
    print("# ANY sound builder sits just under 1 -- the float32 rounding.  What tells the builders apart is the fp64 value seen")
    print("# through that rounding: equal = share of entries equal to fl32(K_ref); outside = entries outside the float32 window")
    print("# [fl32(K_ref (1 - e64)), fl32(K_ref (1 + e64))] of the asserted bound's fp64 part e64 (asserted: 0), out_dir = outside")
    print("# the window of the direct bound's; wide = entries whose window holds more than one float32; oracle64 = the oracle's own")
    print("# fp64 matrix against the 80-bit one, as a share of the direct bound's fp64 part.")
    print()
    print("%-34s %-7s %8s %8s %9s %8s %8s %5s %8s %9s" % ("case", "builder", "entries", "asserted", "direct", "equal", "outside",
                                                       "wide", "out_dir", "oracle64"))
    for r in knm:
        print("%-34s %-7s %8d %8.4f %9.4f %8.5f %8d %5d %8d %9.4f" % (
            r["case"], r["builder"], r["entries"], r["err"], r["direct_ratio"], r["equal"], r["outside"], r["wide"],
            r["outside_direct"], r["oracle64"]))
    print()
    for b in ("direct", "mfma"):
        sel = [r for r in knm if r["builder"] == b]
        if sel:
            w = max(sel, key=lambda r: r["direct_ratio"])
            print("# %-6s %2d cases: worst %.4f of the asserted bound, %.4f of the direct bound (%s); least share equal %.5f; "
                  "%d entries in all outside the direct bound's window" % (
                      b, len(sel), max(r["err"] for r in sel), w["direct_ratio"], w["case"], min(r["equal"] for r in sel),
                      sum(r["outside_direct"] for r in sel)))
    print()
    print("# end to end against the fp64 oracle (n = 1500, m = 140): error beside its bound; gradient families relative to the")
    print("# family's largest entry, beyond the conditioning allowance 8 cond 2^-24 of the vector's largest")
    e2e = [r for r in recs if r["what"] != "knm_f32" and not r["what"].startswith("variant_")]
    tests = []
    for r in e2e:
        key = (r["test"], r.get("case"))
        if key not in tests:
            tests.append(key)
    for key in tests:
        rows = [r for r in e2e if (r["test"], r.get("case")) == key]
        cond = rows[-1].get("cond")
        print("%s  cond %s" % (key[0].split("::")[-1], "%.2e" % cond if cond else "?"))
        seen = {}
        for r in rows:
            seen.setdefault(r["what"], []).append(r)
        for what, rr in seen.items():
            raw = "   before the allowance %s" % "  ".join("%.2e" % r["raw"] for r in rr) if "raw" in rr[0] else ""
            print("    %-18s %s   bound %.1e%s" % (what, "  ".join("%.2e" % r["err"] for r in rr), rr[0]["tol"], raw))
    print()
    print("# gradient-kernel variants against the default evaluation of the same problem (Cov_se_fat, projection, d = 17): recorded,")
    print("# not asserted (l is asserted bit for bit)")
    for r in recs:
        if r["what"].startswith("variant_"):
            print("    %-22s %-28s %.3e" % (r.get("case", "?"), r["what"], r["err"]))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "one run on an MI355X with GPR_MARGINS_LOG set")
