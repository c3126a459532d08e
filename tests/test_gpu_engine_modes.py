"""Every launch mode of the MFMA contraction engine the library issues, entry by entry: tools/engine_modes_check.hip
(build/engine_modes_check, linked against the production engine objects) per group and type.

Each case generates its operands on the host with every byte the launch must not read or write poisoned, launches through
launch_gemm, compares every entry with a long-double host reference of the full formula under the componentwise bound
(K + c) u S, compares everything outside the written set bit for bit, and asserts the plan (kernel, ipw, tail panels, desc2,
syrk, dslices) the case is named for.  DESIGN.md ("Engine launch modes") maps every launch_gemm site to its case; the
reference and bound code has a CPU self-test of its own (tests/test_engine_modes_ref.py)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_AB = [("+1", 0), ("-1", 1), ("+1", 1)]
_PLAIN = ["plain_%s_%s_a%s_b%d_ld16" % (op, sh, _AB[(i + j) % 3][0], _AB[(i + j) % 3][1])
          for i, op in enumerate(["nn", "nt", "tn"]) for j, sh in enumerate(["1x1", "2x3", "3x2"])]
_PLAIN += ["plain_nn_2x2_splitk3", "plain_refusals"]
_PLAIN64 = ["plain_cov_nt_384x384x256_a-1_b1", "plain_cov_nt_384x384x256_a+1_b1", "plain_cov_nt_384x384x256_a+1_b0",
            "plain_trailing_tn_upper_384_k128", "plain_panel_tn_inplace_128x384"]


def _tri(policies):
    # k-slices: single, 2, and what mxm_slices gives at that size (3 at 384, 4 at 512)
    ks = {128: [1, 2], 256: [1, 2], 384: [1, 2, 3], 512: [1, 2, 4]}
    return ["tri_%s_%d_ks%d" % (p, n, k) for p in policies for n in (128, 256, 384, 512) for k in ks[n]]


_BATCH = ["batch_join_%s_mp%d_w%d_nb%d_ks%d" % (j, mp, w, nb, ks)
          for mp, w, nb in [(512, 128, 2), (768, 128, 3), (768, 256, 1), (1024, 256, 2)] for ks in (1, 2)
          for j in ("a_khi_bn", "b_klo_bm")]
_SYRK = ["syrk_tn_w_upper_256_ks8", "syrk_tn_w_upper_256_ks16", "syrk_tn_w_upper_384_ks8", "syrk_tn_ws_upper_128_ks8",
         "syrk_tn_ws_upper_256_ks8", "syrk_tn_ws_upper_384_ks8", "syrk_tn_ws_upper_256_ks16", "syrk_tn_ws_upper_384_ks3"]
_EPI = ["epi_nt_xt_klo_bn_ldm16", "epi_nt_sx_two_phase_den0", "epi_nn_khi_bn_rp_sumsq", "epi_nn_khi_bn_rp_sumsq_dot"]
# (N = 512, two pairs per row panel, is the harness group `paired512`: its host reference takes 6 s, so it is run by hand)
_PAIRED = ["paired_nn_khi_bn_N256", "paired_nt_sx_two_phase_klo_bn_N256"]

CASES = {
    ("plain", "f64"): _PLAIN + _PLAIN64,
    ("plain", "f32"): _PLAIN,
    ("tri", "f64"): _tri(["khi_bn_nn", "klo_bn_nt", "klo_bm_nn", "klo_max_nt_upper", "band_nn_upper"]),
    ("tri", "f32"): _tri(["khi_bn_nn", "klo_bn_nt"]),  # the m x m products of triangular factors are fp64 in the library
    ("batch", "f64"): _BATCH,                             # ... and so are the joins of the triangular inverse
    ("epilogue", "f64"): _EPI,
    ("epilogue", "f32"): _EPI,
    ("syrk", "f64"): _SYRK,
    ("syrk", "f32"): _SYRK,
    ("paired", "f64"): _PAIRED,
    ("paired", "f32"): _PAIRED,
}


def _exe():
    exe = os.path.join(ROOT, "build", "engine_modes_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gpr_amd", "csrc"), "tools"], capture_output=True, timeout=900)
    assert os.path.exists(exe), "build/engine_modes_check not built (make -C gpr_amd/csrc tools)"
    return exe


@pytest.mark.parametrize("group,ty", sorted(CASES), ids=["%s-%s" % k for k in sorted(CASES)])
def test_engine_modes(group, ty):
    out = subprocess.run([_exe(), group, ty], capture_output=True, text=True, timeout=300)
    print(out.stdout[-6000:])
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-1000:])
    lines = {}
    for ln in out.stdout.splitlines():
        m = re.match(r"case (\S+) (f64|f32): (.*)$", ln)
        if m:
            assert m.group(2) == ty and m.group(1) not in lines, ln
            lines[m.group(1)] = m.group(3)
    assert sorted(lines) == sorted(CASES[(group, ty)]), (sorted(set(CASES[(group, ty)]) - set(lines)),
                                                        sorted(set(lines) - set(CASES[(group, ty)])))
    for name, rest in lines.items():
        assert rest.rstrip().endswith(" OK"), (name, rest)
        if name != "plain_refusals":
            assert " plan=ok" in rest and " bad=0 " in rest and " touched=0 " in rest, (name, rest)
            # a worst ratio of exactly 0 would mean exact arithmetic, i.e. operands that cannot show a rounding error
            worst = float(re.search(r"worst=(\S+)", rest).group(1))
            assert 0.0 < worst <= 1.0, (name, rest)
    tail = out.stdout.strip().splitlines()
    assert tail[-1] == "failed: 0" and tail[-2] == "cases: %d" % len(CASES[(group, ty)]), tail[-3:]
