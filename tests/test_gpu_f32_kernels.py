"""The covariance builders of the fp32-bulk mode entry by entry, and the mode end to end at the point widths the rest of the
suite never gives it.

1. K_nm of an fp32-bulk problem (debug_fetch_matrix("knm_rows"): chunk 0 rebuilt by cov_chunk<float>, widened) against the
   direct-difference cross covariance of the oracle (oracle/fitc_oracle.py, spec_calc_shared_cross: exp(log_sf2 +
   inv_ell2_05 * sum_k (p_k - z_k)^2), with diff (diff / ms) + log ms per dimension under multiscales) restated in numpy
   longdouble on the same fp64 operands -- for Cov_se_fat with a projection on the ORACLE's projection of the inputs.  The
   oracle's own fp64 matrix is held to the fp64 part of the bound against that evaluation, which ties the two together.

   u = 2^-53, u32 = 2^-24, gamma_k = k u / (1 - k u), a = inv_ell2_05, arg = log_sf2 + a * acc, every entry of K_ref:

   direct-difference kernels (cov_cross_kernel<DT, float>, cov_cross_wide_kernel<float>, cov_cross_ms_kernel<DT, float>):
       |K_dev - K_ref| <= 1.01 |K_ref| (u32 + 8 u (1 + |arg|) + |a| gamma_N T)
     T = sum_k (p_k - z_k)^2 and N = d + 3 (one rounding of the difference, counted twice in its square, one of the product
     or fused multiply-add, at most d additions); under multiscales T = sum_k (diff^2 / ms + |log ms|), N = 2 d + 5 (division,
     product, two additions per dimension, the logarithm to 2 ulp).  8 u (1 + |arg|) holds the product and the sum behind
     arg (2 u |arg| + u |log_sf2|, |log_sf2| <= 1 here) and exp_fast (1 ulp of libm's, itself 1 ulp: 4 u).

   matrix-core kernel (cov_cross_mfma_kernel<KS4, float>, 16 <= d <= 64 without multiscales; DP = 4 KS4 = 16, 32, 64):
       |K_dev - K_ref| <= 1.01 |K_ref| (u32 + 8 u (1 + |arg|) + |a| (gamma_{DP+3} + 2 u) A_rc),
       A_rc = sum_k (|p_rk - s_k| + |z_ck - s_k|)^2,   s = the centroid of the inducing points as the host sums it.
     The rounded shifts p - s, z - s move the distance by at most 2 u A_rc; the chains behind pn (DP fused multiply-adds),
     zn (KS4 of them and two lane additions) and S (DP products and additions inside the MFMA steps), the addition pn + zn
     and the final fused multiply-add are at most DP + 2 roundings on terms whose magnitudes sum to A_rc; fmax(., 0) only
     moves a negative result towards the true, non-negative distance.  THE OFFSET OF THE DATA APPEARS NOWHERE: s absorbs it.

   with a projection both add |a| 4 gamma_{D+3} sum_k |p_k - z_k| q_k, q = |tproj|^T |x|: the device's projection
   (project_mfma_kernel, D + 3 roundings at most) and the oracle's dgemm each within gamma_{D+3} q_k of the exact p_k.

   All the fp64 terms are some 1e-14 beside u32 = 6e-8: the asserted bound says "the fp32 rounding of a value good to fp64".
   Every sound builder reaches 0.98 ... 0.99 of it -- the rounding itself.  The fp64 value is therefore also checked THROUGH
   the rounding (outside_window): rounding is monotone, so the stored number lies in [fl32(K_ref (1 - e64)),
   fl32(K_ref (1 + e64))], e64 the bracket without u32 -- for all but a handful of entries the single number fl32(K_ref).
   The share of entries equal to fl32(K_ref) is recorded (profiles/f32_kernel_margins.txt) and asserted >= 99 % at offset 1e3.

2. End to end against the fp64 oracle at the stated bounds of the mode (TOL32_* of tests/test_gpu_parity.py) at
   d = 17 ... 100, Cov_se_fat with a projection and with multiscales, several chunks, and the two gradient-kernel variants.

The CPU halves (no mark) check the input conditions, the oracle against the 80-bit evaluation, and a numpy restatement of
the expansion -- the same shift, the same three sums, a float32 round -- against the asserted bound: they test the bound
and the power of the test (without the shift the restatement misses the bound at offset 1e5), not the kernel.
"""
import functools

import numpy as np
import pytest

import gpr_amd
from oracle import fitc_oracle as O
from tests import margins as M
from tests.util import synth

gpu = pytest.mark.gpu

LD = np.longdouble
U64 = 2.0 ** -53
U32 = 2.0 ** -24
SECOND_ORDER = 1.01
LOG_SF2 = 0.1
SIGMA2 = 0.2

# the stated bounds of the fp32-bulk mode, as tests/test_gpu_parity.py
TOL32_L = 1e-4
TOL32_DS2 = 8e-4
TOL32_GRAD = 5e-3
TOL32_COEFF = 5e-3


def gamma(k):
    return k * U64 / (1.0 - k * U64)


# ---- 1. K_nm entry by entry ------------------------------------------------------------------------------------------------
D_ALL = [15, 16, 17, 31, 32, 33, 63, 64, 65, 100]      # the direct kernel below 16; <4>, <8>, <16> at d = DP and d < DP; wide
M_ALL = [1, 16, 17, 33, 127, 128, 129, 200]            # 16-column tiles, 32-column wavefronts (live_c), one and two blocks
ROWS_ALL = [1, 63, 64, 65, 255, 256, 257, 300]         # RC = 64, SLAB = 256, the row < r1 / row < rows guards
M0, ROWS0 = 129, 300


def _knm_cases():
    """(kind, d, m, rows, offset); rows is the problem's n: chunk 0 is then the whole problem and every guard on a padded
    row is exercised by the evaluation and by the fetch alike."""
    out = [("iso", d, M0, ROWS0, 0.0) for d in D_ALL]
    for d in (17, 33):
        out += [("iso", d, m, ROWS0, 0.0) for m in M_ALL if m != M0]
        out += [("iso", d, M0, r, 0.0) for r in ROWS_ALL if r != ROWS0]
    out += [("fat_proj", d, M0, ROWS0, 0.0) for d in (17, 40, 64)]      # launch_project feeds the kernel, D = d + 3
    out += [("fat_ms", 8, M0, ROWS0, 0.0)]                              # cov_cross_ms_kernel<8, float>
    out += [("iso", d, M0, ROWS0, off) for off in (1e3, 1e5) for d in (17, 33, 64)]
    return out


KNM_CASES = _knm_cases()


def _case_id(c):
    return "%s_d%d_m%d_r%d%s" % (c[0], c[1], c[2], c[3], "_off%g" % c[4] if c[4] else "")


def padded_width(d):
    return 16 if d <= 16 else (32 if d <= 32 else 64)


def takes_matrix_cores(kind, d):
    """launch_cov_cross<float>: a shift, no multiscales, 16 <= d <= 64 (mp is always a multiple of 128)"""
    return kind != "fat_ms" and 16 <= d <= 64


def host_centroid(Z):
    """upload_hypers: the coordinates summed over the inducing points in their order, then divided by m"""
    s = np.zeros(Z.shape[0])
    for c in range(Z.shape[1]):
        s = s + Z[:, c]
    return s / Z.shape[1]


@functools.lru_cache(maxsize=None)
def _knm_data(case):
    """Unit-normal points (+ offset on every coordinate of inputs and inducing points alike); the inducing points are draws
    from the same cloud, the first half of them -- as far as there are inputs -- copies of inputs moved by 1 % of the spread,
    so that entries near sf2, where the expansion cancels completely, are there as well as entries of a few tenths."""
    kind, d, m, rows, offset = case
    rng = np.random.default_rng([d, m, rows, len(kind)])
    D = d + 3 if kind == "fat_proj" else d
    X = rng.normal(size=(D, rows))
    near = min(m // 2, rows)
    tproj = lms = None
    if kind == "fat_proj":
        tproj = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d))
        cloud = tproj.T @ np.concatenate([X[:, :near], rng.normal(size=(D, m - near))], axis=1)
        Z = cloud + (0.01 / np.sqrt(d)) * rng.normal(size=(d, m)) * (np.arange(m) < near)
    else:
        Z = np.concatenate([X[:, :near] + 0.01 * rng.normal(size=(d, near)), rng.normal(size=(d, m - near))], axis=1)
    if kind == "fat_ms":
        lms = np.asfortranarray(rng.uniform(-1.0, 1.0, size=(d, m)))
    X = np.asfortranarray(X + offset)
    Z = np.asfortranarray(Z + offset)
    y = np.sin(X.sum(0) - offset * D) + 0.1 * rng.normal(size=rows)
    if kind == "iso":
        ok = O.SeIsoKernel(0.5 * np.log(d) + 0.1, LOG_SF2)      # keeps K_ref between 1e-30 and 1e30 on unit-normal data
        args = dict(log_ell=ok.log_ell, log_sf2=LOG_SF2)
    else:
        ok = O.SeFatKernel(d, LOG_SF2, tproj, None, lms)
        args = dict(log_sf2=LOG_SF2)
        if tproj is not None:
            args["tproj"] = tproj
        if lms is not None:
            args["log_multiscales_m05"] = lms
    return X, y, Z, ok, args


def expansion_restatement(P, Z, s, a, log_sf2, DP, shifted=True):
    """cov_cross_mfma_kernel in fp64 numpy: P (d x rows), Z (d x m) -> rows x m, rounded to float32 and widened again.  The
    same shift, the three sums pn, zn, S over the d live dimensions (the padded ones add exact zeros), pn + zn - 2 S clamped
    at zero, one exp, one float32 round; products and additions round separately here (numpy has no fused multiply-add),
    which is one rounding more per term than the kernel and still inside gamma_{DP+3}.  shifted=False: s = 0."""
    d = P.shape[0]
    sh = s[:d] if shifted else np.zeros(d)
    ps = P - sh[:, None]
    zs = Z - sh[:, None]
    pn = np.zeros(P.shape[1])
    zn = np.zeros(Z.shape[1])
    S = np.zeros((P.shape[1], Z.shape[1]))
    for k in range(d):
        pn = pn + ps[k] * ps[k]
        zn = zn + zs[k] * zs[k]
        S = S + ps[k][:, None] * zs[k][None, :]
    dist = np.maximum((pn[:, None] + zn[None, :]) - 2.0 * S, 0.0)
    return np.exp(a * dist + log_sf2).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _knm_reference(case):
    """The CPU half of a case: K_ref in longdouble, both bounds entry by entry, fl32(K_ref), the restatement's operands.
    Asserts the conditions the bounds rest on."""
    kind, d, m, rows, offset = case
    X, y, Z, ok, args = _knm_data(case)
    iso = kind == "iso"
    a = ok.inv_ell2_05 if iso else -0.5
    pts = np.asarray(X if iso else O.se_fat_project(ok, X))       # (the oracle's projection: fp64 dgemm)
    ms = None if iso else ok.multiscales
    Pl, Zl = pts.astype(LD), np.asarray(Z).astype(LD)
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended type here"
    acc = np.zeros((rows, m), LD)
    T = np.zeros((rows, m), LD)
    for k in range(d):                                            # the oracle's loop: dimensions in increasing order
        diff = Pl[k][:, None] - Zl[k][None, :]
        if ms is None:
            acc += diff * diff
            T += diff * diff
        else:
            sc = ms[k].astype(LD)[None, :]
            acc += diff * (diff / sc) + np.log(sc)
            T += diff * (diff / sc) + np.abs(np.log(sc))
    arg = LD(ok.log_sf2) + LD(a) * acc
    K = np.exp(arg)
    # conditions on the inputs
    assert float(K.min()) >= 1e-30 and float(K.max()) <= 1e30, (case, float(K.min()), float(K.max()))
    assert abs(ok.log_sf2) <= 1.0
    s = host_centroid(np.asarray(Z))
    spread = float(np.std(pts - offset * iso))
    # the inducing points lie inside the cloud: their centroid within five spreads of the cloud's centre (the offset; m = 1
    # is a single draw), every point and every input within ten spreads of the centroid -- |p - s|, |z - s| then know
    # nothing of the offset
    assert np.max(np.abs(s - (offset if iso else 0.0))) <= 5.0 * spread, (case, s, spread)
    assert max(np.max(np.abs(pts - s[:, None])), np.max(np.abs(Z - s[:, None]))) <= 10.0 * spread, case
    absarg = np.abs(arg).astype(np.float64)
    aT = (abs(a) * T).astype(np.float64)
    common = U32 + 8.0 * U64 * (1.0 + absarg)
    if kind == "fat_proj":
        q = np.abs(ok.tproj).T @ np.abs(np.asarray(X))            # d x rows
        pz = np.zeros((rows, m))
        for k in range(d):
            pz += np.abs(pts[k][:, None] - Z[k][None, :]) * q[k][:, None]
        common = common + abs(a) * 4.0 * gamma(d + 3 + 3) * pz   # (D = d + 3)
    e_direct = common + gamma(2 * d + 5 if ms is not None else d + 3) * aT
    A = np.zeros((rows, m))
    for k in range(d):
        A += (np.abs(pts[k] - s[k])[:, None] + np.abs(Z[k] - s[k])[None, :]) ** 2
    e_mfma = common + abs(a) * (gamma(padded_width(d) + 3) + 2.0 * U64) * A
    Kabs = K.astype(np.float64)
    mfma = takes_matrix_cores(kind, d)
    # the oracle itself, in fp64, against this evaluation: within the fp64 part of the direct bound
    k_plain = ok if iso else O.SeFatKernel(d, ok.log_sf2, None, None, ok.log_multiscales_m05)
    K64, _ = O.spec_calc_shared_cross(k_plain, pts, Z)
    r64 = float(np.max(np.abs(K64.astype(LD) - K).astype(np.float64) / ((e_direct - U32) * Kabs)))
    assert r64 <= 1.0, (case, r64)
    def window(e):
        """[fl32(K_ref (1 - e64)), fl32(K_ref (1 + e64))], e64 = the fp64 part of the bracket with its factor 1.01"""
        e64 = (SECOND_ORDER * (e - U32)).astype(LD)
        return ((K * (1 - e64)).astype(np.float32).astype(np.float64), (K * (1 + e64)).astype(np.float32).astype(np.float64))

    return dict(K=K, K32=K.astype(np.float32).astype(np.float64), K64=np.asarray(K64),
                bound_direct=SECOND_ORDER * e_direct * Kabs, bound_mfma=SECOND_ORDER * e_mfma * Kabs,
                window_direct=window(e_direct), window_mfma=window(e_mfma),
                mfma=mfma, pts=pts, Z=np.asarray(Z), s=s, a=a, r64=r64)


def knm_figures(knm, ref):
    """(worst |knm - K_ref| / asserted bound, worst / direct bound, share of entries equal to fl32(K_ref))"""
    err = np.abs(knm.astype(LD) - ref["K"]).astype(np.float64)
    asserted = ref["bound_mfma"] if ref["mfma"] else ref["bound_direct"]
    return float(np.max(err / asserted)), float(np.max(err / ref["bound_direct"])), float(np.mean(knm == ref["K32"]))


def outside_window(knm, ref):
    """(entries outside the float32 window of the asserted bound, entries whose window holds more than one float32).
    Rounding is monotone: an fp64 value within e64 |K_ref| of K_ref rounds into [fl32(K_ref (1 - e64)), fl32(K_ref (1 + e64))].
    For all but a handful of entries the two ends coincide with fl32(K_ref), and the device must return exactly that
    number -- this is the bound of the fp64 value seen through the float32 store, some 1e-14 instead of 6e-8."""
    lo, hi = ref["window_mfma"] if ref["mfma"] else ref["window_direct"]
    return int(np.sum((knm < lo) | (knm > hi))), int(np.sum(lo != hi))


@pytest.mark.parametrize("case", KNM_CASES, ids=_case_id)
def test_bounds_and_input_conditions_hold_on_the_cpu(case):
    """No device.  The conditions on the inputs; the oracle's fp64 matrix inside the fp64 part of the bound, and rounded to
    float32 inside the direct bound and its window; where the matrix-core kernel runs, the restatement of its expansion
    inside the asserted bound and its window.  Offset cases: the restatement equals fl32(K_ref) on 99 % of the entries (what
    the device is asked at 1e3).  Without the shift it still reaches 99.8 % there and stays under the bound -- the count
    does not see a dropped shift at 1e3 -- but it leaves the window at 1e3 and misses the bound a hundredfold at 1e5: a
    kernel that drops the shift cannot pass either."""
    kind, d, m, rows, offset = case
    ref = _knm_reference(case)
    k64 = ref["K64"].astype(np.float32).astype(np.float64)
    r_a, r_d, eq = knm_figures(k64, dict(ref, mfma=False))
    assert r_d <= 1.0 and outside_window(k64, dict(ref, mfma=False))[0] == 0, (case, r_d)
    if not ref["mfma"]:
        return
    _, _, _, ok, _ = _knm_data(case)
    DP = padded_width(d)
    rest = expansion_restatement(ref["pts"], ref["Z"], ref["s"], ref["a"], ok.log_sf2, DP)
    r_a, r_d, eq = knm_figures(rest, ref)
    out, wide = outside_window(rest, ref)
    print("restatement %s: %.4f of the asserted bound, %.4f of the direct one, %.5f equal, %d outside the window (%d wider "
          "than one number)" % (_case_id(case), r_a, r_d, eq, out, wide))
    assert r_a <= 1.0 and out == 0, (case, r_a, out)
    if offset:
        assert eq >= 0.99, (case, eq)
        bare = expansion_restatement(ref["pts"], ref["Z"], ref["s"], ref["a"], ok.log_sf2, DP, shifted=False)
        u_a, u_d, ueq = knm_figures(bare, ref)
        u_out, _ = outside_window(bare, ref)
        print("  without the shift: %.4f of the asserted bound, %.5f equal, %d outside the window" % (u_a, ueq, u_out))
        assert u_out > 0 and ueq < eq, (case, u_out, ueq)
        if offset >= 1e5:
            assert u_a > 1.0, (case, u_a)


def _fetch_knm(case):
    kind, d, m, rows, offset = case
    X, y, Z, ok, args = _knm_data(case)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT, rows, X.shape[0], d, m,
                        precision=gpr_amd.F32_BULK)
    try:
        p.set_inputs(X)
        p.set_targets(y)
        ev = p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
        assert np.isfinite(ev.l)
        return p.debug_fetch_matrix("knm_rows", rows)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("case", KNM_CASES, ids=_case_id)
def test_knm_of_an_fp32_bulk_problem_entry_by_entry(case):
    """Every fetched row against K_ref.  d = 15, 65, 100 and the multiscale case are held to the direct bound, d = 16 ... 64
    to the matrix-core bound: a dispatch that sent d = 15 or 65 to the expansion, or the expansion to a width that drops
    coordinates, shows as a violation.  Offsets: the SAME bound -- it has no offset term.  A kernel without the shift carries
    offset^2 u |a| d of relative error in K: 4e-11 at 1e3, under the bound of 6e-8, so there the share of entries equal to
    fl32(K_ref) must be 99 % as well (the rest are entries whose fp64 value sits within a few ulp of a float32 rounding
    boundary); at 1e5 it is 4e-7 and exceeds the bound outright.  The restatement on the CPU shows that the count alone
    does not see a dropped shift at 1e3 (99.8 % without it), so every entry must also lie in the float32 window of the
    bound's fp64 part (outside_window): that fails without the shift at either offset."""
    kind, d, m, rows, offset = case
    ref = _knm_reference(case)          # (asserts the input conditions before the device is touched)
    knm = _fetch_knm(case)
    assert knm.shape == (rows, m) and np.all(np.isfinite(knm))
    assert np.array_equal(knm, knm.astype(np.float32).astype(np.float64))      # float32 storage, widened
    r_a, r_d, eq = knm_figures(knm, ref)
    out, wide = outside_window(knm, ref)
    out_d, _ = outside_window(knm, dict(ref, mfma=False))
    print("knm %s: %.4f of the asserted bound, %.4f of the direct bound, %.5f equal to fl32(K_ref), %d outside the window "
          "(%d of the direct bound's; %d windows wider than one number)" % (_case_id(case), r_a, r_d, eq, out, out_d, wide))
    M._record("knm_f32", r_a, 1.0, case=_case_id(case), kind=kind, d=d, m=m, rows=rows, offset=offset,
              builder="mfma" if ref["mfma"] else "direct", direct_ratio=r_d, equal=eq, oracle64=ref["r64"],
              outside=out, outside_direct=out_d, wide=wide, entries=int(knm.size))
    assert r_a <= 1.0, (case, r_a, r_d, eq)
    if offset == 1e3:
        assert eq >= 0.99, (case, eq)
    assert out == 0, (case, out, wide)


# ---- 2. end to end at the widths the mode has never run ----------------------------------------------------------------------
N_E2E, M_E2E = 1500, 140
# (kind, d, chunk_rows)
E2E_CASES = [("iso", d, 0) for d in (17, 33, 40, 64, 65, 100)] + [("fat_proj", 17, 0), ("fat_proj", 40, 0), ("fat_ms", 8, 0),
                                                                   ("iso", 33, 512)]


def _e2e_id(c):
    return "%s_d%d%s" % (c[0], c[1], "_chunk%d" % c[2] if c[2] else "")


@functools.lru_cache(maxsize=None)
def _e2e_case(kind, d):
    """(X, y, Z, Problem.eval arguments, gradient families, the fp64 oracle's evaluation)"""
    n, m = N_E2E, M_E2E
    if kind == "iso":
        X, y, Z = synth(600 + d, n, m, d)
        ok = O.SeIsoKernel(0.5 * np.log(d), LOG_SF2)
        args = dict(log_ell=ok.log_ell, log_sf2=LOG_SF2)
        fams = M.families("iso", d, m)
    elif kind == "fat_proj":
        rng = np.random.default_rng(700 + d)
        D = d + 3
        X = np.asfortranarray(rng.normal(size=(D, n)))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d))
        ok = O.SeFatKernel(d, LOG_SF2, P)
        Z = np.asfortranarray(O.se_fat_project(ok, X[:, :m]) + 0.01 * rng.normal(size=(d, m)))
        args = dict(log_sf2=LOG_SF2, tproj=P)
        fams = M.families("fat", d, m, D=D, proj=True)
    else:
        X, y, Z = synth(800 + d, n, m, d)
        X, Z = np.asfortranarray(X / np.sqrt(d)), np.asfortranarray(Z / np.sqrt(d))     # unit length scales: the points carry it
        lms = np.asfortranarray(np.random.default_rng(d).uniform(-1.0, 1.0, size=(d, m)))
        ok = O.SeFatKernel(d, LOG_SF2, None, None, lms)
        args = dict(log_sf2=LOG_SF2, log_multiscales_m05=lms)
        fams = M.families("fat", d, m, ms=True)
    return X, y, Z, args, fams, O.evaluate_fast(ok, Z, X, y, SIGMA2)


def _eval_f32(kind, d, chunk_rows=0, want_repeat=False):
    X, y, Z, args, fams, ref = _e2e_case(kind, d)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT, N_E2E, X.shape[0], d, M_E2E,
                        chunk_rows=chunk_rows, precision=gpr_amd.F32_BULK)
    try:
        p.set_inputs(X)
        p.set_targets(y)
        ev = p.eval(sigma2=SIGMA2, inducing=Z, **args)
        cond = p.condition()[0]
        ev0 = p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **args) if want_repeat else None
    finally:
        p.close()
    return ev, ev0, cond


def _within_the_stated_bounds(ev, cond, kind, d):
    X, y, Z, args, fams, ref = _e2e_case(kind, d)
    assert ev.grad.shape == ref["grad"].shape
    assert M.rel_ok("l", ev.l, ref["l"], TOL32_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL32_DS2)
    assert M.grad_ok(ev.grad, ref["grad"], fams, TOL32_GRAD, cond=cond, unit=M.EPS32)
    assert M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL32_COEFF)


@gpu
@pytest.mark.parametrize("case", E2E_CASES, ids=_e2e_id)
def test_fp32_bulk_end_to_end_at_unvisited_widths(case):
    """Evidence, dl/dsigma2, the gradient family by family (Proj and multiscale families included) and the mean coefficients
    against the fp64 oracle inside the stated bounds of the mode: the <16, float> covariance builder and the wide and
    multiscale ones with float storage, the gradient tiles of those widths with TS = float, and three chunks through the
    builder (chunk_rows = 512).  An evidence-only evaluation on the same hypers gives the same l bit for bit."""
    kind, d, chunk_rows = case
    M.note(case=_e2e_id(case), kind=kind, d=d, n=N_E2E, m=M_E2E, chunk_rows=chunk_rows)
    ev, ev0, cond = _eval_f32(kind, d, chunk_rows, want_repeat=True)
    M.note(_reset=False, cond=cond)
    _within_the_stated_bounds(ev, cond, kind, d)
    assert ev0.l == ev.l


@gpu
@pytest.mark.parametrize("switch", ["GPRHIP_GRAD_SCALAR=1", "GPRHIP_K_RESIDENT=0"])
def test_fp32_bulk_gradient_kernel_variants(switch, monkeypatch):
    """Cov_se_fat with a projection at d = 17 through the scalar gradient kernel and through the matrix-core kernel that
    recomputes K_nm instead of reading the kept copy (both read when the problem is created): the same oracle bounds, the same
    l as the default.  No variant-to-variant gradient tolerance is asserted; the differences are recorded."""
    kind, d = "fat_proj", 17
    X, y, Z, args, fams, ref = _e2e_case(kind, d)
    a, _, cond_a = _eval_f32(kind, d)
    name, value = switch.split("=")
    monkeypatch.setenv(name, value)
    b, _, cond_b = _eval_f32(kind, d)
    M.note(case=switch, kind=kind, d=d, n=N_E2E, m=M_E2E, cond=cond_b)
    _within_the_stated_bounds(a, cond_a, kind, d)
    _within_the_stated_bounds(b, cond_b, kind, d)
    assert a.l == b.l
    for fam, e in M.family_errors(b.grad, a.grad, fams).items():
        M._record("variant_grad." + fam, e, float("nan"))
    M._record("variant_dl_dsigma2", abs(b.dl_dsigma2 - a.dl_dsigma2) / abs(a.dl_dsigma2), float("nan"))
    M._record("variant_coeffs", M.relinf(b.coeffs, a.coeffs), float("nan"))
