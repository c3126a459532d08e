"""The CPU half of tests/test_gpu_sample_paths_pin.py: the 80-bit references of tests/sample_paths_pin_ref.py and their bounds
are pinned here, before any device is involved, on the oracle's own operands (tests/test_input_grads_host._oracle: t, U^-1 and
R~^-1 as float64 matrices, as a device would hold them):
  1. fed the 80-bit state of tests/sample_paths_ref.path_state and the oracle's K, the references reproduce
     sample_paths_from_state -- weights, paths, residuals, samples and gradients at chosen (r, j) -- to the rounding of its
     float64 outputs and of 80-bit sums (the oracle's K is a float64 matrix: it is put in the place of the reference's own K,
     so that the contraction is compared and not the exponential);
  2. float64 restatements of every kernel's arithmetic -- sp_tri_row's k-split and shuffle order for every cw, the shifted
     expansion under fmax, 16-column tiles with four partial sums, p~ rowsum - sum E z~, direct differences in blocks, both
     residual routes, the combination -- stay inside every bound (ratio <= 1) in two summation orders on the device cases;
     the worst ratio is printed and recorded;
     the host's centroid sum is restated and held against shift_of (the device's copy of the shift is not verified);
  3. the eight planted defects of the issue, each applied to the restatement, miss the bound of the entry they touch
     (ratio > 1; defect 8 is the padding predicate, not a ratio); for each the verdict of the max-norm check of
     tests/test_gpu_sample_paths.py (a column's largest deviation over its largest entry, TOL_POST values / TOL_GRAD gradients)
     is printed; defects 1, 2 and 8 pass it, and that follows from sizes asserted here.  The groups whose device ratio is below
     1e-3 of the bound are shown to separate with defects of their own: 3 and 7 on the 17 -> 16 projection (route 2 of the
     evaluator), and two defects on path_grad_at_kernel's direct form (9: a dropped column, 10: p for p~) at d = 3, at d = 1
     and with the 17 -> 16 projection.
"""
import math

import numpy as np
import pytest

from oracle import fitc_oracle as O
from tests import margins as M
from tests import sample_paths_pin_ref as S
from tests import sample_paths_ref as SR
from tests.test_gpu_input_grads import Case, data
from tests.test_gpu_sample_paths_pin import (BASE, EVAL, GRAD_AT, NS, NT, PATHS, RESID, SIGMA2, WEIGHTS, _iso, cw_of, draw_of, draws,
                                             geometry_at, ident, padding_is_zero, pin_points)
from tests.test_input_grads_host import _k64, _kernel, _oracle, _restate_grad, _sum_tiles
from tests.test_posterior_host import _matmul, _sum_lr, _sum_pw

TOL_GRAD, TOL_POST = 1e-8, 3e-10       # as tests/test_gpu_parity.py
LD = S.LD
U = S.U


def _ops(c):
    o = _oracle(c)
    return {k: o[k] for k in ("t", "uinv", "rinv")}


def _worst(what, r, label):
    M.record("host.sp_pin." + what, r, 1.0, case=label)
    print("%s %s: worst ratio %.3g" % (label, what, r))
    return r


# ---- 1. agreement with tests/sample_paths_ref.py --------------------------------------------------------------------------------
def _close(what, new, old, terms):
    """old: float64 outputs of 80-bit sums; terms: the sum of the absolute values behind an entry"""
    tol = 1.5 * U * np.abs(new) + 1e-17 * terms
    bad = np.abs(new - np.asarray(old, LD)) > tol
    assert not np.any(bad), (what, int(np.sum(bad)), float(np.max(np.abs(new - np.asarray(old, LD)))))


@pytest.mark.parametrize("c", [BASE, Case("iso", 64, 10, 3), Case("proj", 200, 65, 2, 5), Case("iso", 200, 40, 17)], ids=ident)
def test_the_references_reproduce_sample_paths_ref_on_its_own_state(c):
    X, y, Z, args = data(c)
    ok = _kernel(c, args)
    nt, ns = NT, 5
    Xt = pin_points(c, nt)[0]
    z, eps = draws(c, nt, ns)
    state = SR.path_state(ok, Z, X, y, SIGMA2)
    t, Ui, Ri = state
    A, eA = S.weights(t, Ui, Ri, z)
    _close("weights", A, SR.weights(state, z), np.abs(t)[:, None] + np.abs(Ui) @ (np.abs(Ri) @ np.abs(z).astype(LD)))
    at = [(r, j) for r in (0, 1, 2, 7, nt - 1) for j in (0, ns - 1)]
    old = SR.sample_paths_from_state(ok, Z, state, Xt, z, SIGMA2, eps=eps, predictive=True, grad_at=at)
    g = dict(geometry_at(c, Xt))
    g["K"] = np.asarray(O.spec_calc_shared_cross(ok, np.asfortranarray(Xt), np.asfortranarray(Z))[0], LD)
    aK, aA = np.abs(g["K"]), np.abs(A)
    F, _ = S.paths(g, A)
    _close("paths", F, old["paths"], aK @ aA)
    res, _ = S.resid(g, Ui, SIGMA2, small=True)
    res2, _ = S.resid(g, Ui, SIGMA2, small=False)
    assert np.array_equal(res, res2)          # the two routes differ in their bounds only
    k = ((g["K"] @ Ui) ** 2).sum(1)
    _close("resid", res, old["resid"], g["sf2"] + k + SIGMA2)
    mid, half = S.samples(F, 0 * F, res, 0 * res, eps)
    sd = np.sqrt(np.maximum(res, 0))[:, None] * np.abs(eps)
    _close("samples", F + np.sqrt(np.maximum(res, 0))[:, None] * eps, old["samples"], aK @ aA + sd)
    assert np.all(np.abs(mid - (F + np.sqrt(np.maximum(res, 0))[:, None] * eps)) <= half), "the interval holds its exact value"
    for direct in (True, False):
        dF, _ = S.path_grads(g, A, direct)
        new = np.stack([dF[j, r] for r, j in at], axis=1)
        lift = (lambda a: a) if g["tp"] is None else (lambda a: a @ np.abs(g["tp"]).T)
        size = np.stack([lift(g["ie2"] * S.G._amoment(g, aK * aA[:, j][None, :]))[r] for r, j in at], axis=1)
        _close("grads", new, old["grads"], size)
    # paths() is input_grads_ref.predict's "means" with t := a_j
    g0 = geometry_at(c, Xt)
    F0, eF0 = S.paths(g0, A)
    mu, emu = S.G.predict(g0, A[:, 1], 0.0, True)["means"]
    assert np.array_equal(F0[:, 1], mu) and np.allclose(np.asarray(eF0[:, 1], np.float64), emu, rtol=1e-14, atol=0)


# ---- 2. float64 restatements inside the bounds ----------------------------------------------------------------------------------
def _tri_rows(T, B, add, cw, split):
    """sp_tri_row in float64: out[i][j] = (add_i +) sum_{k >= i} T[i][k] B[k][j]; split: the k range over 64 / cw lanes, lane kq
    takes k = i + kq, i + kq + kg, ...; the lanes are added by the xor butterfly, lane 0 stores.  Else left to right."""
    m = T.shape[0]
    out = np.zeros_like(B)
    kg = 64 // cw
    for i in range(m):
        terms = T[i, i:][:, None] * B[i:]                                    # (n, ns)
        if split:
            lanes = np.zeros((kg, B.shape[1]))
            for kq in range(min(kg, m - i)):
                lanes[kq] = _sum_lr(terms[kq::kg].T)
            s = 1
            while s < kg:
                lanes = lanes + lanes[np.arange(kg) ^ s]
                s <<= 1
            acc = lanes[0]
        else:
            acc = _sum_lr(terms.T)
        out[i] = acc + add[i] if add is not None else acc
    return out


def restate_weights(ops, z, split):
    cw = cw_of(z.shape[1])
    w1 = _tri_rows(np.triu(ops["rinv"]), z, None, cw, split)
    return _tri_rows(np.triu(ops["uinv"]), w1, ops["t"], cw, split)


@pytest.mark.parametrize("c,nss", WEIGHTS, ids=ident)
def test_float64_weights_stay_inside_their_bound_for_every_split(c, nss):
    ops = _ops(c)
    worst = 0.0
    for ns in (64,) + tuple(nss):
        z, _ = draws(c, 17, ns)
        ref, bound = S.weights(ops["t"], ops["uinv"], ops["rinv"], z)
        for split in (True, False):
            r, at = S.ratio(restate_weights(ops, z, split), ref, bound)
            assert r <= 1.0, (ident(c), ns, split, r, at)
            worst = max(worst, r)
    _worst("restated.weights", worst, ident(c))


def restate_paths(c, Xt, A, order):
    X, y, Z, args = data(c)
    Ke = _k64(c, Xt, Z, args, True)[0]
    return np.stack([order(Ke * A[:, j][None, :]) for j in range(A.shape[1])], axis=1)


def restate_resid(c, Xt, uinv, add, small, order):
    X, y, Z, args = data(c)
    K = _k64(c, Xt, Z, args, small)[0]
    V = _matmul(K, np.triu(uinv), order)
    return (math.exp(args["log_sf2"]) - order(V * V)) + add


def restate_evaluator(c, x, A, dr, sign, order):
    X, y, Z, args = data(c)
    Ke, Pt, Zt, ie2 = _k64(c, x, Z, args, True)
    rs, g = _restate_grad(Ke * A[:, dr].T, Pt, Zt, ie2, order, args.get("tproj"), -sign)
    return sign * rs, g.T


def _sum_blocks64(terms):
    n = terms.shape[-1]
    acc = np.zeros(terms.shape[:-1])
    for lo in range(0, n, 64):
        for cc in range(lo, min(lo + 64, n)):
            acc = acc + terms[..., cc]
    return acc


def restate_grad_at(c, Xt, A, order, defect=None, row=0):
    """path_grad_at_kernel: direct differences of shifted coordinates, ns x nt x D.  defect, planted on one row: "column" --
    the column that weighs most in that row is not added; "unshifted" -- p in the place of p~ in the factor (p - z~)."""
    X, y, Z, args = data(c)
    tp = args.get("tproj")
    _, Pt, Zt, ie2 = _k64(c, Xt, Z, args, False)
    diff = Pt[:, None, :] - Zt[None, :, :]
    dist = _sum_lr(diff * diff)
    a = -0.5 * ie2
    K = np.exp(args["log_sf2"] + a * dist)
    fac = diff
    if defect == "unshifted":
        fac = diff.copy()
        fac[row] = fac[row] + S.shift_of(Z)[None, :]
    out = []
    for j in range(A.shape[1]):
        wv = K * A[:, j][None, :]
        if defect == "column":
            wv[row, int(np.argmax(np.abs(wv[row])))] = 0.0
        g = np.stack([order(wv * fac[:, :, k]) for k in range(diff.shape[2])], axis=-1) * (2.0 * a)
        if tp is not None:
            g = np.stack([_sum_lr(tp[b][None, :] * g) for b in range(tp.shape[0])], axis=-1)
        out.append(g)
    return np.stack(out)


@pytest.mark.parametrize("c,nt,ns", PATHS, ids=ident)
def test_float64_paths_stay_inside_their_bound(c, nt, ns):
    ops = _ops(c)
    Xt = pin_points(c, nt)[0]
    z, _ = draws(c, nt, ns)
    A = restate_weights(ops, z, True)
    F, eF = S.paths(geometry_at(c, Xt), A)
    worst = 0.0
    for order in (_sum_lr, _sum_tiles):
        r, at = S.ratio(restate_paths(c, Xt, A, order), F, eF)
        assert r <= 1.0, (ident(c), order.__name__, r, at)
        worst = max(worst, r)
    _worst("restated.paths", worst, "%s-nt%d-ns%d" % (ident(c), nt, ns))


@pytest.mark.parametrize("c,small", RESID, ids=ident)
def test_float64_samples_stay_inside_the_interval_on_both_residual_routes(c, small):
    ops = _ops(c)
    nt, ns = NT, 5
    Xt = pin_points(c, nt)[0]
    z, eps = draws(c, nt, ns)
    A = restate_weights(ops, z, True)
    g = geometry_at(c, Xt)
    F, eF = S.paths(g, A)
    worst = 0.0
    for add in (0.0, SIGMA2):
        res, e = S.resid(g, ops["uinv"], add, small)
        mid, half = S.samples(F, eF, res, e, eps)
        for order in (_sum_lr, _sum_tiles if small else _sum_pw):
            rd = restate_resid(c, Xt, ops["uinv"], add, small, order)
            r0, at = S.ratio(rd, res, e)
            got = restate_paths(c, Xt, A, order) + np.sqrt(np.maximum(rd, 0.0))[:, None] * eps
            r, at = S.ratio(got, mid, half)
            assert r0 <= 1.0 and r <= 1.0, (ident(c), add, order.__name__, r0, r, at)
            worst = max(worst, r)
    _worst("restated.samples.%s" % ("one_kernel" if small else "engine"), worst, ident(c))


@pytest.mark.parametrize("c", GRAD_AT, ids=ident)
def test_float64_direct_gradients_stay_inside_their_bound(c):
    ops = _ops(c)
    nt, ns = 64, 3
    Xt = pin_points(c, nt)[0]
    A = restate_weights(ops, draws(c, nt, ns)[0], True)
    dF, edF = S.path_grads(geometry_at(c, Xt), A, direct=True)
    worst = 0.0
    for order in (_sum_lr, _sum_blocks64):
        r, at = S.ratio(restate_grad_at(c, Xt, A, order), dF, edF)
        assert r <= 1.0, (ident(c), order.__name__, r, at)
        worst = max(worst, r)
    _worst("restated.grad_at", worst, ident(c))


@pytest.mark.parametrize("c,ns,nd,form", EVAL, ids=ident)
def test_float64_evaluator_stays_inside_its_bounds(c, ns, nd, form):
    ops = _ops(c)
    x = pin_points(c, ns)[0]
    A = restate_weights(ops, draws(c, ns, nd)[0], True)
    dr = draw_of(ns, nd, form)
    worst = 0.0
    for sign in (1.0, -1.0):
        ref = S.evaluator(geometry_at(c, x), A, dr, sign)
        for order in (_sum_lr, _sum_tiles):
            val, grad = restate_evaluator(c, x, A, dr, sign, order)
            rv, rg = S.ratio(val, *ref["values"])[0], S.ratio(grad, *ref["dvalues"])[0]
            assert rv <= 1.0 and rg <= 1.0, (ident(c), sign, order.__name__, rv, rg)
            worst = max(worst, rv, rg)
    _worst("restated.evaluator", worst, "%s-ns%d-nd%d-%s" % (ident(c), ns, nd, form))


@pytest.mark.parametrize("c", sorted(set([c for c, *_ in PATHS] + [c for c, *_ in EVAL] + GRAD_AT), key=ident), ids=ident)
def test_the_restated_host_centroid_against_shift_of(c):
    """The shift of the reference (input_grads_ref.shift_of, numpy's mean) against the sum the library forms on the host,
    restated in float64 (device_shift: left to right, one division).  Both sides are computed HERE: the copy the kernels read
    (p->zshift) has no fetch and is not verified.  The references do not depend on the shift; the bounds do through |p~|, |z~|,
    to which a difference of this size adds a relative 1e-13 at most."""
    X, y, Z, args = data(c)
    assert np.all(np.abs(S.device_shift(Z) - S.shift_of(Z)) <= 2 * S.shift_bound(Z)), ident(c)


# ---- 3. planted defects ---------------------------------------------------------------------------------------------------------
def old_check(got, ref):
    """the check of tests/test_gpu_sample_paths.py: per column (draw) the largest deviation over the largest entry; the worst"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return float(np.max(np.max(np.abs(got - ref), axis=0) / np.maximum(np.max(np.abs(ref), axis=0), 1e-300)))


def _verdict(n, what, entry_ratio, old, tol, must_pass, c=BASE, group="", predicate=False):
    """group: the device group (profiles/sample_paths_pin_margins.txt) whose bound the defect is held against; predicate: the
    entry check is a yes / no test, not a ratio (recorded as inf where it fails)"""
    seen = old > tol
    print("defect %d (%s) on %s [%s]: entry check %s; max-norm check %.3g against %.0e: %s" % (
        n, what, ident(c), group, "fails (a predicate, no ratio)" if predicate and entry_ratio > 1.0 else "ratio %.3g" % entry_ratio,
        old, tol, "sees it" if seen else "passes"))
    M.record("host.sp_pin.defect%d" % n, entry_ratio, 1.0, case=what, on=ident(c), group=group, predicate=bool(predicate),
             old_check=old, old_tol=tol, old_sees=bool(seen))
    assert entry_ratio > 1.0, (n, what, ident(c), entry_ratio)
    assert not (must_pass and seen), (n, what, old, tol)


# the groups whose worst device ratio is below 1e-3 (profiles/sample_paths_pin_margins.txt) get their own planted defects: the
# 17 -> 16 projection (grad_at.d16.proj, eval.r2.d16) and d = 1 (grad_at.d1)
PROJ16 = Case("proj", 200, 65, 16, 17)
LINE = _iso(65, 1)


def _group(c, kind):
    if kind == "eval":
        return "eval.r%d.d%d" % (2 if c.kind == "proj" else 1, c.d)
    return "grad_at.d%d%s" % (c.d, ".proj" if c.kind == "proj" else "")


def _defect_setup(c=BASE):
    ops = _ops(c)
    Xt = pin_points(c, NT)[0]
    z, eps = draws(c, NT, NS)
    g = geometry_at(c, Xt)
    A = restate_weights(ops, z, True)
    return c, ops, Xt, z, eps, g, A


def test_planted_defect_1_one_weight_of_a_column_far_from_every_test_point():
    c, ops, Xt, z, eps, g, A = _defect_setup()
    ref, bound = S.weights(ops["t"], ops["uinv"], ops["rinv"], z)
    F, eF = S.paths(g, A)
    # the column and draw whose term K_rc A_cj is smallest beside the draw's largest sample
    share = (np.max(np.abs(g["K"]), axis=0)[:, None] * np.abs(A) / np.max(np.abs(F), axis=0)[None, :]).astype(np.float64)
    cc, j = np.unravel_index(np.argmin(np.where(A != 0, share, np.inf)), share.shape)
    assert 1e-9 * share[cc, j] < 0.1 * TOL_POST, "no term of the case is small beside its draw's largest sample"   # the size argument
    bad = A.copy()
    bad[cc, j] *= 1.0 + 1e-9
    entry = S.ratio(bad, ref, bound)[0]
    old = old_check(restate_paths(c, Xt, bad, _sum_tiles), F)
    _verdict(1, "one weight times 1 + 1e-9", entry, old, TOL_POST, True)


def test_planted_defect_2_one_far_row_of_the_paths():
    c, ops, Xt, z, eps, g, A = _defect_setup()
    F, eF = S.paths(g, A)
    got = restate_paths(c, Xt, A, _sum_tiles)
    size = (np.max(np.abs(F), axis=1) / np.max(np.abs(F))).astype(np.float64)
    rows = [r for r in range(NT) if r % 3 == 1 and 0 < size[r] < 1e-4 and np.all(np.abs(F[r]) < 1e-4 * np.max(np.abs(F), axis=0))]
    assert rows, "no far row below 1e-4 of every draw's largest sample"              # the size argument: 1e-9 * 1e-4 << TOL_POST
    got[rows[0]] *= 1.0 + 1e-9
    _verdict(2, "one far row times 1 + 1e-9", S.ratio(got[rows[0]], F[rows[0]], eF[rows[0]])[0], old_check(got, F), TOL_POST, True)


@pytest.mark.parametrize("c", [BASE, PROJ16], ids=ident)
def test_planted_defect_3_one_row_of_the_evaluator_gathers_the_next_draw(c):
    c, ops, Xt, z, eps, g, A = _defect_setup(c)
    dr = draw_of(NT, NS, "round")
    ref = S.evaluator(g, A, dr, 1.0)
    bad = dr.copy()
    bad[5] = (bad[5] + 1) % NS
    val, grad = restate_evaluator(c, Xt, A, bad, 1.0, _sum_tiles)
    entry = min(S.ratio(val[5:6], ref["values"][0][5:6], ref["values"][1][5:6])[0],
                S.ratio(grad[:, 5], ref["dvalues"][0][:, 5], ref["dvalues"][1][:, 5])[0])
    # the old check groups a draw's records: the deviation of one start over the largest gradient entry of its draw
    same = dr == dr[5]
    old = float(np.max(np.abs(grad[:, 5] - ref["dvalues"][0][:, 5])) / np.max(np.abs(ref["dvalues"][0][:, same])))
    _verdict(3, "one row gathers draw j + 1", entry, old, TOL_GRAD, False, c, _group(c, "eval"))


def test_planted_defect_4_the_last_summand_of_one_row_of_the_weights_dropped():
    c, ops, Xt, z, eps, g, A = _defect_setup()
    ref, bound = S.weights(ops["t"], ops["uinv"], ops["rinv"], z)
    w1, _ = S.first_product(ops["rinv"], z)
    i = c.m - 2
    bad = A.copy()
    bad[i] = bad[i] - ops["uinv"][i, c.m - 1] * np.asarray(w1[c.m - 1], np.float64)
    _verdict(4, "last summand of a row dropped", S.ratio(bad[i], ref[i], bound[i])[0],
             old_check(restate_paths(c, Xt, bad, _sum_tiles), S.paths(g, A)[0]), TOL_POST, False)


def test_planted_defect_5_column_64_dropped_for_one_row():
    c, ops, Xt, z, eps, g, A = _defect_setup()
    assert c.m == 65
    F, eF = S.paths(g, A)
    got = restate_paths(c, Xt, A, _sum_tiles)
    r = int(np.argmax(np.asarray(g["K"][:, 64], np.float64)))
    got[r] = got[r] - np.asarray(g["K"][r, 64], np.float64) * A[64]
    _verdict(5, "column 64 dropped for one row", S.ratio(got[r], F[r], eF[r])[0], old_check(got, F), TOL_POST, False)


def test_planted_defect_6_sigma2_added_when_predictive_is_off():
    c, ops, Xt, z, eps, g, A = _defect_setup()
    F, eF = S.paths(g, A)
    res, e = S.resid(g, ops["uinv"], 0.0, False)
    mid, half = S.samples(F, eF, res, e, eps)
    rd = restate_resid(c, Xt, ops["uinv"], SIGMA2, False, _sum_pw)
    got = restate_paths(c, Xt, A, _sum_tiles) + np.sqrt(np.maximum(rd, 0.0))[:, None] * eps
    _verdict(6, "sigma2 added with predictive off", S.ratio(got, mid, half)[0], old_check(got, mid), TOL_POST, False)


@pytest.mark.parametrize("c", [BASE, PROJ16], ids=ident)
def test_planted_defect_7_p_in_the_place_of_the_shifted_p(c):
    c, ops, Xt, z, eps, g, A = _defect_setup(c)
    X, y, Z, args = data(c)
    dr = draw_of(NT, NS, "round")
    ref = S.evaluator(g, A, dr, 1.0)
    val, grad = restate_evaluator(c, Xt, A, dr, 1.0, _sum_tiles)
    # -inv_ell2 (p rowsum - acc): inv_ell2 s rowsum too much in the projected space, carried back by tproj where there is one
    extra = float(g["ie2"]) * S.shift_of(Z)
    if args.get("tproj") is not None:
        extra = args["tproj"] @ extra
    bad = grad - extra[:, None] * val[None, :]
    old = max(float(np.max(np.abs(bad[:, dr == j] - ref["dvalues"][0][:, dr == j])) / np.max(np.abs(ref["dvalues"][0][:, dr == j])))
              for j in range(NS))
    _verdict(7, "p for p~ in the gradient", S.ratio(bad, *ref["dvalues"])[0], old, TOL_GRAD, False, c, _group(c, "eval"))


def test_planted_defect_8_a_stale_entry_in_a_padded_column_of_the_weights():
    c, ops, Xt, z, eps, g, A = _defect_setup()
    mp = -(-c.m // 128) * 128
    full = np.zeros((mp, 64))
    full[:c.m, :NS] = A
    assert padding_is_zero(full, c.m, NS)
    full[3, NS] = 0.25                              # what a 64-draw call before this one would leave without the zeroing
    # the kernels stage columns below ns only (sample_paths.hip:120, path_refine.hip:85): no output changes -- the size argument
    F = S.paths(g, A)[0]
    old = old_check(restate_paths(c, Xt, full[:c.m, :NS], _sum_tiles), F)
    assert np.array_equal(full[:c.m, :NS], A) and old <= TOL_POST
    # the entry check here is a PREDICATE, the one tests/test_gpu_sample_paths_pin.check_weights asserts on the device's padded
    # block (every padded entry == 0.0); there is no bound and no ratio: inf stands for "fails"
    entry = float("inf") if not padding_is_zero(full, c.m, NS) else 0.0
    _verdict(8, "stale entry in a padded column", entry, old, TOL_POST, True, predicate=True)


@pytest.mark.parametrize("defect,n", [("column", 9), ("unshifted", 10)])
@pytest.mark.parametrize("c", [BASE, LINE, PROJ16], ids=ident)
def test_planted_defects_9_and_10_on_the_direct_gradient_of_a_draw(c, defect, n):
    """path_grad_at_kernel's bound (C_DIRECT) by itself, also where the device sits below 1e-3 of it: on the row with the largest
    gradient one column is not added (9), or p stands in the place of p~ in the factor p~ - z~ (10)"""
    ops = _ops(c)
    nt, ns = 64, 3
    Xt = pin_points(c, nt)[0]
    A = restate_weights(ops, draws(c, nt, ns)[0], True)
    dF, edF = S.path_grads(geometry_at(c, Xt), A, direct=True)
    row = int(np.argmax(np.max(np.abs(np.asarray(dF[0], np.float64)), axis=1)))
    assert S.ratio(restate_grad_at(c, Xt, A, _sum_blocks64)[:, row], dF[:, row], edF[:, row])[0] <= 1.0    # clean: inside
    got = restate_grad_at(c, Xt, A, _sum_blocks64, defect=defect, row=row)
    old = max(float(np.max(np.abs(got[j] - dF[j])) / np.max(np.abs(dF[j]))) for j in range(ns))
    what = "direct gradient: one column dropped" if defect == "column" else "direct gradient: p for p~ in the factor"
    _verdict(n, what, S.ratio(got[:, row], dF[:, row], edF[:, row])[0], old, TOL_GRAD, False, c, _group(c, "grad_at"))
