"""gprhip_eval_input_grad on the device: the gradient of the log evidence with respect to the training inputs against the
oracle-based reference of tests/input_grad_ref.py (the oracle's own X and K_nm, direct differences in numpy longdouble; pinned
against central differences of the oracle's evidence by tests/test_input_grad_host.py), on every row path and kernel width,
across chunks, with offset inputs, against the merged `Proj gradient, the contract of the entry point, and the torch front end.

Bound: the largest absolute deviation over the n x D matrix, divided by the largest absolute entry of the reference matrix, is at
most BOUND = TOL_GRAD of tests/test_gpu_parity.py (1e-8) -- the project's fp64 bound for a family of the gradient, the one the
inducing-point family is held to -- measured, recorded and asserted by tests/margins.py's check_vec (exactly this ratio).
NO conditioning allowance is applied: the cases are built so that cond(K_m + jitter I) <= 1e6, computed with numpy.linalg.eigvalsh from the oracle's matrix and asserted (the rule
tests/test_gpu_factors.py uses for R).  Every achieved ratio is recorded (GPR_MARGINS_LOG -> profiles/input_grad_margins.txt)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from oracle import fitc_oracle as O
from tests import margins as M
from tests.input_grad_ref import input_grad_from_parts
from tests.test_gpu_parity import TOL_GRAD
from tests.util import cond_of, oracle_km_full, synth, taken

gpu = pytest.mark.gpu
BOUND = TOL_GRAD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND_MAX = 1e6
SIGMA2 = 0.1
ENGINE_ENV = {"GPRHIP_SMALL_PATH": "0", "GPRHIP_MID_PATH": "0"}

PAIRS = [(1, 1), (15, 3), (64, 10), (65, 64), (200, 65), (333, 128), (200, 129), (500, 256), (300, 257), (700, 300)]
PAIRS_ONE_KERNEL = [p for p in PAIRS if p[1] <= 256]     # the shapes small.hip / mid.hip take
# every instantiation of input_grad_kernel<KS4, DT, KR> that launch_input_grad dispatches to (d = 3 is run by the other tests):
# K recomputed <1,1> d = 1 | <2,1> d = 8 | <4,1> d = 15, 16 | <8,2> d = 17 | <16,4> d = 64;  K read, one launch per block of 64
# dimensions: d = 65 -> blocks of 64 and 1 (<0,4>, <0,1>), d = 88 -> 64 and 24 (<0,4>, <0,2>); PROJ_DIMS below reaches the
# read-K kernels through the resident store as well ((30, 24): <0,2>; d = 2 .. 16: <0,1>; D = 70: the rebuilt chunk)
ISO_DIMS = [1, 8, 15, 16, 17, 64, 65, 88]
PAIRS_WIDE = [(64, 10), (200, 129)]
PROJ_DIMS = [(5, 2), (17, 16), (40, 3), (70, 4), (30, 24)]
PAIRS_PROJ = [(64, 10), (200, 129), (700, 300)]


@functools.lru_cache(maxsize=None)
def _case(kind, n, m, d, D=0, het=False, offset=0.0):
    """Inputs (D x n), targets, inducing points (d x m), Problem.eval arguments, the oracle's kernel, cond(K_m + jitter I).
    kind: "iso", "fat" (no projection; D = d) or "proj" (Cov_se_fat with a D x d projection).  The length scale is the largest
    of sqrt(d) 0.8^k at which the condition number is at most 1e5; Cov_se_fat has unit length scales, there the points carry it.
    offset: added to every coordinate of the inputs and the inducing points (iso / fat)."""
    X, y, Z = synth(4000 + 7 * m + d, max(n, m), m, d)
    X, y = np.asfortranarray(X[:, :n]), y[:n].copy()
    rng = np.random.default_rng(100 + m + d)
    hetv = rng.uniform(-7.0, -4.0, size=m) if het else None
    tproj = None
    if kind == "proj":
        Q, _ = np.linalg.qr(rng.normal(size=(D, d)))
        A = np.eye(d) + 0.1 * rng.uniform(-1.0, 1.0, size=(d, d))
        off = rng.normal(size=(D, n))
        X = np.asfortranarray(Q @ X + (off - Q @ (Q.T @ off)))
        tproj = Q @ A
        Z = np.asfortranarray(A.T @ Z)
    ell = float(np.sqrt(d))
    for _ in range(60):
        if kind == "iso":
            ok, Zs = O.SeIsoKernel(float(np.log(ell)), 0.0), np.asfortranarray(Z + offset)
        else:
            tp = None if tproj is None else np.asfortranarray(tproj / ell)
            ok, Zs = O.SeFatKernel(d, 0.0, tp, hetv), np.asfortranarray(Z / ell + offset)
        cond = cond_of(oracle_km_full(ok, Zs) + O.CHOLESKY_JITTER * np.eye(m))
        if cond <= 1e5:
            break
        ell *= 0.8
    assert cond <= 1e5, (kind, n, m, d, ell, cond)
    if kind == "iso":
        args = dict(log_ell=float(np.log(ell)), log_sf2=0.0)
        Xs = np.asfortranarray(X + offset)
    else:
        args = dict(log_sf2=0.0)
        if hetv is not None:
            args["log_hetero_skedasticity"] = hetv
        if tproj is not None:   # the projection carries the scale: the inputs stay as they are
            args["tproj"] = ok.tproj
            Xs = X
        else:
            Xs = np.asfortranarray(X / ell + offset)
    return Xs, y, Zs, args, ok, cond


@functools.lru_cache(maxsize=None)
def _parts(key, variational):
    Xs, y, Zs, args, ok, cond = _case(*key)
    assert cond <= COND_MAX, (key, cond)
    # (hypers=[]: the oracle's own gradient loop over 2 + d m hypers is not needed here)
    return O.evaluate(ok, Zs, Xs, y, SIGMA2, variational=variational, hypers=[], keep=True)


@functools.lru_cache(maxsize=None)
def _reference(key, variational=False, model_only=False):
    Xs, y, Zs, args, ok, cond = _case(*key)
    ref = input_grad_from_parts(ok, Zs, Xs, _parts(key, variational), model_only)
    ref.setflags(write=False)
    return ref


def _problem(key, chunk_rows=0):
    Xs, y, Zs, args, ok, cond = _case(*key)
    kind = key[0]
    D, n = Xs.shape
    d, m = Zs.shape
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT, n, D, d, m, chunk_rows=chunk_rows)
    p.set_inputs(Xs)
    p.set_targets(y)
    return p


def _eval_args(key, **kw):
    Xs, y, Zs, args, ok, cond = _case(*key)
    out = dict(sigma2=SIGMA2, inducing=Zs, **args)
    out.update(kw)
    return out


def _within_bound(what, got, ref, **extra):
    """Largest absolute deviation over the largest absolute reference entry: printed, then recorded and asserted by
    tests/margins.py (check_vec without a conditioning allowance)."""
    print("%s: %.3e of the largest entry (bound %.0e)" % (what, M.relinf(got, ref), BOUND))
    M.note(_reset=False, **extra)
    return M.check_vec(what, got, ref, BOUND)


def _check(key, what, variational=False, model_only=False, chunk_rows=0, path=None):
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind=key[0], n=key[1], m=key[2], d=key[3], D=Xs.shape[0])
    ref = _reference(key, variational, model_only)
    p = _problem(key, chunk_rows)
    try:
        p.set_timing(2)
        ev, g = p.eval_input_grad(**_eval_args(key, variational=variational, model_only=model_only))
        stages = p.last_timings()
        assert "p2_xgrad" in stages
        if path is not None:
            assert taken(stages) == path, (taken(stages), path)
        assert g.shape == ref.shape and np.all(np.isfinite(g))
        _within_bound(what, g, ref, path=taken(stages))
        return g
    finally:
        p.close()


def _path_of(m):
    return "small" if m <= 64 else ("mid" if m <= 256 else "engine")


# ---- 1. against the oracle, every path and width ---------------------------------------------------------------------------
def _objective_of(n):
    """With ONE training point the standard FITC evidence does not depend on that point at all: the diagonal correction makes
    the model's variance of y exactly sf2 + sigma2 wherever x lies, so dl/dx = 0 identically and the oracle's X is what is left
    of O(1) terms after cancellation (3e-16 against an exact 4e-19 for the case below) -- there is no largest entry to be
    relative to.  The variational objective has the trace term -(sf2 - q) / (2 sigma2), which does depend on x: the pair
    n = 1, m = 1 is compared against the oracle under that objective, and the standard one is held to its exact value, zero
    (test_one_training_point_has_no_input_gradient_under_the_standard_objective)."""
    return dict(variational=(n == 1))


@gpu
@pytest.mark.parametrize("n,m", PAIRS)
def test_iso_d3_against_the_oracle(n, m):
    _check(("iso", n, m, 3), "xgrad.iso", path=_path_of(m), **_objective_of(n))


@gpu
@pytest.mark.parametrize("model_only", [False, True])
def test_one_training_point_has_no_input_gradient_under_the_standard_objective(model_only):
    """n = 1, m = 1, standard FITC: the exact gradient is zero (see _objective_of).  Bound: BOUND times the size of the sum the
    zero is made of -- inv_ell2 sum_c T_rc K_rc |p_rk - z_ck| with T_rc = |X0_rc| + |U_rc v_r| + |w_r t_c|, the magnitudes of the
    three terms of X (lib/fitc_gp.ml:1204-1206) from the oracle."""
    key = ("iso", 1, 1, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    parts = _parts(key, False)
    u_mat, x0 = O.calc_us_mat(parts["model"])
    tr = parts["trained"]
    v = O.cm_calc_v1_vec(parts["cm"]) if model_only else tr["v_vec"]
    T = np.abs(x0) + np.abs(u_mat * v[:, None])
    if not model_only:
        T = T + np.abs(np.outer(tr["w_vec"], tr["coeffs"]))
    scale = ok.inv_ell2 * np.max((T * parts["shared"]["knm"]) @ np.abs(Xs[:, :1] - Zs).T)
    p = _problem(key)
    try:
        _, g = p.eval_input_grad(**_eval_args(key, model_only=model_only))
        assert np.all(np.isfinite(g))
        M.check_rel("xgrad.iso_one_point_zero", np.max(np.abs(g)), 0.0, BOUND, floor=scale)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("d", ISO_DIMS)
def test_iso_every_kernel_width(d, n, m):
    _check(("iso", n, m, d), "xgrad.iso_d%d" % d)


@gpu
@pytest.mark.parametrize("n,m", PAIRS)
def test_fat_without_projection(n, m):
    _check(("fat", n, m, 3, 3), "xgrad.fat", path=_path_of(m), **_objective_of(n))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_PROJ)
@pytest.mark.parametrize("D,d", PROJ_DIMS)
def test_fat_with_projection(D, d, n, m):
    _check(("proj", n, m, d, D), "xgrad.proj_%d_%d" % (D, d))


@gpu
def test_heteroskedastic_noise():
    _check(("proj", 200, 65, 2, 5, True), "xgrad.proj_het")


@gpu
@pytest.mark.parametrize("n,m", [(64, 10), (200, 129), (700, 300)])
@pytest.mark.parametrize("variational,model_only", [(True, False), (False, True), (True, True)])
def test_variational_and_model_only(variational, model_only, n, m):
    _check(("iso", n, m, 3), "xgrad.iso_%s_%s" % ("var" if variational else "std", "model" if model_only else "trained"),
           variational=variational, model_only=model_only, path=_path_of(m))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_ONE_KERNEL)
def test_engine_branch_on_the_small_and_mid_shapes(monkeypatch, n, m):
    for k_, v_ in ENGINE_ENV.items():
        monkeypatch.setenv(k_, v_)
    _check(("iso", n, m, 3), "xgrad.iso_engine", path="engine", **_objective_of(n))


@gpu
@pytest.mark.parametrize("n,m", [(64, 10), (200, 129)])
def test_engine_branch_with_a_projection_on_the_small_and_mid_shapes(monkeypatch, n, m):
    for k_, v_ in ENGINE_ENV.items():
        monkeypatch.setenv(k_, v_)
    _check(("proj", n, m, 2, 5), "xgrad.proj_engine", path="engine")


@gpu
@pytest.mark.parametrize("resident", ["0", None])
def test_k_read_and_k_recomputed_agree_with_the_oracle(monkeypatch, resident):
    """Cov_se_fat with a projection on the engine path: K_nm read from the resident store (the default) or recomputed"""
    if resident is not None:
        monkeypatch.setenv("GPRHIP_K_RESIDENT", resident)
    _check(("proj", 700, 300, 2, 5), "xgrad.proj_k_%s" % ("recomputed" if resident == "0" else "resident"), path="engine")


@gpu
def test_hyper_gradient_kernel_choice_does_not_matter(monkeypatch):
    a = _check(("iso", 700, 300, 3), "xgrad.iso")
    monkeypatch.setenv("GPRHIP_GRAD_SCALAR", "1")
    b = _check(("iso", 700, 300, 3), "xgrad.iso_grad_scalar")
    assert np.array_equal(a, b)


# ---- 2. several chunks --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m", [10, 200, 300])
def test_several_chunks_equal_one(m):
    """n = 300 in chunks of 128 rows (m = 10 and m = 200: shapes of the one-kernel passes, sent to the engine row path for this
    call) against the single-chunk evaluation of the same problem, rows at the seams and the ragged last chunk explicitly"""
    key = ("iso", 300, m, 3)
    one = _check(key, "xgrad.iso_one_chunk", path=_path_of(m))
    many = _check(key, "xgrad.iso_chunks", chunk_rows=128, path="engine")
    # (each group of rows against ITS OWN largest entry: no weaker than against the matrix's)
    for rows, name in ((slice(126, 130), "first seam"), (slice(254, 258), "second seam"), (slice(256, 300), "ragged last chunk"),
                       (slice(0, 300), "all rows")):
        _within_bound("xgrad.chunks_vs_one", many[:, rows], one[:, rows], rows=name)


# ---- 3. offset inputs ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", [3, 17])
@pytest.mark.parametrize("n,m", [(64, 10), (700, 300)])
def test_inputs_far_from_the_origin(d, n, m):
    """Inputs and inducing points shifted by 1e5, distances O(1): the bound is the same, the reference uses direct differences"""
    _check(("iso", n, m, d, 0, False, 1e5), "xgrad.iso_offset_d%d" % d)


# ---- 4. consistency with the `Proj gradient -------------------------------------------------------------------------------------
@gpu
def test_consistent_with_the_projection_gradient():
    """Problem A: Cov_se_fat, D = 6, d = 3 with tproj through gprhip_eval.  Problem B: Cov_se_fat without projection on
    P = tproj^T X, the same inducing points, through gprhip_eval_input_grad.  X_big (dl/dP)^T is A's `Proj block.  No oracle."""
    key = ("proj", 200, 20, 3, 6)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    d, m = Zs.shape
    a = _problem(key)
    b = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, d, d, m)
    try:
        eva = a.eval(**_eval_args(key))
        proj = eva.grad[1 + d * m: 1 + d * m + D * d].reshape(D, d)   # big-major
        P = np.asfortranarray(np.asarray(args["tproj"]).T @ Xs)
        b.set_inputs(P)
        b.set_targets(y)
        evb, g = b.eval_input_grad(sigma2=SIGMA2, inducing=Zs, log_sf2=args["log_sf2"])
        got = Xs @ g.T
        _within_bound("xgrad.vs_proj_gradient", got, proj)
        assert abs(evb.l - eva.l) <= 1e-12 * abs(eva.l)
    finally:
        a.close()
        b.close()


# ---- 5. contract --------------------------------------------------------------------------------------------------------------
def _same_evaluation(a, b):
    return (a.l1 == b.l1 and a.l2 == b.l2 and a.l == b.l and a.dl_dsigma2 == b.dl_dsigma2 and np.array_equal(a.grad, b.grad)
            and np.array_equal(a.coeffs, b.coeffs))


@gpu
@pytest.mark.parametrize("n,m", [(64, 10), (200, 129), (700, 300)])
def test_results_are_those_of_eval_bit_for_bit_and_runs_repeat(n, m):
    key = ("iso", n, m, 3)
    p, q = _problem(key), _problem(key)
    try:
        ev0 = q.eval(**_eval_args(key))
        ev1, g1 = p.eval_input_grad(**_eval_args(key))
        ev2, g2 = p.eval_input_grad(**_eval_args(key))
        assert _same_evaluation(ev0, ev1) and _same_evaluation(ev0, ev2)
        assert np.array_equal(g1, g2)
        Xt = np.asfortranarray(_case(*key)[0][:, :7] + 0.05)
        for u, v in zip(p.predict(Xt), q.predict(Xt)):
            assert np.array_equal(u, v)
    finally:
        p.close()
        q.close()


@gpu
def test_host_and_device_outputs_agree_and_padding_rows_stay():
    import torch
    key = ("proj", 200, 65, 2, 5)
    D, n = _case(*key)[0].shape
    p = _problem(key)
    try:
        _, g = p.eval_input_grad(**_eval_args(key))
        out = torch.full((n, D), float("nan"), dtype=torch.float64, device="cuda:0")
        _, none = p.eval_input_grad(out_device_ptr=out.data_ptr(), **_eval_args(key))
        assert none is None
        assert np.array_equal(out.cpu().numpy().T, g)
        _, wide = p.eval_input_grad(ld=D + 3, **_eval_args(key))
        assert wide.shape == (D + 3, n) and np.array_equal(wide[:D], g) and np.all(np.isnan(wide[D:]))
    finally:
        p.close()


@gpu
def test_reuse_v_after_a_change_of_sigma2():
    key = ("iso", 200, 129, 3)
    p, q = _problem(key), _problem(key)
    try:
        p.eval_input_grad(**_eval_args(key))
        _, g = p.eval_input_grad(**_eval_args(key, sigma2=0.25, reuse_v=True))
        _, fresh = q.eval_input_grad(**_eval_args(key, sigma2=0.25))
        _within_bound("xgrad.reuse_v", g, fresh)
    finally:
        p.close()
        q.close()


def _raw(p, hyp, ptr, ld, on_device):
    h, keep = p._hypers(hyp.get("log_ell", 0.0), hyp["log_sf2"], hyp["sigma2"], hyp["inducing"], hyp.get("tproj"), False, False,
                        1e-6, hyp.get("log_hetero_skedasticity"), hyp.get("log_multiscales_m05"), False)
    res = _lib.Result()
    grad = np.zeros(p.n_hypers(hyp.get("tproj") is not None, False, hyp.get("log_multiscales_m05") is not None) + 1)
    coeffs = np.zeros(p.m)
    dp = ctypes.POINTER(ctypes.c_double)
    return p._lib.gprhip_eval_input_grad(p._handle(), ctypes.byref(h), ctypes.byref(res), grad.ctypes.data_as(dp),
                                         coeffs.ctypes.data_as(dp), ctypes.c_void_p(ptr), ld, on_device)


@gpu
def test_refusals_leave_the_problem_as_it_was():
    import torch
    key = ("fat", 64, 10, 3, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    hyp = _eval_args(key)
    fresh = _problem(key)
    p = _problem(key)
    f32 = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, Zs.shape[1], precision=gpr_amd.F32_BULK)
    empty = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, Zs.shape[1])
    try:
        want = fresh.eval(**hyp)
        p.set_timing(2)
        buf = np.full((D, n), np.nan, order="F")
        dev = torch.zeros((n, D), dtype=torch.float64, device="cuda:0")
        lms = np.zeros((D, Zs.shape[1]), order="F")
        assert _raw(p, hyp, None, D, 0) == _lib.EBADARG                                   # dl_dinputs == NULL
        assert _raw(p, hyp, buf.ctypes.data, D - 1, 0) == _lib.EBADARG                    # host: ld < D
        assert _raw(p, hyp, dev.data_ptr(), D + 1, 1) == _lib.EBADARG                     # device: ld != D
        assert _raw(p, dict(hyp, log_multiscales_m05=lms), buf.ctypes.data, D, 0) == _lib.EBADARG
        assert _raw(p, dict(hyp, sigma2=-1.0), buf.ctypes.data, D, 0) == _lib.EBADARG
        f32.set_inputs(Xs)
        f32.set_targets(y)
        assert _raw(f32, hyp, buf.ctypes.data, D, 0) == _lib.EBADARG                      # fp32-bulk problem
        assert _raw(empty, hyp, buf.ctypes.data, D, 0) == _lib.ESTATE                     # no inputs / targets
        assert np.all(np.isnan(buf)) and not dev.any()
        assert p.last_timings() == {}                                                     # nothing was enqueued
        assert _same_evaluation(p.eval(**hyp), want)
        assert "p2_xgrad" not in p.last_timings()                                         # gprhip_eval does not run the step
        ev, g = p.eval_input_grad(**hyp)
        assert _same_evaluation(ev, want) and "p2_xgrad" in p.last_timings()
    finally:
        for q in (fresh, p, f32, empty):
            q.close()


# ---- 6. torch front end -----------------------------------------------------------------------------------------------------
@gpu
def test_torch_front_end():
    import torch
    from gpr_amd.autograd import log_evidence
    key = ("iso", 200, 20, 4)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    d, m = Zs.shape
    dev = torch.device("cuda:0")
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, D, d, m)
    q = _problem(key)
    try:
        ev, g = q.eval_input_grad(**_eval_args(key))
        x = torch.tensor(np.ascontiguousarray(Xs.T), device=dev, requires_grad=True)
        yt = torch.tensor(y, device=dev)
        lsf = torch.tensor(args["log_sf2"], dtype=torch.float64, requires_grad=True)
        lell = torch.tensor(args["log_ell"], dtype=torch.float64, requires_grad=True)
        ls2 = torch.tensor(float(np.log(SIGMA2)), dtype=torch.float64, requires_grad=True)
        z = torch.tensor(np.ascontiguousarray(Zs.T), requires_grad=True)
        l = log_evidence(p, x, yt, log_sf2=lsf, log_sigma2=ls2, inducing=z, log_ell=lell)
        assert l.dim() == 0 and l.dtype == torch.float64
        l.backward()
        # (sigma2 = exp(log(0.1)) differs from 0.1 in the last place at most: the comparison evaluation takes the same value)
        ev, g = q.eval_input_grad(**_eval_args(key, sigma2=float(np.exp(float(ls2.detach())))))
        assert float(l.detach()) == ev.l
        assert np.array_equal(x.grad.cpu().numpy().T, g)
        assert float(lell.grad) == ev.grad[0] and float(lsf.grad) == ev.grad[1]
        assert np.array_equal(z.grad.numpy(), ev.grad[2:].reshape(m, d))
        assert float(ls2.grad) == ev.dl_dsigma2 * float(np.exp(float(ls2.detach())))
        # a linear feature map in front: dl/dA = inputs0^T dl/dinputs
        x0 = torch.tensor(np.ascontiguousarray(Xs.T), device=dev)
        A = torch.eye(D, dtype=torch.float64, device=dev, requires_grad=True)
        l2 = log_evidence(p, (x0 @ A).contiguous(), yt, log_sf2=args["log_sf2"], log_sigma2=float(ls2.detach()), inducing=z.detach(),
                          log_ell=args["log_ell"])
        l2.backward()
        want = (Xs.astype(np.longdouble) @ g.T.astype(np.longdouble)).astype(np.float64)  # (the reference's own sum in 80 bits)
        err_a = float(np.max(np.abs(A.grad.cpu().numpy() - want)) / np.max(np.abs(want)))
        print("A.grad against inputs0^T dl_dinputs: %.3e" % err_a)
        assert err_a <= 1e-14, err_a
        # nothing requires grad: an evidence-only evaluation
        p.set_timing(2)
        l3 = log_evidence(p, x0, yt, log_sf2=args["log_sf2"], log_sigma2=float(ls2.detach()), inducing=z.detach(), log_ell=args["log_ell"])
        assert float(l3) == ev.l or abs(float(l3) - ev.l) <= 1e-12 * abs(ev.l)
        stages = p.last_timings()
        assert stages and not [s for s in stages if s.startswith("p2_")], stages
    finally:
        p.close()
        q.close()


@gpu
def test_torch_front_end_with_a_projection_and_host_targets():
    """Cov_se_fat with tproj (the `Proj slice of the gradient vector), targets given as a host tensor"""
    import torch
    from gpr_amd.autograd import log_evidence
    key = ("proj", 200, 20, 2, 5)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    d, m = Zs.shape
    dev = torch.device("cuda:0")
    p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, d, m)
    q = _problem(key)
    try:
        s2 = float(np.exp(np.log(SIGMA2)))
        ev, g = q.eval_input_grad(**_eval_args(key, sigma2=s2))
        x = torch.tensor(np.ascontiguousarray(Xs.T), device=dev, requires_grad=True)
        tp = torch.tensor(np.ascontiguousarray(args["tproj"]), requires_grad=True)
        z = torch.tensor(np.ascontiguousarray(Zs.T), device=dev, requires_grad=True)
        lsf = torch.tensor(args["log_sf2"], dtype=torch.float64, requires_grad=True)
        l = log_evidence(p, x, torch.tensor(y), log_sf2=lsf, log_sigma2=float(np.log(SIGMA2)), inducing=z, tproj=tp)
        l.backward()
        assert float(l.detach()) == ev.l
        assert np.array_equal(x.grad.cpu().numpy().T, g)
        assert float(lsf.grad) == ev.grad[0]
        assert np.array_equal(z.grad.cpu().numpy(), ev.grad[1:1 + d * m].reshape(m, d))
        assert np.array_equal(tp.grad.numpy(), ev.grad[1 + d * m:1 + d * m + D * d].reshape(D, d))
        # the stored gradients are numbers: a second derivative is refused, not returned as zero
        x2 = torch.tensor(np.ascontiguousarray(Xs.T), device=dev, requires_grad=True)
        l2 = log_evidence(p, x2, torch.tensor(y), log_sf2=args["log_sf2"], log_sigma2=float(np.log(SIGMA2)), inducing=z.detach(),
                          tproj=tp.detach())
        (gx2,) = torch.autograd.grad(l2, x2, create_graph=True)
        with pytest.raises(RuntimeError):
            gx2.sum().backward()
    finally:
        p.close()
        q.close()


# ---- 7. the functor layer and the C++ mirror ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("variational", [False, True], ids=["FITC", "Variational_FITC"])
def test_functor_calc_input_gradient(variational):
    """Deriv.Trained.calc_input_gradient / Deriv.Model.calc_input_gradient against Problem.eval_input_grad, bit for bit --
    including after Model.update_sigma2 (the re-use of V by the functor's bookkeeping) and the state they leave for predictions"""
    from gpr_amd import cov_se_iso, fitc_gp
    key = ("iso", 200, 65, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.Variational_FITC if variational else GP.FITC
    q = _problem(key)
    try:
        kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(log_ell=args["log_ell"], log_sf2=args["log_sf2"]))
        inputs = F.Deriv.Inputs.calc(F.Deriv.Inducing.calc(kernel, Zs), Xs)
        model = F.Deriv.Model.calc(inputs, SIGMA2)
        trained = F.Deriv.Trained.calc(model, y)
        ev, g = q.eval_input_grad(**_eval_args(key, variational=variational))
        got = F.Deriv.Trained.calc_input_gradient(trained)
        assert np.array_equal(got, g)
        assert F.Eval.Trained.calc_log_evidence(trained) == ev.l
        assert F.Deriv.Trained.calc_log_evidence_sigma2(trained) == ev.dl_dsigma2
        Xt = np.asfortranarray(Xs[:, :9] + 0.05)
        means = F.Eval.Means.get(F.Eval.Means.calc(F.Eval.Mean_predictor.calc_trained(trained), F.Eval.Inputs.calc(Xt, inputs.inducing)))
        assert np.array_equal(means, q.predict(Xt, predictive=False, want_variances=False)[0])
        # (the same kernel and inducing points again: the functor re-uses V, so the comparison evaluation does too)
        evm, gm = q.eval_input_grad(**_eval_args(key, variational=variational, model_only=True, reuse_v=True))
        assert np.array_equal(F.Deriv.Model.calc_input_gradient(model), gm)
        # another sigma2 on the same kernel and inducing points: the functor re-uses V (reuse_v), a fresh problem does not
        model2 = F.Deriv.Model.update_sigma2(model, 0.25)
        got2 = F.Deriv.Trained.calc_input_gradient(F.Deriv.Trained.calc(model2, y))
        _, fresh = q.eval_input_grad(**_eval_args(key, variational=variational, sigma2=0.25))
        _within_bound("xgrad.functor_update_sigma2", got2, fresh)
    finally:
        q.close()
        GP.close()


@gpu
def test_cpp_mirror_run_input_grad(tmp_path):
    """gpr::Make_deriv<Cov_se_iso>::run_input_grad (tests/cpp/input_grad_check.cpp, built here with g++ against the header and
    the library) gives Problem.eval_input_grad's matrices bit for bit, trained and model-only"""
    key = ("iso", 200, 65, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    d, n = Xs.shape
    m = Zs.shape[1]
    exe = tmp_path / "input_grad_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "input_grad_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    dump = tmp_path / "case.bin"
    with open(dump, "wb") as f:
        np.array([n, d, m], dtype=np.int64).tofile(f)
        np.array([args["log_ell"], args["log_sf2"], SIGMA2]).tofile(f)
        for a in (Xs, y, Zs):
            np.asfortranarray(a).T.tofile(f) if a.ndim == 2 else a.tofile(f)
    out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split(" ", 1)[0]: np.array(ln.split()[1:], dtype=np.float64) for ln in out.stdout.splitlines()}
    q = _problem(key)
    try:
        ev, g = q.eval_input_grad(**_eval_args(key))
        evm, gm = q.eval_input_grad(**_eval_args(key, model_only=True, reuse_v=True))  # (as the mirror's second call)
        assert vals["l"][0] == ev.l and vals["l1"][0] == evm.l1
        assert np.array_equal(vals["trained"].reshape(n, d).T, g)
        assert np.array_equal(vals["model"].reshape(n, d).T, gm)
    finally:
        q.close()
