"""gprhip_acquire_max_value on the device: max-value entropy search over candidate points from the extremes of drawn paths, its
gradient and the selection of the best top_k.

The criterion is pinned to the device's own posterior -- predict_input_grad, acquire and acquire_max_value on the same points:
`means` and `variances` agree bitwise with gprhip_acquire's (the same kernel body up to the epilogue), and with (a, c_mu, c_v)
the mpmath criterion (tests/max_value_ref.py, 50 digits) at the device's (mu_r, sigma2_r), u = 2^-53 (1 + gamma_max^2):
    values     |values_r - a| <= C_a u a
    dvalues    |dvalues_jr - (c_mu dmu_jr + c_v dsigma2_jr)| <= 4 2^-53 (|c_mu dmu_jr| + |c_v dsigma2_jr|)
                                                                 + C_cmu u |c_mu dmu_jr| + C_cv u mean_j|term_j| |dsigma2_jr|
with the constants C of the CPU grid (tests/test_max_value_host.py); a device ratio above them is a failure.  With a
projection the kernel forms c_mu dmu + c_v dsigma2 in the d projected dimensions and multiplies by tproj afterwards,
predict_input_grad multiplies each gradient first: each side rounds (d + 2) 2^-53 sum_k |T_bk| |.|_k, so that entry b of the
bound takes sum_k |T_bk| |(T^+ dmu_r)_k| in place of |dmu_br| (likewise the variance term; T^+ dmu_r is the gradient in the
projected dimensions, since dmu_r = T times it) and 2 (d + 2) in place of 4.
    c_mu, c_v  recovered per candidate from the D entries of its gradient row by least squares over A = [dmu_r dsigma2_r]:
               with A^+ the pseudo-inverse (numpy's, taken as exact numbers) and chat = A^+ dvalues_r,
               chat - (A^+ A) c = A^+ (A (c_dev - c) + e), e the entries' own rounding (the non-coefficient part of the bound
               above), so  |chat - (A^+ A) c|_k <= |A^+ A|_k. (C_cmu u |c_mu|, C_cv u mean_j|term_j|) + sum_j |A^+_kj| e_j
               -- the CPU-pinned coefficient bounds, and the rounding of the entries carried through the recovery.

Shapes: the smallest that reach every code path -- the one-kernel route (m = 20, d = 3), the general route at m = 70 with
d = 3, 17, 33 (the three DT widths) and with a 5 -> 3 projection; nt = 130 (two 64-point groups and a ragged one) on
problems with 128-row chunks, so that nt crosses a chunk edge and the first chunk's launch has two workgroups (the top-k
tests take 64-row chunks: winners from three chunks)."""
import ctypes
import math
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import margins as M
from tests import max_value_ref as R
from tests.test_gpu_acquire import _check_top
from tests.test_gpu_input_grad import _case
from tests.test_gpu_parity import TOL_GRAD, TOL_POST
from tests.test_gpu_predict_grad import SIGMA2, _path, _problem, _test_points

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 130
CHUNK = 128
TOPK_CHUNK = 64
EPS = 2.0 ** -53
ALL = ("values", "dvalues", "means", "variances")
SMALL = ("iso", 300, 20, 3)
GENERAL = ("iso", 300, 70, 3)
KEYS = [SMALL, GENERAL, ("iso", 300, 70, 17), ("iso", 300, 70, 33), ("proj", 300, 70, 3, 5)]


def _floor_of(key):
    return 1e-10 * math.exp(_case(*key)[3]["log_sf2"])


def _extremes(post, S, maximise):
    """extremes in the units of the posterior: S = 1 the median mean (gamma of both signs), S = 3 that and one far on either
    side (|gamma| >= 45 on every candidate), S = 64 a ladder between the far ones"""
    mu, smax = post["means"], float(np.sqrt(np.max(post["variances"])))
    lo, hi = float(np.min(mu)) - 45.0 * smax, float(np.max(mu)) + 45.0 * smax
    if S == 1:
        return np.array([float(np.median(mu))])
    if S == 3:
        return np.array([hi, float(np.median(mu)), lo] if maximise else [lo, float(np.median(mu)), hi])
    return np.linspace(lo, hi, S)


def _hold(what, key, post, got, extremes, maximise, floor, signs=True):
    """acquire_max_value's outputs `got` against the mpmath criterion at the device's own posterior `post`"""
    refs = R.evaluate(post["means"], post["variances"], extremes, maximise=maximise, var_floor=floor)
    vals, dv = got["values"], got["dvalues"]
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(dv)), what
    D, nt = dv.shape
    proj = key[0] == "proj"
    if proj:
        T = _case(*key)[3]["tproj"]
        d = T.shape[1]
        Tabs, Tpinv = np.abs(T), np.linalg.pinv(T)
    worst_v = worst_g = worst_c = 0.0
    e = mp.mpf(EPS)
    gs = [float(g) for ref in refs for g in ref[4]]
    if signs:
        assert min(gs) < -40 or len(extremes) == 1, min(gs)
        assert min(gs) < 0 < max(gs)
    for r in range(nt):
        a, cmu, cv, cv_abs, _ = refs[r]
        u = R.unit(refs[r])
        err = abs(mp.mpf(float(vals[r])) - a) - R.FLOOR_ULPS * mp.mpf(R.TINY)
        worst_v = max(worst_v, float(err / (u * a)) if err > 0 else 0.0)
        dm, ds = post["dmeans"][:, r], post["dvariances"][:, r]
        if proj:
            am, av = Tabs @ np.abs(Tpinv @ dm), Tabs @ np.abs(Tpinv @ ds)
        else:
            am, av = np.abs(dm), np.abs(ds)
        rounding = []     # per entry: the part of its bound that is the entry's own rounding
        for j in range(D):
            t1, t2 = cmu * float(dm[j]), cv * float(ds[j])
            tiny = R.FLOOR_ULPS * mp.mpf(R.TINY) * (1 + abs(float(dm[j])) + abs(float(ds[j])))
            rounding.append((2 * (d + 2) if proj else 4) * e * (abs(cmu) * float(am[j]) + abs(cv) * float(av[j])) + tiny)
            bound = rounding[j] - tiny + u * (R.C["cmu"] * abs(cmu) * float(am[j]) + R.C["cv"] * cv_abs * float(av[j]))
            errg = abs(mp.mpf(float(dv[j, r])) - (t1 + t2)) - tiny
            if errg <= 0:
                continue
            assert bound > 0, (what, r, j, float(errg))
            worst_g = max(worst_g, float(errg / bound))
        # c_mu and c_v recovered from the row
        A = np.stack([dm, ds], axis=1)
        Ap = np.linalg.pinv(A)
        P = [[mp.fsum(mp.mpf(float(Ap[k, j])) * float(A[j, l]) for j in range(D)) for l in range(2)] for k in range(2)]
        cb = (R.C["cmu"] * u * abs(cmu), R.C["cv"] * u * cv_abs)
        for k in range(2):
            chat = mp.fsum(mp.mpf(float(Ap[k, j])) * float(dv[j, r]) for j in range(D))
            want = P[k][0] * cmu + P[k][1] * cv
            bound = abs(P[k][0]) * cb[0] + abs(P[k][1]) * cb[1] + mp.fsum(abs(float(Ap[k, j])) * rounding[j] for j in range(D))
            errc = abs(chat - want)
            if errc > 0:
                assert bound > 0, (what, r, k, float(errc))
                worst_c = max(worst_c, float(errc / bound))
    print("%s: values ratio c = %.3g (C = %g), gradient error / bound = %.3g, recovered coefficients error / bound = %.3g"
          % (what, worst_v, R.C["a"], worst_g, worst_c))
    M._record("%s.values" % what, worst_v, R.C["a"])
    M._record("%s.dvalues" % what, worst_g, 1.0, proj=proj)
    M._record("%s.coefficients" % what, worst_c, 1.0, proj=proj)
    assert worst_v <= R.C["a"], (what, "values", worst_v)
    assert worst_g <= 1.0, (what, "dvalues", worst_g)
    assert worst_c <= 1.0, (what, "c_mu, c_v", worst_c)
    return refs


@gpu
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_every_route_every_count_both_directions(key):
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind=key[0], n=key[1], m=key[2], d=key[3], D=Xs.shape[0], nt=NT)
    Xt = _test_points(key, NT)
    floor = _floor_of(key)
    p = _problem(key, chunk_rows=CHUNK)
    try:
        post = p.predict_input_grad(Xt, predictive=False)
        acq = p.acquire(Xt, "log_ei", maximise=True, best=0.0, want=("means", "variances"))
        p.set_timing(2)
        for maximise in (True, False):
            for S in (1, 3, 64):
                ext = _extremes(post, S, maximise)
                got = p.acquire_max_value(Xt, ext, maximise=maximise, var_floor=floor, want=ALL)
                stages = p.last_timings()
                assert "pg_grad" in stages and "acq_select" not in stages, stages
                assert _path(stages) == ("small" if key == SMALL else "engine"), stages
                assert np.array_equal(got["means"], acq["means"]) and np.array_equal(got["variances"], acq["variances"])
                assert np.array_equal(got["means"], post["means"]) and np.array_equal(got["variances"], post["variances"])
                _hold("mv.%s.S%d.%s" % ("_".join(map(str, key)), S, "max" if maximise else "min"), key, post, got, ext, maximise, floor)
                assert np.all(got["values"] >= 0.0)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("key", [SMALL, GENERAL], ids=str)
def test_variances_below_the_floor(key):
    """var_floor = the median variance: half the candidates are clamped -- there c_v = 0 exactly, the gradient is c_mu dmu alone
    (the bound of a clamped entry has no variance term at all), and value and c_mu are those of the point (mu, var_floor)"""
    Xt = _test_points(key, NT)
    p = _problem(key, chunk_rows=CHUNK)
    try:
        post = p.predict_input_grad(Xt, predictive=False)
        floor = float(np.median(post["variances"]))
        for maximise in (True, False):
            ext = _extremes(post, 3, maximise)
            got = p.acquire_max_value(Xt, ext, maximise=maximise, var_floor=floor, want=ALL)
            refs = _hold("mv.clamp.%s.%s" % ("_".join(map(str, key)), "max" if maximise else "min"), key, post, got, ext, maximise, floor,
                         signs=False)
            clamped = post["variances"] < floor
            assert 0 < clamped.sum() < NT and all((refs[r][2] == 0) == bool(clamped[r]) for r in range(NT))
            # c_v = 0 exactly: the kernel stores c_mu dmu_j + 0, the rounded product of ONE double c_mu with the entry that
            # predict_input_grad stores -- such a double exists within a few ulp of the quotient of the largest component
            for r in np.flatnonzero(clamped):
                dm, row = post["dmeans"][:, r], got["dvalues"][:, r]
                j0 = int(np.argmax(np.abs(dm)))
                cm = row[j0] / dm[j0]
                cands = [cm]
                for _ in range(4):
                    cands = [np.nextafter(cands[0], -np.inf)] + cands + [np.nextafter(cands[-1], np.inf)]
                assert any(np.array_equal(c * dm, row) for c in cands), (r, cm, row, dm)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("key", [SMALL, GENERAL, ("proj", 300, 70, 3, 5)], ids=str)
@pytest.mark.parametrize("k", [5, 64])
def test_top_k_across_the_chunk_edges_host_and_device_pointers_and_repeats(k, key):
    import torch
    D = _case(*key)[0].shape[0]
    Xt = _test_points(key, NT)
    p = _problem(key, chunk_rows=TOPK_CHUNK)
    try:
        post = p.predict_input_grad(Xt, predictive=False)
        ext = _extremes(post, 3, True)
        kw = dict(maximise=True, var_floor=_floor_of(key))
        full = p.acquire_max_value(Xt, ext, want=ALL, **kw)
        p.set_timing(2)
        got = p.acquire_max_value(Xt, ext, top_k=k, **kw)
        assert "acq_select" in p.last_timings()
        assert np.array_equal(got["values"], full["values"]) and np.array_equal(got["dvalues"], full["dvalues"])
        _check_top(got, full, k)
        if k == 64:  # (64 of 130: from more than one of the chunks 0 .. 63, 64 .. 127, 128 .. 129)
            assert len(set(got["top_index"] // TOPK_CHUNK)) > 1, got["top_index"]
        only = p.acquire_max_value(Xt, ext, want=(), top_k=k, **kw)       # nothing of size nt leaves the device
        assert set(only) == {"top_index", "top_values", "top_dvalues"}
        again = p.acquire_max_value(Xt, ext, want=(), top_k=k, **kw)
        for x in only:
            assert np.array_equal(only[x], got[x], equal_nan=True) and np.array_equal(only[x], again[x], equal_nan=True)
        # device pointers: the same bits; with only the top-k requested the other buffers keep their poison
        dev = torch.device("cuda:0")
        xt = torch.tensor(np.ascontiguousarray(Xt.T), device=dev)
        outs = {w: torch.full((NT, D) if w == "dvalues" else (NT,), float("nan"), dtype=torch.float64, device=dev) for w in ALL}
        ptrs = {w: v.data_ptr() for w, v in outs.items()}
        torch.cuda.synchronize()
        top = p.acquire_max_value(xt.data_ptr(), ext, want=(), out_device_ptrs=ptrs, nt=NT, top_k=k, **kw)
        for x in only:
            assert np.array_equal(only[x], top[x], equal_nan=True)
        assert all(bool(torch.isnan(v).all()) for v in outs.values())
        top = p.acquire_max_value(xt.data_ptr(), ext, want=ALL, out_device_ptrs=ptrs, nt=NT, top_k=k, **kw)
        _check_top(top, full, k)
        for w in ALL:
            g = outs[w].cpu().numpy()
            assert np.array_equal(g if g.ndim == 1 else g.T, full[w]), w
        assert all(np.array_equal(p.acquire_max_value(Xt, ext, want=ALL, **kw)[w], full[w]) for w in ALL)   # two runs, same bits
        # host gradient with ldg > D: rows D.. are left as they were
        wide = np.full((D + 3, NT), np.nan, order="F")
        vp = ctypes.c_void_p
        st = p._lib.gprhip_acquire_max_value(p._handle(), ext.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(ext), 1,
                                             kw["var_floor"], vp(Xt.ctypes.data), D, NT, None, vp(wide.ctypes.data), D + 3, None,
                                             None, 0, None, None, None, 0)
        assert st == _lib.OK and np.array_equal(wide[:D], full["dvalues"]) and np.all(np.isnan(wide[D:]))
    finally:
        p.close()


@gpu
def test_state_rules_and_refusals_leave_the_problem_as_it_was():
    key = ("fat", 64, 10, 3, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    m = Zs.shape[1]
    nt = 65
    Xt = _test_points(key, nt)
    vals = np.full(nt, np.nan)
    ext = np.array([0.3, -0.1, 0.7])
    vp = ctypes.c_void_p

    def raw(q, extremes=ext, n_ext=3, var_floor=1e-10, ld=D, ldg=D, nt=nt, top_k=0, values=True, dvalues=None, on_device=0):
        return q._lib.gprhip_acquire_max_value(q._handle(), extremes.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n_ext, 1,
                                               var_floor, vp(Xt.ctypes.data), ld, nt, vp(vals.ctypes.data) if values else None,
                                               dvalues, ldg, None, None, top_k, None, None, None, on_device)

    p = _problem(key)
    f32 = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m, precision=gpr_amd.F32_BULK)
    empty = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m)
    try:
        kw = dict(maximise=True, best=0.1, var_floor=1e-10)
        before = p.acquire(Xt, "log_ei", **kw)
        p.set_timing(2)
        grad = np.full((D, nt), np.nan, order="F")
        for bad, reason in ((dict(n_ext=0), b"n_extremes"), (dict(n_ext=65), b"n_extremes"),
                            (dict(extremes=np.array([0.3, np.nan, 0.7])), b"finite"), (dict(var_floor=0.0), b"var_floor"),
                            (dict(var_floor=float("inf")), b"var_floor"), (dict(top_k=65), b"top_k"), (dict(top_k=3), b"top_index"),
                            (dict(values=False), b"nothing is requested"), (dict(ld=D - 1), b"bad ld "),
                            (dict(ld=D + 1, on_device=1), b"bad ld "), (dict(dvalues=vp(grad.ctypes.data), ldg=D - 1), b"bad ldg"),
                            (dict(nt=0), b"invalid arguments")):
            assert raw(p, **bad) == _lib.EBADARG, bad
            msg = p._lib.gprhip_last_error()
            assert msg.startswith(b"gprhip_acquire_max_value:") and reason in msg, (bad, msg)
        assert np.all(np.isnan(vals)) and np.all(np.isnan(grad)) and p.last_timings() == {}      # nothing was enqueued
        after = p.acquire(Xt, "log_ei", **kw)
        assert all(np.array_equal(before[w], after[w]) for w in before)
        lms = np.asfortranarray(np.random.default_rng(3).uniform(-1.0, 0.5, size=(D, m)))
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, log_multiscales_m05=lms, **args)
        assert raw(p) == _lib.EBADARG and b"multiscales" in p._lib.gprhip_last_error()
        p.set_targets_many(np.asfortranarray(np.stack([y, 2.0 * y], axis=1)))
        p.eval_targets(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        assert raw(p) == _lib.ESTATE
        assert raw(f32) == _lib.EBADARG and raw(empty) == _lib.ESTATE
        assert np.all(np.isnan(vals))
        # the next correct call works, and a refused one in between changes nothing
        p.set_targets(y)
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        again = p.acquire(Xt, "log_ei", **kw)
        assert raw(p, n_ext=0) == _lib.EBADARG
        assert all(np.array_equal(again[w], p.acquire(Xt, "log_ei", **kw)[w]) for w in again)
        post = p.predict_input_grad(Xt, predictive=False)
        got = p.acquire_max_value(Xt, _extremes(post, 3, True), maximise=True, var_floor=1e-10, want=ALL)
        M.note(cond=cond, kind="fat", n=n, m=m, d=3, nt=nt)
        _hold("mv.after_refusals", key, post, got, _extremes(post, 3, True), True, 1e-10)
    finally:
        for q in (p, f32, empty):
            q.close()


@gpu
@pytest.mark.parametrize("key", [SMALL, GENERAL], ids=str)
def test_after_observe_the_updated_posterior_is_used(key):
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind=key[0], n=key[1], m=key[2], d=key[3], D=Xs.shape[0], nt=NT)
    Xt = _test_points(key, NT)
    floor = _floor_of(key)
    p = _problem(key, chunk_rows=CHUNK)
    try:
        post0 = p.predict_input_grad(Xt, predictive=False)
        ext = _extremes(post0, 3, True)
        before = p.acquire_max_value(Xt, ext, maximise=True, var_floor=floor, want=ALL)
        p.observe(np.asfortranarray(Xt[:, :4]), post0["means"][:4] + 0.5)
        post = p.predict_input_grad(Xt, predictive=False)
        got = p.acquire_max_value(Xt, ext, maximise=True, var_floor=floor, want=ALL)
        assert np.array_equal(got["means"], post["means"]) and np.array_equal(got["variances"], post["variances"])
        assert not np.array_equal(got["values"], before["values"]) and not np.array_equal(got["means"], before["means"])
        _hold("mv.observed.%s" % "_".join(map(str, key)), key, post, got, ext, True, floor, signs=False)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("maximise", [True, False], ids=["max", "min"])
def test_max_value_search_end_to_end(maximise):
    """Draw 0 has z = 0: its path is the posterior mean, so predict_input_grad is a second oracle for its extreme at extreme_x
    (TOL_POST of the largest mean: two kernels sum the same products in different orders).  The extremes are the per-draw
    best of sample_paths_refine from sample_paths' winners, and the criterion is acquire_max_value's on them, bit for bit."""
    key = SMALL
    Xs, y, Zs, args, ok, cond = _case(*key)
    m, nd, k = Zs.shape[1], 4, 3
    grid = _test_points(key, NT)
    lower, upper = grid.min(axis=1) - 0.1, grid.max(axis=1) + 0.1
    z = np.asfortranarray(np.random.default_rng(11).normal(size=(m, nd)))
    z[:, 0] = 0.0
    opts = dict(max_evals=30)
    p = _problem(key, chunk_rows=CHUNK)
    try:
        out = p.max_value_search(z, lower, upper, grid, k, opts, maximise=maximise, want=ALL, acquire_top_k=5)
        tops = p.sample_paths(grid, z, maximise=maximise, top_k=k, want_samples=False)
        cols = tops["top_index"].T.reshape(-1)
        assert np.all(cols >= 0)
        draw_of = np.repeat(np.arange(nd), k)
        ref = p.sample_paths_refine(grid[:, cols], z, draw_of, lower=lower, upper=upper, maximise=maximise, want=("x", "values"), **opts)
        s = 1.0 if maximise else -1.0
        obj = ref["values"].reshape(nd, k)
        assert np.array_equal(out["extremes"], s * obj.max(axis=1))
        where = np.arange(nd) * k + obj.argmax(axis=1)
        assert np.array_equal(out["extreme_x"], ref["x"][:, where])
        # the refined extreme is at least as good as the best grid sample of its draw
        assert np.all(s * out["extremes"] >= s * tops["top_values"][0] - 1e-12)
        mean_at = p.predict_input_grad(np.asfortranarray(out["extreme_x"][:, :1]), predictive=False, want=("means",))["means"][0]
        scale = float(np.max(np.abs(p.predict_input_grad(grid, predictive=False, want=("means",))["means"])))
        assert abs(out["extremes"][0] - mean_at) <= TOL_POST * scale, (out["extremes"][0], mean_at)
        direct = p.acquire_max_value(grid, out["extremes"], maximise=maximise, want=ALL, top_k=5)
        for w in direct:
            assert np.array_equal(direct[w], out[w], equal_nan=True), w
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("key", [SMALL, ("proj", 300, 70, 3, 5)], ids=str)
def test_torch_front_end(key):
    """autograd.acquire_max_value: the forward is Problem.acquire_max_value's values, the backward g[:, None] * dvalues"""
    import torch
    from gpr_amd.autograd import acquire_max_value
    Xt = _test_points(key, NT)
    dev = torch.device("cuda:0")
    p = _problem(key, chunk_rows=CHUNK)
    try:
        post = p.predict_input_grad(Xt, predictive=False)
        for maximise in (True, False):
            ext = _extremes(post, 3, maximise)
            want = p.acquire_max_value(Xt, ext, maximise=maximise)
            x = torch.tensor(np.ascontiguousarray(Xt.T), device=dev, requires_grad=True)
            a = acquire_max_value(p, x, ext, maximise=maximise)
            assert a.shape == (NT,) and a.dtype == torch.float64
            assert np.array_equal(a.detach().cpu().numpy(), want["values"])
            g = torch.linspace(0.5, 2.0, NT, dtype=torch.float64, device=dev)
            (gx,) = torch.autograd.grad((g * a).sum(), x)
            assert np.array_equal(gx.cpu().numpy().T, g.cpu().numpy()[None, :] * want["dvalues"])
            assert np.array_equal(acquire_max_value(p, x.detach(), ext, maximise=maximise).cpu().numpy(), want["values"])
        with pytest.raises(TypeError):
            acquire_max_value(p, x, ext, maximise=True, top_k=3)
    finally:
        p.close()


@gpu
def test_functor_acquisition_calc_max_value():
    from gpr_amd import cov_se_iso, fitc_gp
    key = GENERAL
    Xs, y, Zs, args, ok, cond = _case(*key)
    Xt = _test_points(key, NT)
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    q = _problem(key)
    try:
        kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(log_ell=args["log_ell"], log_sf2=args["log_sf2"]))
        inputs = F.Deriv.Inputs.calc(F.Deriv.Inducing.calc(kernel, Zs), Xs)
        trained = F.Deriv.Trained.calc(F.Deriv.Model.calc(inputs, SIGMA2), y)
        ext = _extremes(q.predict_input_grad(Xt, predictive=False), 3, True)
        kw = dict(maximise=True, top_k=5)
        want = q.acquire_max_value(Xt, ext, **kw)
        got = F.Eval.Acquisition.calc_max_value(trained, F.Eval.Inputs.calc(Xt, inputs.inducing), ext, **kw)
        assert set(got) == set(want) and all(np.array_equal(got[w], want[w]) for w in want)
    finally:
        q.close()
        GP.close()


@gpu
def test_cpp_mirror_method(tmp_path):
    """gpr::Make_deriv<Cov_se_iso>::FITC::Acquisition::calc_max_value (tests/cpp/max_value_check.cpp, built here against the
    header and the library).  The mirror's model state comes from its own sequence of evaluations, so its numbers are held
    to Problem.acquire_max_value's by the bounds of the posterior (TOL_POST / TOL_GRAD of the largest entry, as the mirror
    test of tests/test_gpu_acquire.py; extremes two standard deviations around the means keep the criterion's sensitivity
    to the posterior of order 1), not to its bits; the selection is checked against the mirror's own values."""
    key = ("iso", 200, 65, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    nt, k = 65, 5
    Xt = _test_points(key, nt)
    d, n = Xs.shape
    m = Zs.shape[1]
    exe = tmp_path / "max_value_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "max_value_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    floor = _floor_of(key)
    q = _problem(key)
    try:
        post = q.predict_input_grad(Xt, predictive=False)
        smax = float(np.sqrt(np.max(post["variances"])))
        ext = np.array([float(np.max(post["means"])) + 2.0 * smax, float(np.median(post["means"])), float(np.min(post["means"])) - 2.0 * smax])
        dump = tmp_path / "case.bin"
        with open(dump, "wb") as f:
            np.array([n, d, m, nt, k, len(ext)], dtype=np.int64).tofile(f)
            np.array([args["log_ell"], args["log_sf2"], SIGMA2]).tofile(f)
            np.array([1.0, floor]).tofile(f)
            ext.tofile(f)
            for a in (Xs, y, Zs, Xt):
                np.asfortranarray(a).T.tofile(f) if a.ndim == 2 else a.tofile(f)
        out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        vals = {ln.split(" ", 1)[0]: np.array(ln.split()[1:], dtype=np.float64) for ln in out.stdout.splitlines()}
        want = q.acquire_max_value(Xt, ext, maximise=True, var_floor=floor)
        got_v, got_g = vals["values"], vals["dvalues"].reshape(nt, d).T
        M.check_vec("mv.cpp_mirror.values", got_v, want["values"], TOL_POST)
        M.check_vec("mv.cpp_mirror.dvalues", got_g, want["dvalues"], TOL_GRAD)
        idx = vals["top_index"].astype(np.int64)
        order = np.argsort(-got_v, kind="stable")[:k]
        assert np.array_equal(idx, order)
        assert np.array_equal(vals["top_values"], got_v[idx])
        assert np.array_equal(vals["top_dvalues"].reshape(k, d).T, got_g[:, idx])
    finally:
        q.close()
