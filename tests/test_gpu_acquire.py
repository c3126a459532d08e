"""gprhip_acquire on the device: the acquisition criteria EI, LOG_EI, PI and BOUND over candidate points, their gradient and
the selection of the best top_k.

Layer A pins the criterion to the device's own posterior -- predict_input_grad and acquire on the same points: `means` and
`variances` agree bitwise, and with (a, c_mu, c_v, u) the mpmath criterion (tests/acquire_ref.py, 50 digits) at the device's
(mu_r, sigma2_r):
    values     |values_r - a| <= c 2^-53 (1 + u^2) |a|        (LOG_EI: c 2^-53 (1 + u^2) (1 + |log sigma|), absolute)
    dvalues    |dvalues_jr - (c_mu dmu_jr + c_v dsigma2_jr)| <= (c (1 + u^2) + 4) 2^-53 (|c_mu dmu_jr| + |c_v dsigma2_jr|)
               (with a projection: TOL_GRAD of |c_mu| max_j |dmu_jr| + |c_v| max_j |dsigma2_jr| per row -- the two sides round
               the tproj product differently)
1 + u^2 is the conditioning of Phi, and of delta Phi + sigma phi, with respect to the rounding of u: it is not slack.  Where
EI, PI and their coefficients lie in or below the subnormal range (u < -37) the spacing of the subnormals is what is left of
the precision: a few 2^-1074 (_abs_floor below) are added to those bounds, as absolute terms.
The constant c per kind is C below: at most 10 x the worst ratio achieved over this whole module
(profiles/acquire_margins.txt, GPR_MARGINS_LOG records every one).

Layer B holds `values` end to end against the 80-bit posterior (tests/predict_grad_ref.py) pushed through the mpmath
criterion, to the first-order propagation of the posterior bounds, |c_mu| TOL_POST max|mu| + |c_v| TOL_POST max sigma2, plus
the layer-A bound.

Top-k: top_index against a stable numpy arg-sort of the device's own values; top_values / top_dvalues bitwise the
corresponding entries."""
import ctypes
import math
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from oracle import fitc_oracle as O
from tests import acquire_ref as R
from tests import margins as M
from tests.test_gpu_input_grad import _case
from tests.test_gpu_parity import TOL_GRAD, TOL_POST
from tests.test_gpu_predict_grad import DIMS, NTS, PAIRS, PAIRS_WIDE, PROJ_DIMS, SIGMA2, _path, _path_of, _problem, _reference, _test_points

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 65
EPS = 2.0 ** -53
TINY = 2.0 ** -1074
KAPPA = 2.0
ALL = ("values", "dvalues", "means", "variances")
# the constant c of the layer-A bounds per kind: <= 10 x the worst achieved ratio of profiles/acquire_margins.txt
C = {"ei": 40.0, "log_ei": 35.0, "pi": 30.0, "bound": 8.0}


# The cases take best = median of the reference mu, and the reference must reach u <= -1 and u >= 1 there, so that both sides of
# every formula run.  At these shapes it cannot (one training point or one test point: a flat posterior or a single u = -xi / sigma;
# the other three reach [-0.8, 1.3], [-0.7, 1.1] and [-3.0, 0.8]): they run the median all the same and, on top, best one and
# a half standard deviations below the smallest and above the largest mean, where |u| >= 1.5 on every row by construction.
U_RANGE_SHORT = {(("iso", 1, 1, 3), 65), (("iso", 64, 10, 3), 1), (("iso", 200, 129, 3), 1), (("iso", 64, 10, 8), 65),
                 (("iso", 64, 10, 64), 65), (("proj", 200, 129, 2, 5), 65)}


def _floor_of(key):
    return 1e-10 * math.exp(_case(*key)[3]["log_sf2"])


def _variants(ref_means):
    """(maximise, xi) over both directions and xi in {0, 0.05 std mu}"""
    xi = 0.05 * float(np.std(ref_means))
    return [(True, 0.0), (True, xi), (False, 0.0), (False, xi)]


def _kw(kind, maximise, xi, best, floor, predictive=False):
    return dict(maximise=maximise, best=best, xi=xi if kind != R.BOUND else 0.0, kappa=KAPPA if kind == R.BOUND else 0.0,
                var_floor=floor, predictive=predictive)


def _ref_kw(kw):
    return {k: v for k, v in kw.items() if k != "predictive"}


def _abs_floor(kind, sigma, scale=1.0):
    """what the subnormal spacing leaves of EI / PI and their coefficients in the deep tail"""
    return 8.0 * TINY * max(1.0, sigma, scale) if kind in (R.EI, R.PI) else 0.0


def _layer_a(what, kind, kw, post, got, proj=False, clamp_all=False):
    """acquire's outputs `got` against the mpmath criterion at the device's own posterior `post`"""
    name = R.KIND_NAMES[kind]
    assert np.array_equal(got["means"], post["means"]) and np.array_equal(got["variances"], post["variances"]), what
    a, cmu, cv, us = R.evaluate(kind, post["means"], post["variances"], **_ref_kw(kw))
    vals, dv = got["values"], got["dvalues"]
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(dv)), what
    D, nt = dv.shape
    worst_v = worst_g = 0.0
    e = mp.mpf(EPS)
    for r in range(nt):
        f = 1 + us[r] * us[r]
        sigma = math.sqrt(max(float(post["variances"][r]), kw["var_floor"]))
        if clamp_all:
            assert cv[r] == 0 and float(post["variances"][r]) < kw["var_floor"]
        unit = e * f * (1 + abs(math.log(sigma))) if kind == R.LOG_EI else e * f * abs(a[r])
        err = abs(mp.mpf(float(vals[r])) - a[r]) - _abs_floor(kind, sigma)
        worst_v = max(worst_v, float(err / unit) if err > 0 else 0.0)
        dm, ds = post["dmeans"][:, r], post["dvariances"][:, r]
        if proj:
            ref_row = [cmu[r] * float(dm[j]) + cv[r] * float(ds[j]) for j in range(D)]
            scale = abs(cmu[r]) * float(np.max(np.abs(dm))) + abs(cv[r]) * float(np.max(np.abs(ds)))
            errg = max(abs(mp.mpf(float(dv[j, r])) - ref_row[j]) for j in range(D)) - _abs_floor(kind, sigma, float(np.max(np.abs(dm))))
            worst_g = max(worst_g, float(errg / scale) if errg > 0 else 0.0)
            continue
        for j in range(D):
            t1, t2 = cmu[r] * float(dm[j]), cv[r] * float(ds[j])
            S = abs(t1) + abs(t2)
            errg = abs(mp.mpf(float(dv[j, r])) - (t1 + t2)) - _abs_floor(kind, sigma, abs(float(dm[j])) + abs(float(ds[j])) / sigma)
            if errg <= 0:
                continue
            assert S > 0, (what, r, j, float(errg))
            worst_g = max(worst_g, float((errg / (e * S) - 4) / f))
    print("%s: values ratio c = %.2f, gradient %s = %.3g (c = %g)" % (what, worst_v, "of TOL_GRAD" if proj else "ratio c",
                                                                      worst_g / TOL_GRAD if proj else worst_g, C[name]))
    M._record("%s.values" % what, worst_v, C[name], acq=name)
    M._record("%s.dvalues" % what, worst_g, TOL_GRAD if proj else C[name], acq=name, proj=proj)
    assert worst_v <= C[name], (what, "values", worst_v)
    assert worst_g <= (TOL_GRAD if proj else C[name]), (what, "dvalues", worst_g)
    return us


def _run(key, what, nt=NT, path=None, kinds=R.KINDS, predictive=False, problem=None, **pkw):
    """every kind x direction x xi at one case: predict_input_grad and acquire with all outputs on the same points"""
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind=key[0], n=key[1], m=key[2], d=key[3], D=Xs.shape[0], nt=nt)
    ref = _reference(key, nt, predictive)
    best = float(np.median(ref["means"]))
    Xt = _test_points(key, nt)
    floor = _floor_of(key)
    p = problem if problem is not None else _problem(key, **pkw)
    try:
        post = p.predict_input_grad(Xt, predictive=predictive)
        p.set_timing(2)
        smax = float(np.sqrt(np.max(ref["variances"])))
        bests = [(best, "")]
        if (key, nt) in U_RANGE_SHORT:
            bests += [(float(np.min(ref["means"])) - 1.5 * smax, ".lo"), (float(np.max(ref["means"])) + 1.5 * smax, ".hi")]
        for kind in kinds:
            for b, btag in bests:
                for maximise, xi in _variants(ref["means"]):
                    kw = _kw(kind, maximise, xi, b, floor, predictive)
                    got = p.acquire(Xt, kind, want=ALL, **kw)
                    stages = p.last_timings()
                    assert "pg_grad" in stages and "acq_select" not in stages, stages
                    if path is not None:
                        assert _path(stages) == path, (stages, path)
                    tag = "%s.%s.%s%s%s" % (what, R.KIND_NAMES[kind], "max" if maximise else "min", "_xi" if xi else "", btag)
                    _layer_a(tag, kind, kw, post, got, proj=key[0] == "proj")
                    ur = [R.point(kind, m_, v_, **_ref_kw(kw))[3] for m_, v_ in zip(ref["means"], ref["variances"])]
                    if btag:
                        assert min(abs(u) for u in ur) >= 1, (tag, float(min(ur)), float(max(ur)))
                    elif (key, nt) not in U_RANGE_SHORT:  # both sides of every formula run
                        assert min(ur) <= -1 and max(ur) >= 1, (tag, float(min(ur)), float(max(ur)))
        return p
    finally:
        if problem is None:
            p.close()


# ---- layer A ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", PAIRS)
def test_all_kinds_on_both_kernel_families(n, m):
    _run(("iso", n, m, 3), "acq.iso", path=_path_of(m))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("nt", NTS)
def test_row_tile_edges(nt, n, m):
    _run(("iso", n, m, 3), "acq.iso_nt%d" % nt, nt=nt, path=_path_of(m))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("d", DIMS)
def test_every_kernel_width(d, n, m):
    _run(("iso", n, m, d), "acq.iso_d%d" % d, path=_path_of(m, d))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("D,d", PROJ_DIMS)
def test_with_projection(D, d, n, m):
    _run(("proj", n, m, d, D), "acq.proj_%d_%d" % (D, d), path=_path_of(m, d))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_predictive_variance(n, m):
    _run(("iso", n, m, 3), "acq.iso_predictive", path=_path_of(m), predictive=True)


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_model_state_of_a_variational_evaluation(n, m):
    _run(("iso", n, m, 3), "acq.iso_variational", path=_path_of(m), variational=True)


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_loaded_predictor(n, m):
    """load_predictor with the oracle's coefficients and factors; without factors only the mean-only bound is served"""
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    out = O.evaluate(ok, Zs, Xs, y, SIGMA2, want_grad=False, keep=True)
    model = out["model"]
    Xt = _test_points(key, NT)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, 3, 3, m)
    try:
        p.load_predictor(sigma2=SIGMA2, inducing=Zs, coeffs=out["coeffs"],
                         co_variance_coeffs=(np.triu(model["inducing"]["chol_km"]), np.triu(model["r_mat"])), **args)
        _run(key, "acq.loaded", path=_path_of(m), problem=p)
        p.load_predictor(sigma2=SIGMA2, inducing=Zs, coeffs=out["coeffs"], **args)
        with pytest.raises(gpr_amd.GprHipError) as e:
            p.acquire(Xt, "ei", maximise=True)
        assert e.value.status == _lib.ESTATE
        got = p.acquire(Xt, "bound", maximise=False, kappa=0.0, want=("values", "dvalues", "means"))
        assert np.array_equal(got["values"], -got["means"])
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_three_chunks(n, m):
    _run(("iso", n, m, 3), "acq.iso_chunks", nt=300, path=_path_of(m), chunk_rows=128)


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_bound_without_kappa_runs_the_mean_part_alone(n, m):
    key = ("iso", n, m, 3)
    Xt = _test_points(key, NT)
    p = _problem(key)
    try:
        post = p.predict_input_grad(Xt, predictive=False)
        p.set_timing(2)
        for maximise in (True, False):
            got = p.acquire(Xt, "bound", maximise=maximise, kappa=0.0, want=("values", "dvalues", "means"))
            stages = p.last_timings()
            assert "pg_grad" in stages and not {"pg_m", "pg_gemm", "pg_cov"} & set(stages), stages
            s = 1.0 if maximise else -1.0
            assert np.array_equal(got["means"], post["means"])
            assert np.array_equal(got["values"], s * post["means"]) and np.array_equal(got["dvalues"], s * post["dmeans"])
        full = p.acquire(Xt, "bound", maximise=True, kappa=0.0, want=ALL)   # the variances too: the full route
        assert "pg_grad" in p.last_timings() and np.array_equal(full["variances"], post["variances"])
        assert np.array_equal(full["values"], post["means"]) and np.array_equal(full["dvalues"], post["dmeans"])
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_deep_tail(n, m):
    """best = max mu + 40 max sigma (maximise): u <= -40 on every row.  EI and PI are finite, >= 0 and within their bounds
    (subnormal or 0), LOG_EI and its gradient finite and within theirs; LOG_EI once more at + 1000 max sigma."""
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind="iso", n=n, m=m, d=3, nt=NT)
    ref = _reference(key, NT, False)
    Xt = _test_points(key, NT)
    floor = _floor_of(key)
    smax = float(np.sqrt(np.max(ref["variances"])))
    p = _problem(key)
    try:
        post = p.predict_input_grad(Xt, predictive=False)
        for far, kinds in ((40.0, (R.EI, R.LOG_EI, R.PI)), (1000.0, (R.LOG_EI,))):
            best = float(np.max(ref["means"])) + far * smax
            for kind in kinds:
                kw = _kw(kind, True, 0.0, best, floor)
                got = p.acquire(Xt, kind, want=ALL, **kw)
                us = _layer_a("acq.tail%d.%s" % (far, R.KIND_NAMES[kind]), kind, kw, post, got)
                assert max(us) <= -0.999 * far, float(max(us))
                if kind != R.LOG_EI:
                    assert np.all(got["values"] >= 0.0) and np.all(got["values"] < 1e-300)
                else:
                    assert np.all(got["values"] < -0.4 * far * far)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_clamped_variance(n, m):
    """var_floor = 10 sf2: every row is clamped -- the values are the criterion at (mu, var_floor), dvalues = c_mu dmu"""
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind="iso", n=n, m=m, d=3, nt=NT)
    ref = _reference(key, NT, False)
    Xt = _test_points(key, NT)
    floor = 10.0 * math.exp(args["log_sf2"])
    p = _problem(key)
    try:
        post = p.predict_input_grad(Xt, predictive=False)
        for kind in R.KINDS:
            for maximise in (True, False):
                kw = _kw(kind, maximise, 0.0, float(np.median(ref["means"])), floor)
                got = p.acquire(Xt, kind, want=ALL, **kw)
                _layer_a("acq.clamp.%s" % R.KIND_NAMES[kind], kind, kw, post, got, clamp_all=True)
    finally:
        p.close()


# ---- the contract of the entry point ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", [("proj", 64, 10, 2, 5), ("proj", 200, 129, 2, 5), ("iso", 200, 129, 3)], ids=str)
def test_host_and_device_outputs_agree_padding_rows_stay_and_runs_repeat(key):
    import torch
    D = _case(*key)[0].shape[0]
    Xt = _test_points(key, NT)
    best = float(np.median(_reference(key, NT, False)["means"]))
    p = _problem(key)
    try:
        dev = torch.device("cuda:0")
        xt = torch.tensor(np.ascontiguousarray(Xt.T), device=dev)
        for kind in R.KINDS:
            kw = _kw(kind, True, 0.01, best, _floor_of(key))
            host = p.acquire(Xt, kind, want=ALL, **kw)
            again = p.acquire(Xt, kind, want=ALL, **kw)
            assert all(np.array_equal(host[k], again[k]) for k in ALL)
            default_floor = p.acquire(Xt, kind, want=ALL, **{k: v for k, v in kw.items() if k != "var_floor"})
            assert all(np.array_equal(host[k], default_floor[k]) for k in ALL)
            outs = {k: torch.full((NT, D) if k == "dvalues" else (NT,), float("nan"), dtype=torch.float64, device=dev) for k in ALL}
            torch.cuda.synchronize()
            assert p.acquire(xt.data_ptr(), kind, want=ALL, out_device_ptrs={k: v.data_ptr() for k, v in outs.items()}, nt=NT,
                             **kw) == {}
            for k in ALL:
                g = outs[k].cpu().numpy()
                assert np.array_equal(g if g.ndim == 1 else g.T, host[k]), (kind, k)
            for want in (("values",), ("dvalues",), ("values", "means")):
                part = p.acquire(Xt, kind, want=want, **kw)
                assert set(part) == set(want) and all(np.array_equal(part[k], host[k]) for k in want)
            # host gradient with ldg > D: rows D.. are left as they were
            wide = np.full((D + 3, NT), np.nan, order="F")
            acq = _lib.Acquisition(kind, 1, 0, kw["best"], kw["xi"], kw["kappa"], kw["var_floor"])
            vp = ctypes.c_void_p
            st = p._lib.gprhip_acquire(p._handle(), ctypes.byref(acq), vp(Xt.ctypes.data), D, NT, None, vp(wide.ctypes.data), D + 3,
                                       None, None, 0, None, None, None, 0)
            assert st == _lib.OK and np.array_equal(wide[:D], host["dvalues"]) and np.all(np.isnan(wide[D:]))
    finally:
        p.close()


@gpu
def test_refusals_leave_the_next_correct_call_working():
    key = ("fat", 64, 10, 3, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    m = Zs.shape[1]
    Xt = _test_points(key, NT)
    vals = np.full(NT, np.nan)
    vp = ctypes.c_void_p

    def raw(q, acq, ld=D, nt=NT, top_k=0, top_index=None, values=True, on_device=0):
        return q._lib.gprhip_acquire(q._handle(), ctypes.byref(acq), vp(Xt.ctypes.data), ld, nt, vp(vals.ctypes.data) if values else None,
                                     None, D, None, None, top_k, top_index, None, None, on_device)

    def acq(**kw):
        base = dict(kind=R.EI, maximise=1, predictive=0, best=0.0, xi=0.0, kappa=0.0, var_floor=1e-10)
        base.update(kw)
        return _lib.Acquisition(*[base[f] for f, _ in _lib.Acquisition._fields_])

    p = _problem(key)
    f32 = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m, precision=gpr_amd.F32_BULK)
    empty = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m)
    try:
        p.set_timing(2)
        for bad in (acq(kind=7), acq(xi=-1.0), acq(kind=R.BOUND, kappa=-1.0), acq(var_floor=0.0), acq(var_floor=float("inf")),
                    acq(best=float("nan"))):
            assert raw(p, bad) == _lib.EBADARG
        assert raw(p, acq(), top_k=65, top_index=(ctypes.c_int64 * 65)()) == _lib.EBADARG
        assert raw(p, acq(), top_k=3) == _lib.EBADARG
        assert raw(p, acq(), values=False) == _lib.EBADARG
        assert raw(p, acq(), ld=D - 1) == _lib.EBADARG and raw(p, acq(), ld=D + 1, on_device=1) == _lib.EBADARG
        assert raw(p, acq(), nt=0) == _lib.EBADARG
        assert np.all(np.isnan(vals)) and p.last_timings() == {}                 # nothing was enqueued
        lms = np.asfortranarray(np.random.default_rng(3).uniform(-1.0, 0.5, size=(D, m)))
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, log_multiscales_m05=lms, **args)
        assert raw(p, acq()) == _lib.EBADARG
        p.set_targets_many(np.asfortranarray(np.stack([y, 2.0 * y], axis=1)))
        p.eval_targets(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        assert raw(p, acq()) == _lib.ESTATE
        assert raw(f32, acq()) == _lib.EBADARG and raw(empty, acq()) == _lib.ESTATE
        assert np.all(np.isnan(vals))
        # the next correct call works
        p.set_targets(y)
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        post = p.predict_input_grad(Xt, predictive=False)
        best = float(np.median(post["means"]))
        kw = _kw(R.EI, True, 0.0, best, 1e-10)
        M.note(cond=cond, kind="fat", n=n, m=m, d=3, nt=NT)
        _layer_a("acq.after_refusals", R.EI, kw, post, p.acquire(Xt, R.EI, want=ALL, **kw))
    finally:
        for q in (p, f32, empty):
            q.close()


# ---- layer B: end to end ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_values_end_to_end(n, m):
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind="iso", n=n, m=m, d=3, nt=NT)
    ref = _reference(key, NT, True)
    Xt = _test_points(key, NT)
    best = float(np.median(ref["means"]))
    mu_max, var_max = float(np.max(np.abs(ref["means"]))), float(np.max(ref["variances"]))
    p = _problem(key)
    try:
        p.set_timing(2)
        for kind in R.KINDS:
            name = R.KIND_NAMES[kind]
            for maximise, xi in _variants(ref["means"]):
                kw = _kw(kind, maximise, xi, best, _floor_of(key), True)
                got = p.acquire(Xt, kind, want=("values",), **kw)["values"]
                assert _path(p.last_timings()) == _path_of(m)
                a, cmu, cv, us = R.evaluate(kind, ref["means"], ref["variances"], **_ref_kw(kw))
                worst = 0.0
                for r in range(NT):
                    f = 1 + us[r] * us[r]
                    sigma = math.sqrt(float(ref["variances"][r]))
                    layer_a = C[name] * EPS * f * ((1 + abs(math.log(sigma))) if kind == R.LOG_EI else abs(a[r]))
                    bound = abs(cmu[r]) * TOL_POST * mu_max + abs(cv[r]) * TOL_POST * var_max + layer_a
                    worst = max(worst, float(abs(mp.mpf(float(got[r])) - a[r]) / bound))
                print("acq.end_to_end.%s: worst error / bound %.3g" % (name, worst))
                M._record("acq.end_to_end.%s" % name, worst, 1.0, acq=name)
                assert worst <= 1.0, (name, maximise, xi, worst)
    finally:
        p.close()


# ---- top-k -----------------------------------------------------------------------------------------------------------------------
def _expect_top(values, k):
    order = np.argsort(-values, kind="stable")
    order = order[~np.isnan(values[order])][:k]
    return np.concatenate([order, np.full(k - len(order), -1, dtype=np.int64)])


def _check_top(got, full, k):
    want = _expect_top(full["values"], k)
    assert np.array_equal(got["top_index"], want), (got["top_index"], want)
    sel = want[want >= 0]
    assert np.array_equal(got["top_values"][:len(sel)], full["values"][sel])
    assert np.array_equal(got["top_dvalues"][:, :len(sel)], full["dvalues"][:, sel])
    assert np.all(np.isnan(got["top_values"][len(sel):])) and np.all(np.isnan(got["top_dvalues"][:, len(sel):]))


@gpu
@pytest.mark.parametrize("key", [("iso", 64, 10, 3), ("proj", 200, 129, 2, 5)], ids=str)
@pytest.mark.parametrize("k", [1, 5, 16, 64])
def test_top_k(k, key):
    Xt = _test_points(key, 200)
    best = float(np.median(_reference(key, 200, False)["means"]))
    p = _problem(key)
    try:
        p.set_timing(2)
        for kind in (R.EI, R.LOG_EI):
            kw = _kw(kind, True, 0.0, best, _floor_of(key))
            full = p.acquire(Xt, kind, **kw)
            got = p.acquire(Xt, kind, top_k=k, **kw)
            assert "acq_select" in p.last_timings()
            assert np.array_equal(got["values"], full["values"]) and np.array_equal(got["dvalues"], full["dvalues"])
            _check_top(got, full, k)
            only = p.acquire(Xt, kind, want=(), top_k=k, **kw)            # nothing of size nt leaves the device
            assert set(only) == {"top_index", "top_values", "top_dvalues"}
            assert all(np.array_equal(only[x], got[x], equal_nan=True) for x in only)
            again = p.acquire(Xt, kind, want=(), top_k=k, **kw)
            assert all(np.array_equal(only[x], again[x], equal_nan=True) for x in only)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_top_k_over_three_chunks_short_lists_and_ties(n, m):
    key = ("iso", n, m, 3)
    best = float(np.median(_reference(key, 200, False)["means"]))
    kw = _kw(R.LOG_EI, False, 0.0, best, _floor_of(key))
    p = _problem(key, chunk_rows=128)
    try:
        Xt = _test_points(key, 300)
        full = p.acquire(Xt, R.LOG_EI, **kw)
        for k in (5, 64):
            _check_top(p.acquire(Xt, R.LOG_EI, want=(), top_k=k, **kw), full, k)
        # nt = 5 < k = 16: the tail is -1 and what lies beyond stays as it was (NaN-filled by the front end)
        few = np.asfortranarray(Xt[:, :5])
        _check_top(p.acquire(few, R.LOG_EI, want=(), top_k=16, **kw), p.acquire(few, R.LOG_EI, **kw), 16)
        # points j and j + 100 identical, here across two chunks: bitwise equal values, the lower index first
        dup = np.asfortranarray(np.concatenate([Xt[:, :100], Xt[:, :100], Xt[:, 200:250]], axis=1))
        fd = p.acquire(dup, R.LOG_EI, **kw)
        assert np.array_equal(fd["values"][:100], fd["values"][100:200])
        got = p.acquire(dup, R.LOG_EI, want=(), top_k=16, **kw)
        _check_top(got, fd, 16)
        idx = got["top_index"]
        pairs = [(a, b) for a, b in zip(idx[:-1], idx[1:]) if a < 100 and b == a + 100]
        assert pairs, idx
    finally:
        p.close()
    q = _problem(key)   # ... and inside one slab of one chunk
    try:
        fd = q.acquire(dup, R.LOG_EI, **kw)
        _check_top(q.acquire(dup, R.LOG_EI, want=(), top_k=16, **kw), fd, 16)
    finally:
        q.close()


@gpu
def test_top_k_with_device_pointers():
    import torch
    key = ("iso", 200, 129, 3)
    D, nt, k = 3, 200, 16
    Xt = _test_points(key, nt)
    best = float(np.median(_reference(key, nt, False)["means"]))
    kw = _kw(R.EI, True, 0.0, best, _floor_of(key))
    p = _problem(key)
    try:
        full = p.acquire(Xt, R.EI, **kw)
        dev = torch.device("cuda:0")
        xt = torch.tensor(np.ascontiguousarray(Xt.T), device=dev)
        dvals = torch.full((nt, D), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        for want, ptrs in (((), {}), (("dvalues",), {"dvalues": dvals.data_ptr()})):
            got = p.acquire(xt.data_ptr(), R.EI, want=want, out_device_ptrs=ptrs, nt=nt, top_k=k, **kw)
            _check_top(got, full, k)
        assert np.array_equal(dvals.cpu().numpy().T, full["dvalues"])
    finally:
        p.close()


# ---- front ends ------------------------------------------------------------------------------------------------------------------
@gpu
def test_functor_acquisition_calc():
    from gpr_amd import cov_se_iso, fitc_gp
    key = ("iso", 200, 65, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    Xt = _test_points(key, NT)
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    q = _problem(key)
    try:
        kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(log_ell=args["log_ell"], log_sf2=args["log_sf2"]))
        inputs = F.Deriv.Inputs.calc(F.Deriv.Inducing.calc(kernel, Zs), Xs)
        trained = F.Deriv.Trained.calc(F.Deriv.Model.calc(inputs, SIGMA2), y)
        kw = dict(maximise=True, best=0.1, xi=0.01, top_k=5)
        want = q.acquire(Xt, "ei", **kw)
        got = F.Eval.Acquisition.calc(trained, F.Eval.Inputs.calc(Xt, inputs.inducing), "ei", **kw)
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    finally:
        q.close()
        GP.close()


@gpu
def test_cpp_mirror_method(tmp_path):
    """gpr::Make_deriv<Cov_se_iso>::FITC::Acquisition::calc (tests/cpp/acquire_check.cpp, built here against the header and the
    library).  The mirror's model state comes from its own sequence of evaluations, so its numbers are held to the layer-B
    form of bound against Problem.acquire's rather than to its bits; the selection is checked against its own values."""
    key = ("iso", 200, 65, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    Xt = _test_points(key, NT)
    d, n = Xs.shape
    m, k = Zs.shape[1], 5
    exe = tmp_path / "acquire_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "acquire_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    floor = _floor_of(key)
    dump = tmp_path / "case.bin"
    with open(dump, "wb") as f:
        np.array([n, d, m, NT, k], dtype=np.int64).tofile(f)
        np.array([args["log_ell"], args["log_sf2"], SIGMA2]).tofile(f)
        np.array([R.EI, 1, 1, 0.1, 0.01, 0.0, floor], dtype=np.float64).tofile(f)
        for a in (Xs, y, Zs, Xt):
            np.asfortranarray(a).T.tofile(f) if a.ndim == 2 else a.tofile(f)
    out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split(" ", 1)[0]: np.array(ln.split()[1:], dtype=np.float64) for ln in out.stdout.splitlines()}
    q = _problem(key)
    try:
        want = q.acquire(Xt, "ei", maximise=True, predictive=True, best=0.1, xi=0.01, var_floor=floor)
        got_v, got_g = vals["values"], vals["dvalues"].reshape(NT, d).T
        M.check_vec("acq.cpp_mirror.values", got_v, want["values"], TOL_POST)
        M.check_vec("acq.cpp_mirror.dvalues", got_g, want["dvalues"], TOL_GRAD)
        idx = vals["top_index"].astype(np.int64)
        assert np.array_equal(idx, _expect_top(got_v, k))
        assert np.array_equal(vals["top_values"], got_v[idx])
        assert np.array_equal(vals["top_dvalues"].reshape(k, d).T, got_g[:, idx])
    finally:
        q.close()


@gpu
@pytest.mark.parametrize("key", [("iso", 200, 20, 4), ("proj", 200, 129, 2, 5)], ids=str)
def test_torch_front_end(key):
    """autograd.acquire: the forward is Problem.acquire's values, the backward g[:, None] * dvalues"""
    import torch
    from gpr_amd.autograd import acquire
    Xt = _test_points(key, NT)
    dev = torch.device("cuda:0")
    p = _problem(key)
    try:
        for kind in ("ei", "log_ei", "pi", "bound"):
            kw = dict(maximise=False, best=0.05, xi=0.01) if kind != "bound" else dict(maximise=False, kappa=KAPPA)
            want = p.acquire(Xt, kind, **kw)
            x = torch.tensor(np.ascontiguousarray(Xt.T), device=dev, requires_grad=True)
            a = acquire(p, x, kind, **kw)
            assert a.shape == (NT,) and a.dtype == torch.float64
            assert np.array_equal(a.detach().cpu().numpy(), want["values"])
            g = torch.linspace(0.5, 2.0, NT, dtype=torch.float64, device=dev)
            (gx,) = torch.autograd.grad((g * a).sum(), x)
            assert np.array_equal(gx.cpu().numpy().T, g.cpu().numpy()[None, :] * want["dvalues"])
            assert np.array_equal(acquire(p, x.detach(), kind, **kw).cpu().numpy(), want["values"])
        with pytest.raises(TypeError):
            acquire(p, x, "ei", maximise=True, top_k=3)
    finally:
        p.close()
