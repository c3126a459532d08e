"""gprhip_predict_input_grad on the device: means, variances and their gradients with respect to the test inputs against the
80-bit reference of tests/predict_grad_ref.py (from the oracle's K_m and K_nm; pinned against central differences of the
oracle's predict_means / predict_variances by tests/test_predict_grad_host.py), on both paths and every kernel width, across
chunks, from a loaded predictor, with offset inputs, the contract of the entry point and the front ends.

Bounds: the largest absolute deviation over the largest absolute reference entry is at most TOL_POST (3e-10) for the means and
the variances and TOL_GRAD (1e-8) for each gradient matrix -- the bounds of tests/test_gpu_parity.py -- asserted through
tests/margins.check_vec with NO conditioning allowance; every case has cond(K_m + jitter I) <= 1e5, computed by eigvalsh of the
oracle's matrix and asserted.  Plain float64 numpy through the explicit-M route deviates from the 80-bit reference by at most
9.3e-13 on a gradient and 3.4e-13 on the variances over these shapes: the reference sits more than 300 x inside both bounds.
Every achieved ratio is recorded (GPR_MARGINS_LOG -> profiles/predict_grad_margins.txt)."""
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
from tests.predict_grad_ref import model_state, predict_grad_from_state
from tests.test_gpu_input_grad import _case
from tests.test_gpu_parity import TOL_GRAD, TOL_POST

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND_MAX = 1e5
SIGMA2 = 0.1
NAMES = ("means", "variances", "dmeans", "dvariances")
BOUNDS = dict(means=TOL_POST, variances=TOL_POST, dmeans=TOL_GRAD, dvariances=TOL_GRAD)

PAIRS = [(1, 1), (15, 3), (64, 10), (65, 64), (200, 65), (333, 128), (200, 129), (500, 256), (300, 257), (700, 300)]
NTS = [1, 15, 64, 65, 200]        # row-tile edges of the kernels (16 per wavefront, 64 per workgroup) and a ragged last block
NT = 65
# every instantiation of predict_grad_kernel<KS4, DT, VAR> (d = 3 is run by the other tests): <1,1> d = 1 | <2,1> d = 8 |
# <4,1> d = 15, 16 | <8,2> d = 17 | <16,4> d = 64, and at (64, 10) the three DT of small_predict_grad_kernel: 4 | 8 | 16
DIMS = [1, 8, 15, 16, 17, 64]
PAIRS_WIDE = [(64, 10), (200, 129)]
PROJ_DIMS = [(5, 2), (17, 16), (40, 3), (70, 4)]


def _test_points(key, nt, seed=0):
    """nt test inputs (D x nt) around the training inputs of the case: training points (drawn with replacement) moved by half
    the spread of the inducing points"""
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    rng = np.random.default_rng(7000 + seed + nt)
    spread = float(np.std(Zs - Zs.mean(1, keepdims=True))) if Zs.shape[1] > 1 else 0.5
    spread = spread if spread > 0 else 0.5
    scale = spread if key[0] != "proj" else float(np.std(Xs)) or 1.0
    return np.asfortranarray(Xs[:, rng.integers(0, n, size=nt)] + 0.5 * scale * rng.normal(size=(D, nt)))


@functools.lru_cache(maxsize=None)
def _state(key):
    Xs, y, Zs, args, ok, cond = _case(*key)
    assert cond <= COND_MAX, (key, cond)
    return model_state(ok, Zs, Xs, y, SIGMA2)


@functools.lru_cache(maxsize=None)
def _reference(key, nt, predictive=True):
    Xs, y, Zs, args, ok, cond = _case(*key)
    ref = predict_grad_from_state(ok, Zs, _state(key), _test_points(key, nt), SIGMA2, predictive)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _problem(key, chunk_rows=0, evaluate=True, **kw):
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    d, m = Zs.shape
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO if key[0] == "iso" else gpr_amd.COV_SE_FAT, n, D, d, m, chunk_rows=chunk_rows)
    p.set_inputs(Xs)
    p.set_targets(y)
    if evaluate:
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, **dict(args, **kw))
    return p


def _hold(what, got, ref, **extra):
    """The four outputs against the reference: printed, then recorded and asserted by tests/margins.py"""
    M.note(_reset=False, **extra)
    for name in NAMES:
        if name not in got:
            continue
        assert got[name].shape == ref[name].shape and np.all(np.isfinite(got[name])), (what, name)
        print("%s.%s: %.3e of the largest entry (bound %.0e)" % (what, name, M.relinf(got[name], ref[name]), BOUNDS[name]))
    for name in NAMES:
        if name in got:
            M.check_vec("%s.%s" % (what, name), got[name], ref[name], BOUNDS[name])


def _path(stages):
    return "engine" if "pg_cov" in stages else "small"


def _check(key, what, nt=NT, path=None, **kw):
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind=key[0], n=key[1], m=key[2], d=key[3], D=Xs.shape[0], nt=nt)
    ref = _reference(key, nt)
    p = _problem(key, **kw)
    try:
        p.set_timing(2)
        got = p.predict_input_grad(_test_points(key, nt))
        stages = p.last_timings()
        assert "pg_grad" in stages, stages
        if path is not None:
            assert _path(stages) == path, (stages, path)
        if _path(stages) == "engine":
            assert "pg_m" in stages and "pg_gemm" in stages, stages
        _hold(what, got, ref, path=_path(stages))
        return got
    finally:
        p.close()


def _path_of(m, d=3):
    return "small" if m <= 64 and d <= 16 else "engine"


# ---- 1. against the reference, both paths and every width ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", PAIRS)
def test_iso_d3_against_the_reference(n, m):
    _check(("iso", n, m, 3), "pgrad.iso", path=_path_of(m))


@gpu
@pytest.mark.parametrize("n,m", [p for p in PAIRS if p[1] <= 64])
def test_small_shapes_on_the_engine_path(n, m, monkeypatch):
    """the shapes of the one-kernel path once more with that path disabled at problem creation"""
    monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")
    _check(("iso", n, m, 3), "pgrad.iso_engine", path="engine")


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("nt", NTS)
def test_row_tile_edges(nt, n, m):
    _check(("iso", n, m, 3), "pgrad.iso_nt%d" % nt, nt=nt, path=_path_of(m))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("d", DIMS)
def test_every_kernel_width(d, n, m):
    _check(("iso", n, m, d), "pgrad.iso_d%d" % d, path=_path_of(m, d))


@gpu
@pytest.mark.parametrize("d", [1, 8, 16])
def test_every_kernel_width_of_the_engine_kernel_at_few_inducing_points(d, monkeypatch):
    monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")
    _check(("iso", 64, 10, d), "pgrad.iso_engine_d%d" % d, path="engine")


@gpu
@pytest.mark.parametrize("n,m", PAIRS)
def test_fat_without_projection(n, m):
    _check(("fat", n, m, 3, 3), "pgrad.fat", path=_path_of(m))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("D,d", PROJ_DIMS)
def test_fat_with_projection(D, d, n, m):
    _check(("proj", n, m, d, D), "pgrad.proj_%d_%d" % (D, d), path=_path_of(m, d))


@gpu
@pytest.mark.parametrize("n,m", [(64, 10), (200, 65)])
def test_heteroskedastic_noise(n, m):
    _check(("proj", n, m, 2, 5, True), "pgrad.proj_het", path=_path_of(m))


@gpu
@pytest.mark.parametrize("n,m", [(64, 10), (200, 129), (700, 300)])
def test_model_state_of_a_variational_evaluation(n, m):
    """(the variational objective changes the evidence and its gradient, not the predictor: the reference is the same)"""
    _check(("iso", n, m, 3), "pgrad.iso_variational", path=_path_of(m), variational=True)


@gpu
@pytest.mark.parametrize("offset", [1e3, 1e5])
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_far_from_the_origin(n, m, offset):
    _check(("iso", n, m, 3, 0, False, offset), "pgrad.iso_offset_%g" % offset, path=_path_of(m))


# ---- 2. several chunks -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_several_chunks(n, m):
    """131072 + 65 test points: two chunks.  Rows are independent, so the reference is computed for the rows around the chunk
    edge, the ends and 200 random rows alone; every output must be finite everywhere."""
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    nt = 131072 + 65
    rng = np.random.default_rng(11)
    Xt = np.asfortranarray(np.tile(_test_points(key, 4099), (1, nt // 4099 + 1))[:, :nt] + 1e-3 * rng.normal(size=(Xs.shape[0], nt)))
    rows = np.unique(np.concatenate([np.arange(0, 70), np.arange(131072 - 70, 131072 + 65), rng.integers(0, nt, size=200)]))
    ref = predict_grad_from_state(ok, Zs, _state(key), np.asfortranarray(Xt[:, rows]), SIGMA2, True)
    M.note(cond=cond, kind="iso", n=n, m=m, d=3, nt=nt)
    p = _problem(key)
    try:
        got = p.predict_input_grad(Xt)
        for name in NAMES:
            assert np.all(np.isfinite(got[name])), name
        _hold("pgrad.chunks", {k: (v[rows] if v.ndim == 1 else v[:, rows]) for k, v in got.items()}, ref)
    finally:
        p.close()


# ---- 3. loaded predictor ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_loaded_predictor(n, m):
    """load_predictor with the oracle's coefficients and factors, no training inputs; without factors dvariances is refused
    (GPRHIP_ESTATE) and dmeans alone works"""
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind="iso", n=n, m=m, d=3, nt=NT)
    out = O.evaluate(ok, Zs, Xs, y, SIGMA2, want_grad=False, keep=True)
    model = out["model"]
    ref = _reference(key, NT)
    Xt = _test_points(key, NT)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, 3, 3, m)
    try:
        p.load_predictor(sigma2=SIGMA2, inducing=Zs, coeffs=out["coeffs"],
                         co_variance_coeffs=(np.triu(model["inducing"]["chol_km"]), np.triu(model["r_mat"])), **args)
        _hold("pgrad.loaded", p.predict_input_grad(Xt), ref)
        p.load_predictor(sigma2=SIGMA2, inducing=Zs, coeffs=out["coeffs"], **args)
        for want in (("dvariances",), ("variances",), NAMES):
            with pytest.raises(gpr_amd.GprHipError) as e:
                p.predict_input_grad(Xt, want=want)
            assert e.value.status == _lib.ESTATE
        _hold("pgrad.loaded_means_only", p.predict_input_grad(Xt, want=("means", "dmeans")), ref)
    finally:
        p.close()


# ---- 4. the contract of the entry point ------------------------------------------------------------------------------------------
def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


@gpu
@pytest.mark.parametrize("key", [("proj", 64, 10, 2, 5), ("proj", 200, 129, 2, 5), ("iso", 200, 129, 3)], ids=str)
def test_host_and_device_outputs_agree_and_padding_rows_stay(key):
    import torch
    D = _case(*key)[0].shape[0]
    Xt = _test_points(key, NT)
    p = _problem(key)
    try:
        host = p.predict_input_grad(Xt)
        dev = torch.device("cuda:0")
        xt = torch.tensor(np.ascontiguousarray(Xt.T), device=dev)
        outs = {"means": torch.full((NT,), float("nan"), dtype=torch.float64, device=dev),
                "variances": torch.full((NT,), float("nan"), dtype=torch.float64, device=dev),
                "dmeans": torch.full((NT, D), float("nan"), dtype=torch.float64, device=dev),
                "dvariances": torch.full((NT, D), float("nan"), dtype=torch.float64, device=dev)}
        torch.cuda.synchronize()
        assert p.predict_input_grad(xt.data_ptr(), out_device_ptrs={k: v.data_ptr() for k, v in outs.items()}, nt=NT) is None
        for k in NAMES:
            got = outs[k].cpu().numpy()
            assert np.array_equal(got if got.ndim == 1 else got.T, host[k]), k
        wide = p.predict_input_grad(Xt, ldg=D + 3)
        for k in ("dmeans", "dvariances"):
            assert wide[k].shape == (D + 3, NT) and np.array_equal(wide[k][:D], host[k]) and np.all(np.isnan(wide[k][D:]))
        assert np.array_equal(wide["means"], host["means"]) and np.array_equal(wide["variances"], host["variances"])
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("key", [("iso", 64, 10, 3), ("iso", 200, 129, 3), ("proj", 200, 129, 2, 5)], ids=str)
def test_every_null_combination_predictive_and_repeatability(key):
    """Every non-empty subset of the four outputs gives the bits of the full request -- a mean-only one without G and its
    product --; `predictive` moves the variances by exactly sigma2 and no gradient bit; two runs are bit-identical;
    gprhip_predict before and after returns identical bits, and its values agree to TOL_POST."""
    Xt = _test_points(key, NT)
    p = _problem(key)
    try:
        before = p.predict(Xt)
        p.set_timing(2)
        full = p.predict_input_grad(Xt)
        assert _same(full, p.predict_input_grad(Xt))
        for mask in range(1, 16):
            want = tuple(nm for i, nm in enumerate(NAMES) if mask >> i & 1)
            got = p.predict_input_grad(Xt, want=want)
            stages = p.last_timings()
            assert set(got) == set(want)
            if not {"variances", "dvariances"} & set(want):
                assert "pg_gemm" not in stages and "pg_cov" not in stages and "pg_m" not in stages, (want, stages)
            for nm in want:
                assert np.array_equal(got[nm], full[nm]), (want, nm)
        latent = p.predict_input_grad(Xt, predictive=False)
        assert np.array_equal(latent["variances"] + SIGMA2, full["variances"])
        for nm in ("means", "dmeans", "dvariances"):
            assert np.array_equal(latent[nm], full[nm]), nm
        after = p.predict(Xt)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        M.check_vec("pgrad.means_vs_predict", full["means"], before[0], TOL_POST)
        M.check_vec("pgrad.variances_vs_predict", full["variances"], before[1], TOL_POST)
    finally:
        p.close()


@gpu
def test_m_is_formed_once_per_model_state():
    key = ("iso", 200, 129, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    Xt = _test_points(key, NT)
    p = _problem(key)
    try:
        p.set_timing(2)
        first = p.predict_input_grad(Xt)
        assert "pg_m" in p.last_timings()
        again = p.predict_input_grad(Xt)
        assert "pg_m" not in p.last_timings() and _same(first, again)
        p.eval(want_grad=False, sigma2=0.25, inducing=Zs, **args)
        other = p.predict_input_grad(Xt)
        assert "pg_m" in p.last_timings() and not np.array_equal(other["dvariances"], first["dvariances"])
    finally:
        p.close()


def _raw(p, Xt, outs, ld=None, ldg=None, on_device=0, nt=None):
    D = Xt.shape[0]
    vp = ctypes.c_void_p
    ptrs = [vp(outs[k].ctypes.data) if outs.get(k) is not None else vp(None) for k in NAMES]
    return p._lib.gprhip_predict_input_grad(p._handle(), vp(Xt.ctypes.data), D if ld is None else ld,
                                            Xt.shape[1] if nt is None else nt, 1, *ptrs, D if ldg is None else ldg, on_device)


@gpu
def test_refusals_leave_the_next_correct_call_working():
    key = ("fat", 64, 10, 3, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    m = Zs.shape[1]
    Xt = _test_points(key, NT)
    ref = _reference(key, NT)
    outs = {"means": np.full(NT, np.nan), "variances": np.full(NT, np.nan), "dmeans": np.full((D, NT), np.nan, order="F"),
            "dvariances": np.full((D, NT), np.nan, order="F")}
    untouched = lambda: all(np.all(np.isnan(v)) for v in outs.values())
    p = _problem(key)
    f32 = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m, precision=gpr_amd.F32_BULK)
    empty = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m)
    wide = gpr_amd.Problem(gpr_amd.COV_SE_ISO, 40, 65, 65, 5)
    try:
        p.set_timing(2)
        assert _raw(p, Xt, {}) == _lib.EBADARG                                    # all four outputs NULL
        assert _raw(p, Xt, outs, ld=D - 1) == _lib.EBADARG                        # host: ld < D
        assert _raw(p, Xt, outs, ldg=D - 1) == _lib.EBADARG                       # host: ldg < D
        assert _raw(p, Xt, outs, ld=D + 1, on_device=1) == _lib.EBADARG           # device: ld != D
        assert _raw(p, Xt, outs, nt=0) == _lib.EBADARG
        assert untouched() and p.last_timings() == {}                             # nothing was enqueued
        # a multiscale model state
        lms = np.asfortranarray(np.random.default_rng(3).uniform(-1.0, 0.5, size=(D, m)))
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, log_multiscales_m05=lms, **args)
        assert _raw(p, Xt, outs) == _lib.EBADARG and untouched()
        # after eval_targets: the means and their gradient are refused, the variance part is served
        p.set_targets_many(np.asfortranarray(np.stack([y, 2.0 * y], axis=1)))
        p.eval_targets(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        assert _raw(p, Xt, outs) == _lib.ESTATE
        assert _raw(p, Xt, {"dmeans": outs["dmeans"]}) == _lib.ESTATE and untouched()
        _hold("pgrad.after_eval_targets", p.predict_input_grad(Xt, want=("variances", "dvariances")), ref)
        # fp32-bulk problem, no model, 65 point dimensions
        assert _raw(f32, Xt, outs) == _lib.EBADARG
        assert _raw(empty, Xt, outs) == _lib.ESTATE
        rng = np.random.default_rng(5)
        Xw, Zw = np.asfortranarray(rng.normal(size=(65, 40))), np.asfortranarray(rng.normal(size=(65, 5)))
        wide.set_inputs(Xw)
        wide.set_targets(rng.normal(size=40))
        wide.eval(want_grad=False, log_ell=float(np.log(8.0)), log_sf2=0.0, sigma2=SIGMA2, inducing=Zw)
        ow = {"dmeans": np.full((65, 4), np.nan, order="F")}
        assert _raw(wide, np.asfortranarray(Xw[:, :4]), ow) == _lib.EBADARG and np.all(np.isnan(ow["dmeans"]))
        assert untouched()
        # the next correct call works
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        assert _raw(p, Xt, outs) == _lib.OK
        _hold("pgrad.after_refusals", outs, ref)
    finally:
        for q in (p, f32, empty, wide):
            q.close()


# ---- 5. front ends ---------------------------------------------------------------------------------------------------------------
@gpu
def test_functor_calc_input_gradient():
    """Means.calc_input_gradient / Variances.calc_input_gradient give Problem.predict_input_grad's matrices bit for bit"""
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
        model = F.Deriv.Model.calc(inputs, SIGMA2)
        trained = F.Deriv.Trained.calc(model, y)
        want = q.predict_input_grad(Xt)
        tin = F.Eval.Inputs.calc(Xt, inputs.inducing)
        dm = F.Eval.Means.calc_input_gradient(F.Eval.Mean_predictor.calc_trained(trained), tin)
        dv = F.Eval.Variances.calc_input_gradient(F.Eval.Co_variance_predictor.calc_model(model), SIGMA2, tin)
        assert np.array_equal(dm, want["dmeans"]) and np.array_equal(dv, want["dvariances"])
    finally:
        q.close()
        GP.close()


@gpu
def test_cpp_mirror_methods(tmp_path):
    """gpr::Make<Cov_se_iso>::Means::calc_input_gradient / Variances::calc_input_gradient (tests/cpp/predict_grad_check.cpp,
    built here with g++ against the header and the library) against the reference, to the bounds of every other case"""
    key = ("iso", 200, 65, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    Xt = _test_points(key, NT)
    d, n = Xs.shape
    m = Zs.shape[1]
    exe = tmp_path / "predict_grad_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "predict_grad_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    dump = tmp_path / "case.bin"
    with open(dump, "wb") as f:
        np.array([n, d, m, NT], dtype=np.int64).tofile(f)
        np.array([args["log_ell"], args["log_sf2"], SIGMA2]).tofile(f)
        for a in (Xs, y, Zs, Xt):
            np.asfortranarray(a).T.tofile(f) if a.ndim == 2 else a.tofile(f)
    out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split(" ", 1)[0]: np.array(ln.split()[1:], dtype=np.float64) for ln in out.stdout.splitlines()}
    q = _problem(key)
    try:
        # (the mirror's state comes from its own sequence of evaluations -- a gradient evaluation, then the model's --, not
        # from the one evidence-only evaluation here: the matrices are held to the reference, the means' also to these bits)
        want = q.predict_input_grad(Xt)
        got = {"dmeans": vals["dmeans"].reshape(NT, d).T, "dvariances": vals["dvariances"].reshape(NT, d).T}
        M.note(cond=cond, kind="iso", n=n, m=m, d=d, nt=NT)
        _hold("pgrad.cpp_mirror", got, _reference(key, NT))
        assert np.array_equal(got["dmeans"], want["dmeans"])
    finally:
        q.close()


@gpu
@pytest.mark.parametrize("key", [("iso", 200, 20, 4), ("proj", 200, 129, 2, 5)], ids=str)
def test_torch_front_end(key):
    """autograd.predict: the backward of mean.sum() and of var.sum() equals the C ABI's matrices, the gradient of an upper
    confidence bound the chain-rule combination of the library's outputs, and a second derivative raises"""
    import torch
    from gpr_amd.autograd import predict
    Xt = _test_points(key, NT)
    dev = torch.device("cuda:0")
    p = _problem(key)
    try:
        want = p.predict_input_grad(Xt)
        x = torch.tensor(np.ascontiguousarray(Xt.T), device=dev, requires_grad=True)
        mean, var = predict(p, x)
        assert mean.shape == (NT,) and var.shape == (NT,) and mean.dtype == torch.float64
        assert np.array_equal(mean.detach().cpu().numpy(), want["means"])
        assert np.array_equal(var.detach().cpu().numpy(), want["variances"])
        (gm,) = torch.autograd.grad(mean.sum(), x, retain_graph=True)
        (gv,) = torch.autograd.grad(var.sum(), x, retain_graph=True)
        assert np.array_equal(gm.cpu().numpy().T, want["dmeans"]) and np.array_equal(gv.cpu().numpy().T, want["dvariances"])
        (gu,) = torch.autograd.grad((mean + 2.0 * torch.sqrt(var)).sum(), x)
        chain = want["dmeans"] + (1.0 / np.sqrt(want["variances"]))[None, :] * want["dvariances"]
        err = M.relinf(gu.cpu().numpy().T, chain)
        print("UCB gradient against the chain rule of the library's outputs: %.3e" % err)
        assert err <= 1e-14, err
        latent = predict(p, x.detach(), predictive=False)[1]
        assert float(torch.max(torch.abs(latent + SIGMA2 - var.detach()))) <= 1e-15
        x2 = torch.tensor(np.ascontiguousarray(Xt.T), device=dev, requires_grad=True)
        mean2, _ = predict(p, x2)
        (g2,) = torch.autograd.grad(mean2.sum(), x2, create_graph=True)
        with pytest.raises(RuntimeError):
            g2.sum().backward()
    finally:
        p.close()
