"""Every entry of the posterior calls -- gprhip_predict, gprhip_predict_targets, gprhip_covariances, gprhip_cov_samples,
gprhip_train_stats -- against tests/posterior_ref.py: the 80-bit contraction of the covariances at the test points with the
DEVICE'S OWN t, U^-1 and R~^-1 of the same model state (debug_fetch "t", "uinv", "rinv"), within the derived running-error bound of
that module.  The factors are pinned elsewhere (tests/test_gpu_factors.py, tests/test_gpu_row_operands.py); here conditioning
never enters: no oracle, no Problem.condition(), no tolerance in this file.  tests/test_posterior_host.py pins the reference
and the bound on the CPU over the same list of cases.

Shapes are the smallest at which each kernel can go wrong (read off the launch code):
  small_predict_kernel<4 | 8 | 16>  64 test points per workgroup, m <= 64, d <= 16        nt 1, 63, 64, 65, 200; m 1, 16, 17, 64
  do_predict's engine path          cov_cross_kernel 32 rows per block, row_sumsq_dot_kernel 4 rows per workgroup, 128-row padding
                                    of the engine operands, variance_combine_kernel 256 per block: nt 1, 3, 4, 5, 127 .. 129, 255 .. 257;
                                    m 65, 128, 129, 256, 257 (a last live column in a new 128-block), m = 17 with the one-kernel paths off
  do_covariances                    the same edges in nt, and nt 15, 16, 17
  do_cov_samples                    nt x nt factorisation with m_real = nt in a partly live block; sym_from_upper_kernel 16 x 16 tiles
  do_train_stats                    residual_stats_kernel 256 per block, row chunks of 128 and 256
Test points are a fixed mix: training inputs themselves, inducing points themselves (lifted through the pseudo-inverse of a
projection), training inputs moved half a spread, and points so far off that every K entry underflows -- there the mean must
be +0.0 and the variance (sf2 - 0) + add bit for bit.  sigma2 = 0.1; one sigma2 = 1e-4 case per path puts variances at the
training inputs near 1e-4 sf2.
Most models have log_sf2 = 0 (tests/util.py::factor_case); one case per call -- predict on either path, covariances,
predict_targets, train_stats -- runs at log_sf2 = 0.3, so that a dropped or squared sf2 and the |log sf2| term of kappa show.
Which path a posterior call takes is INFERRED, not asserted: do_predict has no stage names, so predict_path() restates its
predicate (gprhip.hip: small_path && !f32 && m <= 64 && d <= 16 && no multiscales); only the evaluation's path is read off
last_timings().  The multiscale models evaluate on the small path and predict through cov_cross_ms_kernel and the engine.
The fetched U^-1 and R~^-1 come with zeros below the diagonal because the fetch writes them there; what the device holds
below the diagonal is seen through the outputs only.
Left out: sharded prediction across devices; batch lanes (tests/test_gpu_batch.py::test_lane_problems_serve_predictions already
holds a lane's predict to the single problem's bit for bit).
"""
import collections
import ctypes
import functools
import math

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import margins as M
from tests import posterior_ref as R
from tests.test_gpu_f32_kernels import host_centroid
from tests.test_gpu_factors import factor_ratio
from tests.util import factor_case, synth
from tests.util import taken as _taken

gpu = pytest.mark.gpu

SIGMA2 = 0.1
JITTER = 1e-6

Case = collections.namedtuple("Case", "path kind n m d D env chunk sigma2 variational f32 log_sf2",
                              defaults=(0, (), 0, SIGMA2, False, False, 0.0))
FORCED = (("GPRHIP_SMALL_PATH", "0"), ("GPRHIP_MID_PATH", "0"))
N = 200
LOG_SF2 = 0.3

NT_SMALL = (1, 63, 64, 65, 200)
NT_ENGINE = (1, 3, 4, 5, 127, 128, 129, 255, 256, 257)
NT_COV = (1, 15, 16, 17, 127, 128, 129, 257)

SMALL = [Case("small", "iso", N, m, 3) for m in (1, 16, 17, 64)] + [Case("small", "iso", N, 17, d) for d in (1, 4, 5, 8, 9, 16)] + \
    [Case("small", "fat_proj_het", N, 17, 3, 5), Case("small", "fat_het", N, 17, 3), Case("small", "iso", N, 17, 3, sigma2=1e-4),
     Case("small", "iso", N, 17, 3, log_sf2=LOG_SF2)]
ENGINE = [Case("mid", "iso", N, m, 3) for m in (65, 128, 129, 256)] + [Case("engine", "iso", N, 257, 3)] + \
    [Case("engine", "iso", N, 17, 3, env=FORCED), Case("engine", "iso", N, 129, 17), Case("engine", "iso", N, 129, 65),
     Case("mid", "fat_proj_het", N, 129, 3, 5), Case("mid", "fat_het", N, 129, 3), Case("small", "fat_ms", N, 17, 3),
     Case("small", "fat_proj_ms", N, 17, 3, 5), Case("small", "fat_het_ms", N, 17, 3), Case("small", "fat_proj_het_ms", N, 17, 3, 5),
     Case("engine", "fat_proj_het_ms", N, 17, 3, 5, env=FORCED), Case("mid", "iso", N, 129, 3, sigma2=1e-4),
     Case("mid", "iso", N, 129, 3, log_sf2=LOG_SF2),
     Case("mid", "iso", N, 129, 3, variational=True), Case("engine", "iso", N, 257, 3, variational=True)]
CHUNK128 = Case("mid", "iso", 300, 129, 3, chunk=128)
F32 = [Case("engine", "iso", N, m, d, f32=True) for m in (129, 257) for d in (3, 17)]
COV = [Case("small", "iso", N, 17, 3), Case("mid", "iso", N, 129, 3), Case("engine", "iso", N, 257, 3),
       Case("small", "fat_ms", N, 17, 3), Case("mid", "fat_proj_het", N, 129, 3, 5),
       Case("engine", "fat_proj_het_ms", N, 17, 3, 5, env=FORCED), Case("mid", "iso", N, 129, 3, log_sf2=LOG_SF2)]
STATS = [Case(path, "iso", n, m, 3, chunk=chunk) for path, m in (("small", 17), ("mid", 65), ("engine", 257))
         for n, chunk in ((1, 0), (255, 0), (256, 0), (257, 0), (700, 256), (300, 128))] + \
    [Case("mid", "iso", 257, 65, 3, log_sf2=LOG_SF2)]
STATS_F32 = [Case("engine", "iso", N, m, d, f32=True) for m in (129, 257) for d in (3, 17)]
LOADED = [Case("small", "iso", N, 17, 3), Case("mid", "iso", N, 129, 3), Case("engine", "fat_het", N, 273, 3)]
TARGETS = [(Case("engine", "iso", N, m, 3), k) for m in (17, 129) for k in (1, 2, 16)] + [(Case("engine", "fat_proj_het", N, 17, 3, 5), 2),
                                                                                         (Case("engine", "iso", N, 17, 3, log_sf2=LOG_SF2), 2)]
HOST_CASES = SMALL + ENGINE + [CHUNK128] + F32 + COV + STATS + STATS_F32 + LOADED + [c for c, k in TARGETS]   # tests/test_posterior_host.py


def case_id(c):
    s = "%s%s-n%d-m%d-d%d" % (c.path + "-" if c.path else "", c.kind, c.n, c.m, c.d)
    s += ("-D%d" % c.D if c.D else "") + ("-forced" if c.env else "") + ("-c%d" % c.chunk if c.chunk else "")
    s += ("-s%g" % c.sigma2 if c.sigma2 != SIGMA2 else "") + ("-var" if c.variational else "") + ("-f32" if c.f32 else "")
    return s + ("-lsf%g" % c.log_sf2 if c.log_sf2 else "")


def predict_path(c):
    """The path do_predict takes, restated from its predicate (inferred, not asserted: the call has no stage names)"""
    forced = ("GPRHIP_SMALL_PATH", "0") in c.env
    return "small" if (c.m <= 64 and c.d <= 16 and "ms" not in c.kind and not c.f32 and not forced) else "engine"


@functools.lru_cache(maxsize=None)
def _factor_case(kind, n, m, d, D):
    return factor_case(kind, n, m, d, D or None)


def data(c):
    X, y, Z, args, ok, cond = _factor_case(c.kind, c.n, c.m, c.d, c.D)
    return X, y, Z, (dict(args, log_sf2=c.log_sf2) if c.log_sf2 else args)


def hypers_of(c, args):
    """keyword arguments of posterior_ref.geometry"""
    return dict(iso=c.kind == "iso", log_sf2=args["log_sf2"], log_ell=args.get("log_ell", 0.0), tproj=args.get("tproj"),
                log_ms=args.get("log_multiscales_m05"), bulk32=c.f32)


def points_of(X, Z, args, nt):
    """The fixed mix of points() for any training inputs X (D x n), inducing points Z (d x m) and keyword arguments of
    Problem.eval: (test inputs D x nt, mask of the far points)."""
    n, (d, m) = X.shape[1], Z.shape
    tp = args.get("tproj")
    lift = (lambda p: p) if tp is None else (lambda p: tp @ np.linalg.solve(tp.T @ tp, p))
    rng = np.random.default_rng(77 + nt)
    ie2 = np.exp(-2.0 * args.get("log_ell", 0.0))
    reach = np.sqrt(2.0 * 900.0 * 3.0 / ie2) + 2.0 * float(np.max(np.abs(Z)))      # exponent below -800 with multiscales <= 2.2 too
    Xt = np.empty((X.shape[0], nt))
    far = np.zeros(nt, dtype=bool)
    for i in range(nt):
        kind = i % 5
        if kind == 0:
            Xt[:, i] = X[:, (7 * i) % n]
        elif kind == 1:
            Xt[:, i] = lift(Z[:, (3 * i) % m])
        elif kind == 2:
            Xt[:, i] = X[:, (5 * i) % n] + 0.5 * X.std() * rng.normal(size=X.shape[0]) / np.sqrt(X.shape[0])
        elif kind == 4:
            Xt[:, i] = lift(Z[:, (11 * i) % m] + 0.5 * Z.std() * rng.normal(size=d) / np.sqrt(d))
        else:
            e = np.zeros(d)
            e[i % d] = reach * (1.0 + 0.1 * rng.uniform())
            Xt[:, i] = lift(Z[:, i % m] + e)
            far[i] = True
    Xt = np.asfortranarray(Xt)
    Xt.setflags(write=False)
    return Xt, far


@functools.lru_cache(maxsize=None)
def points(c, nt):
    """(test inputs D x nt, mask of the far points): entry i is of kind i mod 5 -- a training input, an inducing point,
    a training input moved half a spread, a point beyond the reach of every inducing point, an inducing point moved half a
    spread.  The period 5 walks every kind through every position of the 4-, 16-, 64- and 256-row blocks of the kernels."""
    X, y, Z, args = data(c)
    assert X.shape[1] == c.n and Z.shape == (c.d, c.m)
    return points_of(X, Z, args, nt)


def _frozen(g):
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


@functools.lru_cache(maxsize=8)
def geometry(c, nt):
    """The 80-bit covariances at the test points of a case and their weights: device-independent, shared by the tests"""
    X, y, Z, args = data(c)
    return _frozen(R.geometry(points(c, nt)[0], Z, **hypers_of(c, args)))


Operands = collections.namedtuple("Operands", "t uinv rinv")


def fetch_operands(p, c, t=None):
    uinv, rinv = p.debug_fetch_matrix("uinv"), p.debug_fetch_matrix("rinv")
    if c.f32:   # the round-to-nearest copies launch_to_float makes
        uinv, rinv = uinv.astype(np.float32), rinv.astype(np.float32)
    return Operands(p.debug_fetch("t") if t is None else t, uinv, rinv)


def _cov(kind):
    return gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT


def open_problem(c, monkeypatch, n=None):
    for k, val in c.env:
        monkeypatch.setenv(k, val)        # read when the problem is created
    X, y, Z, args = data(c)
    return gpr_amd.Problem(_cov(c.kind), c.n if n is None else n, X.shape[0], c.d, c.m, chunk_rows=c.chunk,
                           precision=gpr_amd.F32_BULK if c.f32 else gpr_amd.F64)


def evaluated(c, monkeypatch):
    """A problem after one evaluation on the path the case names"""
    X, y, Z, args = data(c)
    p = open_problem(c, monkeypatch)
    p.set_inputs(X)
    p.set_targets(y)
    p.set_timing(2)
    ev = p.eval(sigma2=c.sigma2, inducing=Z, variational=c.variational, want_grad=False, **args)
    assert _taken(set(p.last_timings())) == c.path, (case_id(c), sorted(p.last_timings()))
    p.set_timing(0)
    return p, ev


def hold(label, what, got, ref, bound):
    """Every entry within its bound; the worst ratio is recorded first."""
    got = np.asarray(got)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (label, what, got.shape, ref.shape)
    r, at = R.ratio(got, ref, bound)
    M.record("post." + what, r, 1.0, case=label, scale=float(np.max(np.abs(ref))) if ref.size else 0.0,
             bound=float(np.max(bound)) if ref.size else 0.0)
    assert r <= 1.0, "%s %s: entry %d: got %r, reference %r, bound %.3e (x %.2f)" % (
        label, what, at, float(got.ravel()[at]), float(ref.ravel()[at]), float(np.ravel(bound)[at]), r)
    return r


def predict_raw(p, Xt, predictive, want_means, want_vars):
    """gprhip_predict with either output left out"""
    nt = Xt.shape[1]
    mu = np.full(nt, np.nan) if want_means else None
    var = np.full(nt, np.nan) if want_vars else None
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None
    _lib.check(p._lib.gprhip_predict(p._handle(), ptr(Xt), Xt.shape[0], nt, int(predictive), ptr(mu), ptr(var)))
    return mu, var


def check_predict_at(p, Xt, far, g, sigma2, log_sf2, ops, label, means=True, predict=None):
    """check_predict at given test points Xt with their 80-bit geometry g, on whatever state `ops` was fetched from;
    predict(Xt, predictive, want_means, want_vars) stands in for the device where given"""
    predict = predict or (lambda *a: predict_raw(p, *a))
    sf2 = math.exp(log_sf2)        # the host's libm, as the library's exp(log_sf2)
    ch = R.chain(g, ops.uinv, ops.rinv)
    mu_ref, mu_b = R.mean(g, ops.t) if means else (None, None)
    for predictive in (False, True):
        add = sigma2 if predictive else 0.0
        var_ref, var_b = R.variance(g, ch, add)
        for want_m, want_v in ((means, True), (False, True)) + (((True, False),) if means else ()):
            mu, var = predict(Xt, predictive, want_m, want_v)
            if want_m:
                hold(label, "mean", mu, mu_ref, mu_b)
                assert np.all(mu[far] == 0.0) and not np.any(np.signbit(mu[far])), label
            if want_v:
                hold(label, "variance", var, var_ref, var_b)
                assert np.all(var[far] == (sf2 - 0.0) + add), label
    return var_ref, var_b


def check_predict(p, c, nt, ops, label, means=True):
    """means, variances (predictive and not; together and each alone) at the fixed mix of nt test points"""
    Xt, far = points(c, nt)
    return check_predict_at(p, Xt, far, geometry(c, nt), c.sigma2, c.log_sf2, ops, "%s-nt%d" % (label, nt), means)


# ---- predict ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", SMALL + ENGINE + F32, ids=case_id)
def test_every_mean_and_variance_against_the_80_bit_contraction_of_the_device_operands(c, monkeypatch):
    p, ev = evaluated(c, monkeypatch)
    try:
        Xt = points(c, 65)[0]
        before = p.predict(Xt)
        ops = fetch_operands(p, c)
        after = p.predict(Xt)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])    # a fetch only copies
        assert np.array_equal(ops.t, ev.coeffs)
        for nt in (NT_SMALL if predict_path(c) == "small" else (5, 129) if c.f32 else NT_ENGINE):
            check_predict(p, c, nt, ops, case_id(c))
    finally:
        p.close()


@gpu
def test_enlarged_prediction_buffers_then_a_smaller_call(monkeypatch):
    """chunk_rows = 128: nt = 300 exceeds the training chunk (do_predict allocates predA / predB of 1024 rows), nt = 100 after
    it runs in the training chunk's buffers again"""
    c = CHUNK128
    p, ev = evaluated(c, monkeypatch)
    try:
        ops = fetch_operands(p, c)
        for nt in (300, 100, 300):
            check_predict(p, c, nt, ops, case_id(c))
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("c", [Case("small", "iso", N, 17, 3), Case("mid", "iso", N, 65, 3)], ids=case_id)
def test_the_chunk_crossing_at_131072_test_points(c, monkeypatch):
    """nt = 131072 + 65: two chunks.  The reference is formed on the rows [0, 256) and [131072 - 128, 131072 + 65) only; the bulk is
    held by equality with a second call on the same points in pieces of 4096."""
    nt = 131072 + 65
    base, far = points(c, 512)
    Xt = np.asfortranarray(np.tile(base, (1, -(-nt // 512)))[:, :nt])
    rows = np.r_[0:256, 131072 - 128:nt]
    X, y, Z, args = data(c)
    p, ev = evaluated(c, monkeypatch)
    try:
        ops = fetch_operands(p, c)
        mu, var = p.predict(Xt, predictive=False)
        g = R.geometry(Xt[:, rows], Z, **hypers_of(c, args))
        mu_ref, mu_b = R.mean(g, ops.t)
        var_ref, var_b = R.variance(g, R.chain(g, ops.uinv, ops.rinv), 0.0)
        hold(case_id(c) + "-cross", "mean", mu[rows], mu_ref, mu_b)
        hold(case_id(c) + "-cross", "variance", var[rows], var_ref, var_b)
        for lo in range(0, nt, 4096):
            m2, v2 = p.predict(np.asfortranarray(Xt[:, lo:lo + 4096]), predictive=False)
            assert np.array_equal(m2, mu[lo:lo + 4096]) and np.array_equal(v2, var[lo:lo + 4096]), lo
    finally:
        p.close()


@gpu
def test_a_jitter_dominated_model_holds_the_same_bound():
    """d = 1, m = 176 on a line (tests/test_gpu_parity.py::test_mean_coefficients_against_an_80_bit_evaluation needs 3e-7 against
    the oracle there): with the device's own t, U^-1, R~^-1 the bound holds unchanged."""
    n, m, d, log_ell = 2630, 176, 1, -0.0496
    X, y, Z = synth(5000 + n, n, m, d)
    Xt = np.asfortranarray(np.random.default_rng(6).normal(size=(d, 200)))
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=1024)
    try:
        p.set_inputs(X)
        p.set_targets(y)
        p.eval(log_ell=log_ell, log_sf2=0.1, sigma2=0.05, inducing=Z, want_grad=False)
        t, uinv, rinv = p.debug_fetch("t"), p.debug_fetch_matrix("uinv"), p.debug_fetch_matrix("rinv")
        mu, var = p.predict(Xt, predictive=False)
    finally:
        p.close()
    g = R.geometry(Xt, Z, iso=True, log_sf2=0.1, log_ell=log_ell)
    mu_ref, mu_b = R.mean(g, t)
    var_ref, var_b = R.variance(g, R.chain(g, uinv, rinv), 0.0)
    hold("jitter-dominated", "mean", mu, mu_ref, mu_b)
    hold("jitter-dominated", "variance", var, var_ref, var_b)


# ---- loaded predictor ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", LOADED, ids=case_id)
def test_a_loaded_predictor_against_its_own_operands(c, monkeypatch):
    X, y, Z, args = data(c)
    p, ev = evaluated(c, monkeypatch)
    try:
        U, Rm = p.co_variance_coeffs()
    finally:
        p.close()
    q = open_problem(c, monkeypatch, n=64)     # a fresh problem that never sees training data
    try:
        q.load_predictor(coeffs=ev.coeffs, sigma2=c.sigma2, inducing=Z, **args)
        with pytest.raises(_lib.GprHipError) as err:
            q.debug_fetch_matrix("uinv")
        assert err.value.status == _lib.ESTATE and "co-variance" in str(err.value)
        q.load_predictor(coeffs=ev.coeffs, co_variance_coeffs=(U, Rm), sigma2=c.sigma2, inducing=Z, **args)
        ops = fetch_operands(q, c)
        assert np.array_equal(ops.t, ev.coeffs)
        for nt in (1, 129):
            check_predict(q, c, nt, ops, case_id(c) + "-loaded")
        check_covariances(q, c, 17, ops, case_id(c) + "-loaded")
    finally:
        q.close()


# ---- predict_targets ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,k", TARGETS, ids=lambda v: case_id(v) if isinstance(v, Case) else "k%d" % v)
def test_every_mean_of_every_target_column(c, k, monkeypatch):
    X, y, Z, args = data(c)
    Y = np.asfortranarray(y[:, None] * (1.0 + 0.25 * np.arange(k))[None, :] + 0.1 * np.random.default_rng(k).normal(size=(c.n, k)))
    p = open_problem(c, monkeypatch)
    try:
        p.set_inputs(X)
        p.set_targets_many(Y)
        p.set_timing(2)
        ev = p.eval_targets(sigma2=c.sigma2, inducing=Z, want_grad=False, **args)
        assert "p1_targets" in p.last_timings()
        ops = fetch_operands(p, c, t=ev.coeffs)      # (the factors of a several-target evaluation are fetched as any other's)
        for nt in (1, 129):
            Xt, far = points(c, nt)
            g = geometry(c, nt)
            mu_ref, mu_b = R.mean(g, ev.coeffs)
            mu = p.predict_targets(Xt)
            hold("%s-k%d-nt%d" % (case_id(c), k, nt), "target_means", mu, mu_ref, mu_b)
            assert np.all(mu[far] == 0.0) and not np.any(np.signbit(mu[far]))
            check_predict(p, c, nt, ops, case_id(c) + "-targets", means=False)
    finally:
        p.close()


# ---- covariances, cov_samples -------------------------------------------------------------------------------------------------
def check_covariances_at(p, Xt, g, sigma2, ops, label):
    """check_covariances at given test points Xt with their 80-bit geometry g, on whatever state `ops` was fetched from"""
    ch = R.chain(g, ops.uinv, ops.rinv)
    out = {}
    for kind in ("FITC", "FIC"):
        for predictive in (False, True):
            add = sigma2 if predictive else 0.0
            cov = p.covariances(Xt, kind=kind, predictive=predictive)
            ref, bound = R.covariances(g, ch, kind, add)
            hold(label, kind + (".predictive" if predictive else ""), cov, ref, bound)
            assert np.array_equal(cov, cov.T), (label, kind)
            out[kind, predictive] = cov
    var_ref, var_b = R.variance(g, ch, 0.0)
    _, var = p.predict(Xt, predictive=False)
    cref, cb = R.covariances(g, ch, "FITC", 0.0)
    gap = np.abs(np.diag(out["FITC", False]) - var)
    M.record("post.fitc_diag_vs_variance", float(np.max(gap / (np.diag(cb) + var_b))), 1.0, case=label)
    assert np.all(gap <= np.diag(cb) + var_b), label
    return out["FITC", False]


def check_covariances(p, c, nt, ops, label):
    return check_covariances_at(p, points(c, nt)[0], geometry(c, nt), c.sigma2, ops, "%s-nt%d" % (label, nt))


@gpu
@pytest.mark.parametrize("c", COV, ids=case_id)
def test_every_entry_of_the_covariance_matrices(c, monkeypatch):
    p, ev = evaluated(c, monkeypatch)
    try:
        ops = fetch_operands(p, c)
        for nt in NT_COV if c.kind == "iso" else (17, 129):
            check_covariances(p, c, nt, ops, case_id(c))
    finally:
        p.close()


def cov_samples_raw(p, cov, nt, ld, add_diag, means, z):
    """gprhip_cov_samples on the leading nt x nt block of a Fortran matrix with leading dimension ld"""
    z = np.asfortranarray(z)
    out = np.full((nt, z.shape[1]), np.nan, order="F")
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _lib.check(p._lib.gprhip_cov_samples(p._handle(), ptr(cov), ld, nt, float(add_diag), JITTER, ptr(np.ascontiguousarray(means)),
                                         ptr(z), z.shape[1], ptr(out)))
    return out


@gpu
@pytest.mark.parametrize("nt", [1, 127, 128, 129, 257])
def test_the_sampler_factor_and_every_sample(nt, monkeypatch):
    """The device's own FITC matrix plus add_diag, in a buffer whose leading dimension exceeds nt.  z = I returns the columns of
    L = chol(A)^T: held to |L L^T - A|_ij <= 4 gamma_{nt+1} (|L| |L|^T)_ij + 2 u |A_ij| (factor_ratio of
    tests/test_gpu_factors.py) with A = cov + (add_diag + jitter) I in 80 bits; its strict upper part is exactly zero.  With
    that L as a given operand every sample is within (nt + 2) u (|means_i| + sum_k |L_ik| |z_kj|)."""
    c = Case("mid", "iso", N, 129, 3)
    add_diag = 0.05
    p, ev = evaluated(c, monkeypatch)
    try:
        cov = p.covariances(points(c, nt)[0], kind="FITC", predictive=False)
        ld = nt + 3
        buf = np.full((ld, nt), np.nan, order="F")
        buf[:nt] = np.triu(cov)
        L = cov_samples_raw(p, buf, nt, ld, add_diag, np.zeros(nt), np.eye(nt))
        assert np.all(np.triu(L, 1) == 0.0)
        A = np.triu(cov).astype(R.LD)
        A[np.diag_indices(nt)] += R.LD(add_diag) + R.LD(JITTER)
        ratio, _ = factor_ratio(np.ascontiguousarray(L.T), A)
        M.record("post.sampler_factor", ratio, 4.0, case="nt%d" % nt)
        assert ratio <= 4.0, (nt, ratio)
        rng = np.random.default_rng(nt)
        means = rng.normal(size=nt)
        for ns in (1, 5, 128, 129):
            z = rng.normal(size=(nt, ns))
            s = cov_samples_raw(p, buf, nt, ld, add_diag, means, z)
            ref, bound = R.samples(L, means, z)
            hold("nt%d-ns%d" % (nt, ns), "samples", s, ref, bound)
    finally:
        p.close()


# ---- train_stats --------------------------------------------------------------------------------------------------------------
def stats_shift(c, Z):
    """gprhip_train_stats of an fp32-bulk problem with 16 <= d <= 64 builds K through cov_cross_mfma_kernel: its centroid"""
    return host_centroid(Z) if (c.f32 and 16 <= c.d <= 64 and "ms" not in c.kind) else None


@gpu
@pytest.mark.parametrize("c", STATS + STATS_F32, ids=case_id)
def test_training_means_and_residual_sums(c, monkeypatch):
    X, y, Z, args = data(c)
    p, ev = evaluated(c, monkeypatch)
    try:
        t = p.debug_fetch("t")
        sums, mu = p.train_stats(want_means=True)
        sums2, none = p.train_stats(want_means=False)
    finally:
        p.close()
    assert none is None and np.array_equal(sums, sums2)
    g = R.geometry(X, Z, **hypers_of(c, args), shift=stats_shift(c, Z))
    mu_ref, mu_b = R.mean(g, t)
    hold(case_id(c), "train_means", mu, mu_ref, mu_b)
    st = R.train_stats(y, mu)
    assert sums[2] == st["maxad"], (sums[2], st["maxad"])
    for i in (0, 1, 3):
        rel = abs(float((R.LD(sums[i]) - st["sums"][i]) / st["sums"][i]))
        M.record("post.train_sums[%d]" % i, rel / st["rel"], 1.0, case=case_id(c))
        assert rel <= st["rel"], (i, sums[i], st["sums"][i], rel, st["rel"])
