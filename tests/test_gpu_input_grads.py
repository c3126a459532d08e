"""Every entry of gprhip_predict_input_grad and gprhip_eval_input_grad against tests/input_grads_ref.py: the 80-bit contraction
of the DEVICE'S OWN operands of the same model state (debug_fetch "t", "uinv", "rinv", "pg_m", "x_rows"), within the derived
running-error bound of that module -- no oracle, no condition number, no tolerance in this file -- and M = U^-1 (I - R~^-1 R~^-T)
U^-T itself ("pg_m") against the fetched factors.  tests/test_input_grads_host.py pins the reference and the bounds on the CPU
over the same cases.

Shapes sit on the kernels' own edges (read off the launch code): predict_grad_kernel<KS4, DT, VAR> d 1 4|5 8|9 16|17 32|33 64,
16 columns per tile, PG_CP = 64 columns per panel, 16 rows per wavefront and 64 per workgroup; small_predict_grad_kernel<DT>
m <= 64, d <= 16; input_grad_kernel<KS4, DT, KR> the same widths, and K read for d > 64 (blocks of 64 dimensions and a
remainder; the shift is the first inducing point) and with a projection; mxm_slices splits K at mp >= 384 (m >= 257).
Test points (points()): entry i is of kind i mod 3 -- a training input; a point 5 .. 8 length scales from the NEAREST inducing
point (beyond the inducing point that lies furthest along a direction, so the distance is exact); an inducing point moved a
quarter of a length scale -- and, from 15 points on, entry 13 lies beyond the reach of every inducing point: every K entry
underflows, the mean is +0.0, the variance (sf2 - 0) + add and the gradients zero, bit for bit.
The path is read off last_timings(): pg_cov / pg_gemm / pg_m present or absent, p2_xgrad.
Left out: gprhip_sample_paths' winner gradients (their weights have no fetch), row chunks of eval_input_grad beyond the first
("x_rows" serves one chunk), fp32-bulk problems, sharded prediction, batch lanes."""
import collections
import functools
import math

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import input_grads_ref as G
from tests import margins as M
from tests import posterior_ref as R
from tests.test_gpu_input_grad import _case
from tests.util import taken

gpu = pytest.mark.gpu
SIGMA2 = 0.1
LOG_SF2 = 0.3
NAMES = ("means", "variances", "dmeans", "dvariances")

# kind "iso" | "fat" | "proj"; forced: the one-kernel paths switched off at problem creation (GPRHIP_SMALL_PATH / GPRHIP_MID_PATH)
Case = collections.namedtuple("Case", "kind n m d D het offset forced log_sf2", defaults=(0, False, 0.0, False, 0.0))
DIMS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64)
DIMS_SMALL = (1, 4, 5, 8, 9, 16)
MS = (1, 15, 16, 17, 63, 64, 65, 129, 257)
NTS = (1, 15, 16, 17, 63, 64, 65, 129)
NTS_SMALL = (1, 63, 64, 65)
PROJ_DIMS = ((5, 2), (17, 16), (40, 3), (70, 4))

# (case, test-point counts): every value of an axis against an interior and an edge value of the other two
ENGINE = [(Case("iso", 100, 65, d, forced=d <= 16), (17, 64)) for d in DIMS] + \
    [(Case("iso", 100, 40, d, forced=True), (40,)) for d in DIMS] + \
    [(Case("iso", max(m, 100), m, 3, forced=True), (40, 65)) for m in MS] + \
    [(Case("iso", max(m, 100), m, 17), (16,)) for m in MS] + \
    [(Case("iso", 200, 129, 3, forced=True), NTS), (Case("iso", 100, 40, 17), NTS)] + \
    [(Case("fat", 100, 65, 3, 3, forced=True), (65,)), (Case("proj", 100, 65, 2, 5, True, forced=True), (65,)),
     (Case("iso", 100, 65, 3, forced=True, log_sf2=LOG_SF2), (65,)), (Case("iso", 100, 65, 3, offset=1e3, forced=True), (65,))] + \
    [(Case("proj", 100, 65, d, D, forced=True), (40,)) for D, d in PROJ_DIMS]
SMALL = [(Case("iso", 100, 17, d), (63,)) for d in DIMS_SMALL] + [(Case("iso", 100, 64, d), (65,)) for d in (1, 16)] + \
    [(Case("iso", 100, m, 3), NTS_SMALL) for m in (1, 17, 63, 64)] + \
    [(Case("fat", 100, 17, 3, 3), (65,)), (Case("proj", 100, 17, 2, 5, True), (65,)), (Case("iso", 100, 17, 3, log_sf2=LOG_SF2), (65,)),
     (Case("iso", 100, 17, 3, offset=1e3), (65,))] + [(Case("proj", 100, 17, d, D), (40,)) for D, d in PROJ_DIMS[:1] + PROJ_DIMS[2:]]
M_CASES = [Case("iso", max(m, 100), m, 3, forced=True) for m in (1, 17, 64, 65, 128, 129, 256, 257, 300)]
ROWS = (1, 17, 64, 65, 129)
# gprhip_eval_input_grad: (case, variational, model-only); m = 17 / 65 / 257: the small, mid and engine row paths.  K is READ
# (input_grad_kernel<0, DT, true>) on the engine row path with more than 64 dimensions (the rebuilt chunk) or with a projection
# (the resident store); everywhere else it is recomputed from the expansion.
XGRAD = [(Case("iso", n, m, 3), False, False) for m in (17, 65, 257) for n in ROWS] + \
    [(Case("iso", 65, 65, d), False, False) for d in DIMS] + \
    [(Case("iso", 65, m, d, forced=True), False, False) for m, d in ((17, 65), (65, 88), (257, 128), (65, 129))] + \
    [(Case("proj", 65, 65, d, D, forced=f), False, False) for D, d in PROJ_DIMS for f in (True, False)] + \
    [(Case("fat", 65, 65, 3, 3), False, False), (Case("proj", 65, 17, 2, 5, True, forced=True), False, False),
     (Case("iso", 65, 65, 3, log_sf2=LOG_SF2), False, False), (Case("iso", 65, 65, 3), True, False),
     (Case("iso", 65, 65, 3), False, True)] + \
    [(Case("iso", 65, m, 3, offset=1e3), False, False) for m in (17, 65, 257)]
PREDICT_CASES = ENGINE + SMALL      # tests/test_input_grads_host.py


def case_id(c):
    if not isinstance(c, Case):
        return "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)
    s = "%s-n%d-m%d-d%d" % (c.kind, c.n, c.m, c.d) + ("-D%d" % c.D if c.D else "") + ("-het" if c.het else "")
    return s + ("-off%g" % c.offset if c.offset else "") + ("-forced" if c.forced else "") + ("-lsf%g" % c.log_sf2 if c.log_sf2 else "")


def data(c):
    """inputs (D x n), targets, inducing points (d x m), the keyword arguments of Problem.eval"""
    Xs, y, Zs, args, ok, cond = _case(c.kind, c.n, c.m, c.d, c.D, c.het, c.offset)
    return Xs, y, Zs, dict(args, log_sf2=c.log_sf2)


def hypers_of(c, args):
    return dict(iso=c.kind == "iso", log_sf2=args["log_sf2"], log_ell=args.get("log_ell", 0.0), tproj=args.get("tproj"))


def xgrad_reads_k(c, path):
    """whether input_grad_kernel multiplies a K from memory (gprhip.hip: the engine row path's chunk loop)"""
    return path == "engine" and (c.kind == "proj" or c.d > 64)


def expected_path(c):
    return "engine" if (c.forced or c.m > 64 or c.d > 16) else "small"


@functools.lru_cache(maxsize=None)
def points(c, nt):
    """(test inputs D x nt, mask of the rows whose every K entry underflows); see the module docstring"""
    X, y, Z, args = data(c)
    tp = args.get("tproj")
    lift = (lambda p: p) if tp is None else (lambda p: tp @ np.linalg.solve(tp.T @ tp, p))
    ell = math.exp(args.get("log_ell", 0.0))
    rng = np.random.default_rng(911 + nt)
    Xt = np.empty((X.shape[0], nt))
    dead = np.zeros(nt, dtype=bool)
    for i in range(nt):
        kind = i % 3
        e = rng.normal(size=c.d)
        e /= np.linalg.norm(e)
        zf = Z[:, int(np.argmax(e @ Z))]          # no inducing point lies further along e
        if nt >= 15 and i == 13:
            Xt[:, i] = lift(zf + math.sqrt(2.0 * 900.0) * ell * e)
            dead[i] = True
        elif kind == 0:
            Xt[:, i] = X[:, (7 * i) % c.n]
        elif kind == 1:
            Xt[:, i] = lift(zf + (5.0 + (i // 3) % 4) * ell * e)
        else:
            Xt[:, i] = lift(Z[:, (5 * i) % c.m] + 0.25 * ell * e)
    Xt = np.asfortranarray(Xt)
    Xt.setflags(write=False)
    return Xt, dead


def _frozen(g):
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


@functools.lru_cache(maxsize=4)
def geometry(c, nt):
    X, y, Z, args = data(c)
    return _frozen(G.geometry(points(c, nt)[0], Z, **hypers_of(c, args)))


def open_problem(c, monkeypatch, n=None):
    if c.forced:
        monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")     # read when the problem is created
        monkeypatch.setenv("GPRHIP_MID_PATH", "0")
    X, y, Z, args = data(c)
    return gpr_amd.Problem(gpr_amd.COV_SE_ISO if c.kind == "iso" else gpr_amd.COV_SE_FAT, c.n if n is None else n, X.shape[0], c.d, c.m)


def evaluated(c, monkeypatch, **kw):
    X, y, Z, args = data(c)
    p = open_problem(c, monkeypatch)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **dict(args, **kw))
    return p


def hold(label, what, got, ref, bound):
    """Every entry within its bound; the worst ratio is recorded first."""
    got = np.asarray(got)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (label, what, got.shape, ref.shape)
    r, at = G.ratio(got, ref, bound)
    M.record("igrads." + what, r, 1.0, case=label, scale=float(np.max(np.abs(ref))) if ref.size else 0.0,
             bound=float(np.max(bound)) if ref.size else 0.0)
    print("%s %s: worst entry at %.3f of its bound" % (label, what, r))
    assert r <= 1.0, "%s %s: entry %d: got %r, reference %r, bound %.3e (x %.2f)" % (
        label, what, at, float(got.ravel()[at]), float(ref.ravel()[at]), float(np.ravel(bound)[at]), r)
    return r


def reference(c, nt, ops, path, add, var=True):
    """{name: (reference, bound)} in the layout of Problem.predict_input_grad, from the fetched operands"""
    g = geometry(c, nt)
    Gm = eG = None
    if var:
        Gm, eG = G.g_engine(g, ops["pg_m"]) if path == "engine" else G.g_small(g, ops["uinv"], ops["rinv"])
    ref = G.predict(g, ops["t"], add, path == "engine", Gm, eG)
    return {k: ((v.T, b.T) if v.ndim == 2 else (v, b)) for k, (v, b) in ref.items()}


def check_predict(p, c, nt, path, label, fetch_var=True):
    """the four outputs and the mean-only form at the fixed mix of nt test points"""
    X, y, Z, args = data(c)
    Xt, dead = points(c, nt)
    label = "%s-nt%d" % (label, nt)
    sf2 = math.exp(c.log_sf2)
    p.set_timing(2)
    ops = dict(t=p.debug_fetch("t"))
    inst = "%s.d%d" % (path, c.d)
    if fetch_var:
        full = p.predict_input_grad(Xt)
        stages = set(p.last_timings())
        assert ("pg_cov" in stages and "pg_gemm" in stages) == (path == "engine") and "pg_grad" in stages, (label, stages)
        ops.update(uinv=p.debug_fetch_matrix("uinv"), rinv=p.debug_fetch_matrix("rinv"))
        if path == "engine":
            ops["pg_m"] = p.debug_fetch_matrix("pg_m")
            again = p.predict_input_grad(Xt)
            assert "pg_m" not in p.last_timings() and all(np.array_equal(full[k], again[k]) for k in NAMES), label   # a fetch only copies
        ref = reference(c, nt, ops, path, SIGMA2)
        for name in NAMES:
            hold(label, "%s.var.%s" % (inst, name), full[name], *ref[name])
        assert np.all(full["means"][dead] == 0.0) and not np.any(np.signbit(full["means"][dead])), label
        assert np.all(full["variances"][dead] == (sf2 - 0.0) + SIGMA2), label
        assert np.all(full["dmeans"][:, dead] == 0.0) and np.all(full["dvariances"][:, dead] == 0.0), label
    mean = p.predict_input_grad(Xt, want=("means", "dmeans"))
    assert not {"pg_cov", "pg_gemm", "pg_m"} & set(p.last_timings()), label
    ref = reference(c, nt, ops, path, SIGMA2, var=False)
    for name in ("means", "dmeans"):
        hold(label, "%s.mean.%s" % (inst, name), mean[name], *ref[name])
    assert np.all(mean["means"][dead] == 0.0) and np.all(mean["dmeans"][:, dead] == 0.0), label
    p.set_timing(0)
    return ops


# ---- gprhip_predict_input_grad -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,nts", PREDICT_CASES, ids=case_id)
def test_every_entry_of_the_prediction_gradient_against_the_device_operands(c, nts, monkeypatch):
    p = evaluated(c, monkeypatch)
    try:
        for nt in nts:
            check_predict(p, c, nt, expected_path(c), case_id(c))
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("c", [Case("iso", 100, 17, 3), Case("iso", 100, 65, 3), Case("iso", 100, 40, 17)], ids=case_id)
def test_the_mean_part_from_a_predictor_loaded_with_coefficients_alone(c, monkeypatch):
    X, y, Z, args = data(c)
    p = evaluated(c, monkeypatch)
    try:
        t = p.debug_fetch("t")
    finally:
        p.close()
    q = open_problem(c, monkeypatch, n=64)
    try:
        q.load_predictor(coeffs=t, sigma2=SIGMA2, inducing=Z, **args)
        check_predict(q, c, 65, expected_path(c), case_id(c) + "-coeffs", fetch_var=False)
    finally:
        q.close()


@gpu
@pytest.mark.parametrize("c", [Case("iso", 100, 17, 3), Case("iso", 100, 65, 3), Case("iso", 300, 257, 3)], ids=case_id)
def test_means_and_variances_against_gprhip_predict_through_the_two_bounds(c, monkeypatch):
    """different kernels: no bits are demanded; each lies within its own bound of the same 80-bit value"""
    nt = 65
    p = evaluated(c, monkeypatch)
    try:
        path = expected_path(c)
        Xt = points(c, nt)[0]
        full = p.predict_input_grad(Xt)
        mu, var = p.predict(Xt)
        ops = dict(t=p.debug_fetch("t"), uinv=p.debug_fetch_matrix("uinv"), rinv=p.debug_fetch_matrix("rinv"))
        if path == "engine":
            ops["pg_m"] = p.debug_fetch_matrix("pg_m")
    finally:
        p.close()
    g = geometry(c, nt)
    ref = reference(c, nt, ops, path, SIGMA2)
    mu_ref, mu_b = R.mean(g, ops["t"])
    var_ref, var_b = R.variance(g, R.chain(g, ops["uinv"], ops["rinv"]), SIGMA2)
    hold(case_id(c), "vs_predict.means", full["means"], _ld64(mu), ref["means"][1] + mu_b)
    # the two 80-bit variances differ by what M_dev differs from the factors' M: both bounds and that difference's own
    dv = np.abs(ref["variances"][0] - var_ref).astype(np.float64)
    hold(case_id(c), "vs_predict.variances", full["variances"], _ld64(var), ref["variances"][1] + var_b + dv)
    if path == "engine":
        Mr, Mb = G.m_matrix(ops["uinv"], ops["rinv"])
        K = np.abs(g["K"])
        assert np.all(dv <= ((K @ Mb) * K).sum(1)), case_id(c)      # ... which the bound of M accounts for


def _ld64(a):
    return np.asarray(a, dtype=R.LD)


# ---- M by itself ---------------------------------------------------------------------------------------------------------------
def check_m(p, c, label):
    uinv, rinv = p.debug_fetch_matrix("uinv"), p.debug_fetch_matrix("rinv")
    Mr, Mb = G.m_matrix(uinv, rinv)
    Md = p.debug_fetch_matrix("pg_m")
    hold(label, "pg_m", Md, Mr, Mb)
    assert np.array_equal(Md, Md.T) or G.ratio(Md.T, Mr, Mb)[0] <= 1.0, label
    return Md


@gpu
@pytest.mark.parametrize("c", M_CASES, ids=case_id)
def test_m_against_the_fetched_factors_also_after_a_second_model(c, monkeypatch):
    X, y, Z, args = data(c)
    Xt = points(c, 17)[0]
    p = evaluated(c, monkeypatch)
    try:
        with pytest.raises(_lib.GprHipError) as err:      # between the evaluation and the first variance call
            p.debug_fetch_matrix("pg_m")
        assert err.value.status == _lib.ESTATE and "pg_m" in str(err.value)
        p.predict_input_grad(Xt, want=("means", "dmeans"))
        with pytest.raises(_lib.GprHipError):
            p.debug_fetch_matrix("pg_m")
        p.predict_input_grad(Xt)
        first = check_m(p, c, case_id(c))
        # the padding: K's padding columns are exact zeros (cov_cross_kernel), so G = K M needs M's padding rows finite, and
        # predict_grad_kernel never multiplies G's padding columns; the live block of the padded fetch is the plain fetch
        mp = -(-c.m // 128) * 128
        full = p.debug_fetch_matrix("pg_m", rows=mp)
        assert np.array_equal(full[:c.m, :c.m], first) and np.all(np.isfinite(full)), case_id(c)
        # a second model: other hyper-parameters
        other = dict(args, log_sf2=args["log_sf2"] + 0.4)
        if "log_ell" in other:
            other["log_ell"] += 0.2
        p.eval(sigma2=0.3, inducing=Z, want_grad=False, **other)
        with pytest.raises(_lib.GprHipError):
            p.debug_fetch_matrix("pg_m")
        p.predict_input_grad(Xt)
        second = check_m(p, c, case_id(c) + "-second")
        assert c.m == 1 or not np.array_equal(first, second)
        # a loaded predictor with co-variance coefficients: the first model's factors again
        q = evaluated(c, monkeypatch)
        try:
            t, (Uc, Rc) = q.debug_fetch("t"), q.co_variance_coeffs()
        finally:
            q.close()
        p.load_predictor(coeffs=t, co_variance_coeffs=(Uc, Rc), sigma2=SIGMA2, inducing=Z, **args)
        with pytest.raises(_lib.GprHipError):
            p.debug_fetch_matrix("pg_m")
        p.predict_input_grad(Xt)
        check_m(p, c, case_id(c) + "-loaded")
    finally:
        p.close()


# ---- gprhip_eval_input_grad ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,variational,model_only", XGRAD, ids=case_id)
def test_every_entry_of_the_training_input_gradient_against_the_device_x(c, variational, model_only, monkeypatch):
    X, y, Z, args = data(c)
    p = open_problem(c, monkeypatch)
    try:
        p.set_inputs(X)
        p.set_targets(y)
        p.set_timing(2)
        ev, got = p.eval_input_grad(sigma2=SIGMA2, inducing=Z, variational=variational, model_only=model_only, **args)
        stages = set(p.last_timings())
        path = taken(stages)
        assert "p2_xgrad" in stages, stages
        if c.d <= 16 and c.kind != "proj":
            assert path == ("engine" if c.forced else "small" if c.m <= 64 else "mid" if c.m <= 256 else "engine"), stages
        Xd = p.debug_fetch_matrix("x_rows", rows=c.n)
    finally:
        p.close()
    read_k = xgrad_reads_k(c, path)
    g = G.geometry(X, Z, **hypers_of(c, args))
    ref, bound = G.train_input_grad(g, Xd, read_k)
    hold("%s-%s%s%s" % (case_id(c), path, "-variational" if variational else "", "-model" if model_only else ""),
         "xgrad.%s.d%d" % ("readK" if read_k else "recompute", c.d), got, ref.T, bound.T)
