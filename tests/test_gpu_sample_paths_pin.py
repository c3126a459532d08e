"""Every entry of gprhip_sample_paths and gprhip_sample_paths_refine against tests/sample_paths_pin_ref.py: the 80-bit
contraction of the DEVICE'S OWN operands of the same model state (debug_fetch "t", "uinv", "rinv" after the evaluation, the
weights "sp_a" after the call), within the derived running-error bound of that module -- no oracle, no condition number, no
tolerance in this file.  The weights are held against the factors, everything else against the fetched weights, so the two
errors are held separately.  tests/test_sample_paths_pin_host.py pins the reference and the bounds on the CPU.

The cases are those of tests/test_gpu_input_grad._case (through tests/test_gpu_input_grads.data: cond <= 1e5 asserted there),
one axis at a time around ("iso", 200, 65, 3), nt = 65, ns = 17; the shapes sit on the kernels' edges, read off the launch code:
  weights   sp_tri_row's cw in {1, 2, 4, 8, 16}, one workgroup behind a barrier (mp <= 128 and ns <= 4) or two launches;
  paths     sample_paths_kernel<KS4, DT, NB> d 1 4|5 8|9 16|17 32|33 64, NB = ceil(ns / 16), panels of 64 or 32 columns
            (DP + NW > 96), 16 columns per tile, 16 points per wavefront and 64 per workgroup;
  residual  one kernel (m <= 64, d <= 16) or launch_cov_cross + engine product + row sums of squares;
  gradient  path_grad_at_kernel at EVERY row (top_k = nt = 64), path_eval through max_evals = 1 and through a trace.
Test points (pin_points): those of tests/test_gpu_input_grads.points -- training inputs, points 5 .. 8 length scales from the
nearest inducing point, inducing points moved a quarter of a length scale, entry 13 beyond the reach of every inducing point
(every K entry underflows: the path is +0.0 bit for bit) -- and entry 2 ON an inducing point."""
import functools

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import margins as M
from tests import sample_paths_pin_ref as S
from tests.test_gpu_input_grads import PROJ_DIMS, Case, case_id, data, hypers_of, points

gpu = pytest.mark.gpu
SIGMA2 = 0.1
BASE = Case("iso", 200, 65, 3)
NT, NS = 65, 17
DIMS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64)


def _iso(m=65, d=3, **kw):
    return Case("iso", max(m, 200) if m > 64 else 200, m, d, **kw)


# ---- the cases (tests/test_sample_paths_pin_host.py walks the same lists) -----------------------------------------------------
WEIGHT_NS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 64)
WEIGHTS = [(_iso(m), (3, 17)) for m in (1, 15, 64, 128, 129, 257)] + [(BASE, WEIGHT_NS)]
# (case, nt, ns)
PATHS = [(_iso(65, d), NT, NS) for d in DIMS] + [(BASE, NT, ns) for ns in (16, 33, 49, 64)] + \
    [(_iso(65, 64), NT, 32), (_iso(65, 64), NT, 33)] + \
    [(_iso(m), NT, NS) for m in (15, 16, 17, 31, 32, 33, 63, 64, 129)] + \
    [(BASE, nt, NS) for nt in (1, 15, 16, 17, 63, 64, 130)] + \
    [(Case("fat", 200, 65, 3, 3), NT, NS)] + [(Case("proj", 200, 65, d, D), NT, NS) for D, d in PROJ_DIMS] + \
    [(_iso(65, 3, offset=1e3), NT, NS), (_iso(65, 3, offset=1e5), NT, NS)]
# (case, the one-kernel residual)
RESID = [(Case("iso", 64, 10, 3), True), (BASE, False), (_iso(40, 17), False)]
GRAD_AT = [_iso(m) for m in (63, 64, 65, 129)] + [_iso(65, d) for d in (1, 17, 64)] + [Case("proj", 200, 65, d, D) for D, d in PROJ_DIMS]
# (case, starts, draws, form of draw_of)
EVAL = [(BASE, ns, 17, "round") for ns in (1, 16, 17, 64, 65)] + [(BASE, 65, nd, "round") for nd in (1, 64)] + \
    [(BASE, 65, 17, f) for f in ("const", "reversed")] + [(_iso(65, d), 65, 17, "round") for d in (9, 17, 33, 64)] + \
    [(_iso(m), 65, 17, "reversed") for m in (15, 33, 64, 129)] + [(Case("proj", 200, 65, d, D), 65, 17, "round") for D, d in PROJ_DIMS]
TRACE = [(BASE, 33, 5, "round"), (Case("proj", 200, 65, 2, 5), 33, 5, "reversed")]


def ident(v):
    return case_id(v) if isinstance(v, Case) else str(v)


def _lift(args):
    tp = args.get("tproj")
    return (lambda p: p) if tp is None else (lambda p: tp @ np.linalg.solve(tp.T @ tp, p))


@functools.lru_cache(maxsize=None)
def pin_points(c, nt):
    """(test inputs D x nt, the rows whose every K entry underflows); entry 2 lies on an inducing point"""
    X, y, Z, args = data(c)
    Xt, dead = points(c, nt)
    Xt = np.array(Xt, order="F")
    if nt >= 3:
        Xt[:, 2] = _lift(args)(Z[:, 0])
    Xt.setflags(write=False)
    return Xt, dead


def draws(c, nt, ns):
    rng = np.random.default_rng(5000 + 131 * c.m + 7 * ns + nt)
    return np.asfortranarray(rng.normal(size=(c.m, ns))), np.asfortranarray(rng.normal(size=(nt, ns)))


def draw_of(ns, nd, form):
    i = np.arange(ns)
    return {"const": np.full(ns, nd - 1), "round": i % nd, "reversed": (nd - 1) - i % nd}[form].astype(np.int32)


def geometry_at(c, Xt):
    X, y, Z, args = data(c)
    return S.geometry(Xt, Z, **hypers_of(c, args))


def open_problem(c, chunk_rows=0, n=None):
    X, y, Z, args = data(c)
    return gpr_amd.Problem(gpr_amd.COV_SE_ISO if c.kind == "iso" else gpr_amd.COV_SE_FAT, c.n if n is None else n, X.shape[0], c.d,
                           c.m, chunk_rows=chunk_rows)


def evaluated(c, chunk_rows=0):
    X, y, Z, args = data(c)
    p = open_problem(c, chunk_rows)
    try:
        p.set_inputs(X)
        p.set_targets(y)
        p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
    except Exception:
        p.close()
        raise
    return p


def operands(p):
    return dict(t=p.debug_fetch("t"), uinv=p.debug_fetch_matrix("uinv"), rinv=p.debug_fetch_matrix("rinv"))


def hold(label, what, got, ref, bound):
    """Every entry within its bound; the worst ratio is recorded first."""
    got = np.asarray(got)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (label, what, got.shape, ref.shape)
    r, at = S.ratio(got, ref, bound)
    M.record("sp_pin." + what, r, 1.0, case=label, scale=float(np.max(np.abs(ref))) if ref.size else 0.0,
             bound=float(np.max(bound)) if ref.size else 0.0)
    print("%s %s: worst entry at %.3f of its bound" % (label, what, r))
    assert r <= 1.0, "%s %s: entry %d: got %r, reference %r, bound %.3e (x %.2f)" % (
        label, what, at, float(got.ravel()[at]), float(ref.ravel()[at]), float(np.ravel(bound)[at]), r)
    return r


def cw_of(ns):
    cw = 1
    while cw < ns and cw < 16:
        cw <<= 1
    return cw


def padding_is_zero(full, m, ns):
    """the padded [mp][64] block: rows >= m and columns >= ns exactly zero"""
    return bool(np.all(full[m:] == 0.0) and np.all(full[:, ns:] == 0.0))


def check_weights(p, c, ops, z, label):
    """ "sp_a" of the call just made against the factors; the padded block; returns the fetched weights"""
    ns = z.shape[1]
    A = p.debug_fetch_matrix("sp_a")
    assert A.shape == (c.m, ns), (label, A.shape)
    ref, bound = S.weights(ops["t"], ops["uinv"], ops["rinv"], z)
    route = "one_launch" if (c.m <= 128 and ns <= 4) else "two_launches"
    hold(label, "weights.cw%d.%s" % (cw_of(ns), route), A, ref, bound)
    mp = -(-c.m // 128) * 128
    full = p.debug_fetch_matrix("sp_a", rows=mp)
    assert full.shape == (mp, 64) and np.array_equal(full[:c.m, :ns], A), label
    assert padding_is_zero(full, c.m, ns), (label, "padding not zero")
    return A


def box_of(c, wide):
    X, y, Z, args = data(c)
    if wide:
        return np.full(X.shape[0], -1e6), np.full(X.shape[0], 1e6)
    return X.min(axis=1).copy(), X.max(axis=1).copy()


# ---- the fetch itself ----------------------------------------------------------------------------------------------------------
@gpu
def test_sp_a_is_a_state_error_without_weights_of_the_current_model():
    c = BASE
    X, y, Z, args = data(c)
    Xt = pin_points(c, 17)[0]
    z, _ = draws(c, 17, 3)
    p = evaluated(c)
    try:
        def refused():
            with pytest.raises(_lib.GprHipError) as err:
                p.debug_fetch_matrix("sp_a")
            assert err.value.status == _lib.ESTATE and "sp_a" in str(err.value)
        refused()                                            # between the evaluation and the first call
        first = p.sample_paths(Xt, z)["samples"]
        A = p.debug_fetch_matrix("sp_a")
        assert np.array_equal(p.sample_paths(Xt, z)["samples"], first) and np.array_equal(p.debug_fetch_matrix("sp_a"), A)   # a copy only
        with pytest.raises(_lib.GprHipError) as err:         # too short for m x ns
            out = np.empty(c.m * 3 - 1)
            _lib.check(p._lib.gprhip_debug_fetch(p._handle(), b"sp_a", out.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)), out.size))
        assert err.value.status == _lib.EBADARG
        with pytest.raises(ValueError):                      # neither m nor mp rows: no layout of the library's
            p.debug_fetch_matrix("sp_a", rows=c.m + 1)
        p.eval(sigma2=0.3, inducing=Z, want_grad=False, **args)
        refused()                                            # after the next evaluation
        p.sample_paths(Xt, z)
        assert not np.array_equal(p.debug_fetch_matrix("sp_a"), A)
        ops = operands(p)
        U_, R_ = p.co_variance_coeffs()
        p.load_predictor(coeffs=ops["t"], co_variance_coeffs=(U_, R_), sigma2=0.3, inducing=Z, **args)
        refused()                                            # after load_predictor
    finally:
        p.close()


# ---- the weights ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,nss", WEIGHTS, ids=ident)
def test_every_weight_against_the_fetched_factors(c, nss):
    X, y, Z, args = data(c)
    Xt = pin_points(c, 17)[0]
    lo, hi = box_of(c, True)
    p = evaluated(c)
    try:
        ops = operands(p)
        for ns in (64,) + tuple(nss):                        # (a 64-draw call first: every later call finds its columns used)
            z, _ = draws(c, 17, ns)
            p.sample_paths(Xt, z)
            A = check_weights(p, c, ops, z, "%s-ns%d" % (case_id(c), ns))
            # the same z through gprhip_sample_paths_refine: the same bits, the same padding
            p.sample_paths_refine(Xt, z, draw_of(17, ns, "round"), lower=lo, upper=hi, max_evals=1)
            B = check_weights(p, c, ops, z, "%s-ns%d-refine" % (case_id(c), ns))
            assert np.array_equal(A, B), (case_id(c), ns)
    finally:
        p.close()


# ---- the paths -----------------------------------------------------------------------------------------------------------------
def check_paths(p, c, nt, ns, label, ops=None):
    Xt, dead = pin_points(c, nt)
    z, _ = draws(c, nt, ns)
    got = p.sample_paths(Xt, z)["samples"]
    A = p.debug_fetch_matrix("sp_a")
    if ops is not None:
        check_weights(p, c, ops, z, label)
    F, eF = S.paths(geometry_at(c, Xt), A)
    ks4 = 1 if c.d <= 4 else 2 if c.d <= 8 else 4 if c.d <= 16 else 8 if c.d <= 32 else 16
    hold(label, "paths.ks%d.nb%d" % (ks4, (ns + 15) // 16), got, F, eF)
    assert np.all(got[dead] == 0.0) and not np.any(np.signbit(got[dead])), label
    return got, A


@gpu
@pytest.mark.parametrize("c,nt,ns", PATHS, ids=ident)
def test_every_path_value_against_the_fetched_weights(c, nt, ns):
    p = evaluated(c)
    try:
        check_paths(p, c, nt, ns, "%s-nt%d-ns%d" % (case_id(c), nt, ns), operands(p))
    finally:
        p.close()


@gpu
def test_paths_of_a_loaded_predictor_and_over_three_chunks():
    c = BASE
    X, y, Z, args = data(c)
    p = evaluated(c, chunk_rows=128)
    try:
        ops = operands(p)
        U_, R_ = p.co_variance_coeffs()
        check_paths(p, c, 300, NS, case_id(c) + "-chunks128-nt300", ops)
    finally:
        p.close()
    q = open_problem(c, n=64)
    try:
        q.load_predictor(coeffs=ops["t"], co_variance_coeffs=(U_, R_), sigma2=SIGMA2, inducing=Z, **args)
        check_paths(q, c, NT, NS, case_id(c) + "-loaded", operands(q))
    finally:
        q.close()


# ---- the residual part and the samples -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,small", RESID, ids=ident)
def test_every_sample_with_eps_inside_the_interval_of_the_residual(c, small):
    import torch
    nt, ns = NT, 5
    Xt, dead = pin_points(c, nt)
    z, eps = draws(c, nt, ns)
    g = geometry_at(c, Xt)
    p = evaluated(c)
    try:
        ops = operands(p)
        # the route is the driver's one_kernel_path(), the predicate behind plan.small of every call at test points:
        # gprhip_predict_input_grad forms K and G in memory (stages pg_cov, pg_gemm) exactly when it is false
        p.set_timing(2)
        p.predict_input_grad(Xt)
        stages = set(p.last_timings())
        assert ("pg_cov" in stages and "pg_gemm" in stages) == (not small) and "pg_grad" in stages, (case_id(c), stages)
        p.set_timing(0)
        for predictive in (False, True):
            label = "%s-%s" % (case_id(c), "predictive" if predictive else "latent")
            got = p.sample_paths(Xt, z, eps=eps, predictive=predictive)["samples"]
            A = p.debug_fetch_matrix("sp_a")
            F, eF = S.paths(g, A)
            res, e = S.resid(g, ops["uinv"], SIGMA2 if predictive else 0.0, small)
            mid, half = S.samples(F, eF, res, e, eps)
            hold(label, "samples.%s" % ("one_kernel" if small else "engine"), got, mid, half)
            # entry 2 lies on an inducing point: the argument of the root is at the level of the jitter, and still inside
            assert predictive or res[2] < 1e-3 * g["sf2"], (label, float(res[2]))
            # eps and the samples in device memory: the same bits
            dev = torch.device("cuda:0")
            xt = torch.tensor(np.ascontiguousarray(Xt.T), device=dev)
            et = torch.tensor(np.ascontiguousarray(eps.T), device=dev)
            out = torch.full((ns, nt), float("nan"), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            p.sample_paths(xt.data_ptr(), z, eps=et.data_ptr(), predictive=predictive, out_device_ptrs={"samples": out.data_ptr()}, nt=nt)
            assert np.array_equal(out.cpu().numpy().T, got), label
    finally:
        p.close()


# ---- the gradient of a draw at every row ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", GRAD_AT, ids=ident)
def test_the_gradient_of_every_draw_at_every_row(c):
    nt, ns = 64, NS                                                      # top_k = nt = 64: every row is a winner
    Xt, dead = pin_points(c, nt)
    z, _ = draws(c, nt, ns)
    p = evaluated(c)
    try:
        outs = [p.sample_paths(Xt, z, top_k=64, maximise=mx) for mx in (True, False)]
        A = p.debug_fetch_matrix("sp_a")
    finally:
        p.close()
    dF, edF = S.path_grads(geometry_at(c, Xt), A, direct=True)           # ns x nt x D
    for mx, out in zip((True, False), outs):
        idx = out["top_index"]                                           # top_k x ns
        assert all(sorted(idx[:, j]) == list(range(nt)) for j in range(ns)), "every row is a winner of every draw"
        got = np.empty((ns, nt, Xt.shape[0]))
        for j in range(ns):
            got[j, idx[:, j]] = out["top_dvalues"][:, :, j].T
        hold("%s-%s" % (case_id(c), "max" if mx else "min"), "grad_at.d%d%s" % (c.d, ".proj" if c.kind == "proj" else ""), got, dF, edF)
        assert np.all(got[:, dead] == 0.0), case_id(c)


# ---- the refinement evaluator at arbitrary points ------------------------------------------------------------------------------
def check_evaluator(label, what, c, A, dr, sign, x, values, dvalues):
    """objective and gradient at the points x (D x k) for the draws dr against path_eval's form"""
    ref = S.evaluator(geometry_at(c, x), A, dr, sign)
    hold(label, what + ".values", values, *ref["values"])
    hold(label, what + ".dvalues", dvalues, *ref["dvalues"])


@gpu
@pytest.mark.parametrize("c,ns,nd,form", EVAL, ids=ident)
def test_the_evaluator_of_the_refinement_at_every_start(c, ns, nd, form):
    route = 2 if c.kind == "proj" else 1
    starts = pin_points(c, ns)[0]
    z, _ = draws(c, ns, nd)
    dr = draw_of(ns, nd, form)
    p = evaluated(c)
    try:
        p.set_timing(2)
        for wide in (False, True):
            for mx in (True, False):
                lo, hi = box_of(c, wide)
                out = p.sample_paths_refine(starts, z, dr, lower=lo, upper=hi, maximise=mx, max_evals=1)
                stages = p.last_timings()
                assert ("prf_kernel" in stages) == (route == 1) and ("prf_eval" in stages) == (route == 2), stages
                A = p.debug_fetch_matrix("sp_a")
                clipped = np.clip(starts, lo[:, None], hi[:, None])
                assert np.array_equal(out["x"], clipped) and (wide or ns < 3 or not np.array_equal(clipped, starts)), "the clip moves starts"
                label = "%s-ns%d-nd%d-%s-%s-%s" % (case_id(c), ns, nd, form, "wide" if wide else "box", "max" if mx else "min")
                check_evaluator(label, "eval.r%d.d%d" % (route, c.d), c, A, dr, 1.0 if mx else -1.0, out["x"], out["values"], out["dvalues"])
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("c,ns,nd,form", TRACE, ids=ident)
def test_every_trace_record_of_eight_evaluations(c, ns, nd, form):
    route = 2 if c.kind == "proj" else 1
    starts = pin_points(c, ns)[0]
    z, _ = draws(c, ns, nd)
    dr = draw_of(ns, nd, form)
    lo, hi = box_of(c, False)
    D = starts.shape[0]
    p = evaluated(c)
    try:
        p.set_timing(2)
        out = p.sample_paths_refine(starts, z, dr, lower=lo, upper=hi, max_evals=8,
                                    want=("x", "values", "dvalues", "evals", "accepted", "status", "trace"))
        stages = p.last_timings()
        assert ("prf_kernel" in stages) == (route == 1) and ("prf_eval" in stages) == (route == 2), stages
        A = p.debug_fetch_matrix("sp_a")
    finally:
        p.close()
    recs = [(i, e) for i in range(ns) for e in range(int(out["evals"][i]))]
    assert len(recs) > ns, "some start takes more than one evaluation"
    tr = np.array([out["trace"][i, e] for i, e in recs])                 # [x (D) | gradient (D) | value | alpha | accepted]
    label = "%s-ns%d-nd%d-%s-trace" % (case_id(c), ns, nd, form)
    check_evaluator(label, "trace.r%d" % route, c, A, dr[[i for i, e in recs]], 1.0, np.asfortranarray(tr[:, :D].T), tr[:, 2 * D],
                    tr[:, D:2 * D].T)
    check_evaluator(label, "trace.r%d.final" % route, c, A, dr, 1.0, out["x"], out["values"], out["dvalues"])
