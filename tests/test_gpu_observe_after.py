"""Every posterior call on the states gprhip_observe, gprhip_posterior_restore and their neighbours leave behind
(tests/observe_after_cases.py: routes A - F, every row path), against the 80-bit contraction of the operands fetched from that
very state -- so that a read of a buffer the update does not refresh cannot pass by being made alike on both sides.
tests/test_observe_after_host.py shows on the CPU that these checks pass an honest double-precision device and miss a stale
factor by four orders of magnitude and more.

Per state: ratios() of the cases module (R~'^-1 and t against R~' and b'; predict; predict_input_grad; the path weights and the
paths; covariances of both kinds; r_mat; the training means), then with the helpers of the calls' own pin tests, bounds unchanged:
check_predict_at / check_covariances_at (tests/test_gpu_posterior.py: outputs each alone, exact bits at far points), cov_samples on
the FITC matrix (posterior_ref.samples), acquire's four criteria with top_k = 4 (_layer_a, _check_top of tests/test_gpu_acquire.py),
acquire_refine (the trace check of tests/test_gpu_refine.py), sample_paths with per-draw top-k and sample_paths_refine (check_weights,
check_evaluator of tests/test_gpu_sample_paths_pin.py on every trace record, _check_rule of tests/test_gpu_path_refine.py);
chol_km and cond_km keep their bits.  A model-only state serves the variance side; what it refused before the observation it
refuses after it with the same status.
Route A at m = 17, 129, 300 is also held to the refit of the n + k rows from scratch in 80 bits, route C's predict likewise."""
import numpy as np
import pytest

import gpr_amd
from tests import acquire_ref as AR
from tests import margins as M
from tests import observe_after_cases as OA
from tests import observe_ref as O
from tests import posterior_ref as R
from tests import sample_paths_ref as SPR
from tests.predict_grad_ref import predict_grad_ref
from tests.test_gpu_acquire import ALL, C, EPS, _check_top, _kw, _layer_a, _ref_kw
from tests.test_gpu_factors import factor_ratio
from tests.test_gpu_observe import N, SIGMA2, problem, split
from tests.test_gpu_parity import TOL_POST
from tests.test_gpu_path_refine import _check_rule, _records
from tests.test_gpu_posterior import JITTER, Operands, check_covariances_at, check_predict_at, cov_samples_raw, predict_raw
from tests.test_gpu_refine import OPTS
from tests.test_gpu_refine import _check as check_refine_trace
from tests.test_gpu_sample_paths_pin import check_evaluator, check_weights
from tests.util import taken

gpu = pytest.mark.gpu
FORCED = (("GPRHIP_SMALL_PATH", "0"), ("GPRHIP_MID_PATH", "0"))
NSTARTS = 4


class Device:
    """a Problem behind the calls ratios() makes"""

    def __init__(self, p, targets=True, has_training=True):
        self.p, self.targets, self.has_training = p, targets, has_training

    def fetch(self):
        p = self.p
        out = dict(uinv=p.debug_fetch_matrix("uinv"), rinv=p.debug_fetch_matrix("rinv"), rtil=p.debug_fetch_matrix("rtil"))
        if self.targets:
            out.update(t=p.debug_fetch("t"), bvec=p.debug_fetch("bvec"))
        return out

    def predict(self, Xt, predictive):
        return self.p.predict(Xt, predictive=predictive) if self.targets else predict_raw(self.p, Xt, predictive, False, True)

    def predict_input_grad(self, Xt):
        return self.p.predict_input_grad(Xt, **({} if self.targets else dict(want=("variances", "dvariances"))))

    def weights(self, Xt, z):
        s = self.p.sample_paths(Xt, z)["samples"]
        return self.p.debug_fetch_matrix("sp_a"), s

    def covariances(self, Xt, kind, predictive):
        return self.p.covariances(Xt, kind=kind, predictive=predictive)

    def factors(self):
        return self.p.co_variance_coeffs()

    def train_means(self):
        return self.p.train_stats(want_means=True)[1]


def opened(s, monkeypatch, variant=None):
    """a problem after eval on the n rows, on the row path the state names (read off the timing names)"""
    if s.c.forced:
        for k, v in FORCED:
            monkeypatch.setenv(k, v)
    X, y, Xn, yn, Z, args = split(s.c, 1)
    variant = s.variant if variant is None else variant
    p = problem(s.c)
    p.set_inputs(X)
    p.set_targets(y)
    p.set_timing(2)
    ev = p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, model_only=variant == "model-only", **args)
    assert taken(set(p.last_timings())) == s.path, (OA.state_id(s), sorted(p.last_timings()))
    p.set_timing(0)
    if variant == "loaded":
        q = problem(s.c)
        q.load_predictor(sigma2=SIGMA2, inducing=Z, coeffs=ev.coeffs, co_variance_coeffs=p.co_variance_coeffs(), **args)
        p.close()
        p = q
    return p


def box_of(c):
    X = split(c, 1)[0]
    return X.min(axis=1).copy(), X.max(axis=1).copy()


def refine_calls(p, c, trace=False):
    """(acquire_refine's outputs, sample_paths_refine's, the arguments) from four starts, max_evals = 12"""
    lo, hi = box_of(c)
    starts = np.asfortranarray(OA.live(c)[:, :NSTARTS])
    mu = p.predict(starts, predictive=False)[0]
    kw = dict(maximise=True, best=float(np.median(mu)), xi=0.0, kappa=0.0, var_floor=1e-10, predictive=False)
    want = dict(want=gpr_amd.Problem.REFINE_OUTPUTS) if trace else {}
    dr = np.arange(NSTARTS, dtype=np.int32) % OA.NS
    a = p.acquire_refine(starts, "ei", lower=lo, upper=hi, **want, **kw, **OPTS)
    b = p.sample_paths_refine(starts, OA.draws(c), dr, lower=lo, upper=hi, **want, **OPTS)
    return a, b, (lo, hi, kw, dr)


def downstream(p, c, targets=True, has_training=True):
    """every downstream call once; the outputs, for the routes that compare bits"""
    Xt = OA.points_at(c, OA.NT)[0]
    dev = Device(p, targets, has_training)
    out = dict(var=dev.predict(Xt, True)[1], cond=np.array(p.condition()))
    out.update({"pg_" + k: v for k, v in dev.predict_input_grad(Xt).items()})
    for kind in ("FITC", "FIC"):
        out["cov_" + kind] = p.covariances(Xt, kind=kind, predictive=False)
    out["cov_samples"] = p.cov_samples(out["cov_FITC"], np.zeros(OA.NT), np.eye(OA.NT)[:, :3], add_diag=0.05)
    out["chol_km"], out["r_mat"] = p.co_variance_coeffs()
    if targets:
        out["mean"] = dev.predict(Xt, True)[0]
        a = p.acquire(OA.live(c), "ei", maximise=True, best=0.1, want=ALL, top_k=4)
        out.update({"acq_" + k: v for k, v in a.items()})
        sp = p.sample_paths(Xt, OA.draws(c), top_k=4)
        out.update({"sp_" + k: v for k, v in sp.items()})
        ra, rb, _ = refine_calls(p, c)
        out.update({"rf_" + k: v for k, v in ra.items()})
        out.update({"prf_" + k: v for k, v in rb.items()})
        if has_training:
            out["train_sums"], out["train_means"] = p.train_stats(want_means=True)
    return out


def equal_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def pin(p, s, targets=True, has_training=True):
    """every check of the module docstring on the state p is in; returns the fetched operands.
    has_training=False: a predictor loaded into a fresh problem.  It has no training means, and until an observation re-forms
    them its R~^-1 = U R^-1 and R~ = R U^-1 are two separate products of the loaded R (do_load_predictor), not an inverse pair
    to the bound of a triangular inversion, and its t is the caller's: the two state checks belong to the observed states."""
    c = s.c
    label = OA.state_id(s)
    args = split(c, 1)[5]
    dev = Device(p, targets, has_training)
    ops = dev.fetch()
    assert all(np.all(np.isfinite(v)) for v in ops.values()), label
    skipped = set() if has_training else {"train_means", "state.rinv", "state.t"}
    if s.route == "A":      # (the loaded variant after its observation: the state checks hold, there are no training inputs)
        skipped -= {"state.rinv", "state.t"}
    r = OA.ratios(dev, c, ops, only=set(OA.OUTPUTS) - skipped)
    for name, v in sorted(r.items()):
        print("%s %s: worst error / bound %.3g" % (label, name, v))
        M.record("observe.after." + name, v, 1.0, route=s.route, m=c.m, k=s.k, variant=s.variant + ("-forced" if c.forced else ""), d=c.d)
    assert set(r) == set(OA.OUTPUTS if targets else OA.OUTPUTS_MODEL_ONLY) - skipped, sorted(r)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, (label, bad)
    # the outputs each alone, the exact bits at far points; both covariance kinds, the sampler on the FITC matrix
    Xt, far = OA.points_at(c, OA.NT)
    o3 = Operands(ops.get("t"), ops["uinv"], ops["rinv"])
    check_predict_at(p, Xt, far, OA.geometry(c, OA.NT), SIGMA2, args["log_sf2"], o3, label, means=targets)
    for nt in OA.NT_COV:
        cov = check_covariances_at(p, OA.points_at(c, nt)[0], OA.geometry(c, nt), SIGMA2, o3, "%s-nt%d" % (label, nt))
    nt = OA.NT_COV[-1]
    L = cov_samples_raw(p, np.asfortranarray(np.triu(cov)), nt, nt, 0.05, np.zeros(nt), np.eye(nt))
    A = np.triu(cov).astype(R.LD)
    A[np.diag_indices(nt)] += R.LD(0.05) + R.LD(JITTER)
    fr = factor_ratio(np.ascontiguousarray(L.T), A)[0]
    M.record("observe.after.sampler_factor", fr, 4.0, route=s.route, m=c.m, k=s.k, variant=s.variant)
    assert fr <= 4.0 and np.all(np.triu(L, 1) == 0.0), (label, fr)
    rng = np.random.default_rng(nt)
    mu0, zz = rng.normal(size=nt), rng.normal(size=(nt, 5))
    ref, bound = R.samples(L, mu0, zz)
    rs = R.ratio(cov_samples_raw(p, np.asfortranarray(np.triu(cov)), nt, nt, 0.05, mu0, zz), ref, bound)[0]
    M.record("observe.after.cov_samples", rs, 1.0, route=s.route, m=c.m, k=s.k, variant=s.variant)
    assert rs <= 1.0, (label, "cov_samples", rs)
    if not targets:
        return ops
    # acquire: the four criteria at the device's own posterior (pinned above), top_k = 4
    live = OA.live(c)
    post = p.predict_input_grad(live, predictive=False)
    best = float(np.median(post["means"]))
    M.note(kind=c.kind, n=N, m=c.m, d=c.d, D=live.shape[0], nt=live.shape[1], route=s.route, k=s.k, variant=s.variant)
    for kind in AR.KINDS:
        kw = _kw(kind, True, 0.0, best, 1e-10 * np.exp(args["log_sf2"]))
        got = p.acquire(live, kind, want=ALL, top_k=4, **kw)
        _layer_a("observe.after.acquire.%s" % AR.KIND_NAMES[kind], kind, kw, post, got, proj=c.kind == "proj")
        _check_top(got, got, 4)
    # sample_paths: per-draw top-k on the pinned samples (the lower index first among equal values)
    z = OA.draws(c)
    sp = p.sample_paths(Xt, z, top_k=4)
    check_weights(p, c, ops, z, label)
    for j in range(OA.NS):
        order = np.argsort(-sp["samples"][:, j], kind="stable")[:4]
        assert np.array_equal(sp["top_index"][:, j], order) and np.array_equal(sp["top_values"][:, j], sp["samples"][order, j]), (label, j)
    # the two refinement calls from their traces
    ra, rb, (lo, hi, kw, dr) = refine_calls(p, c, trace=True)
    check_refine_trace(p, "observe.after.acquire_refine", ra, "ei", kw, lo, hi, None, OPTS, proj=c.kind == "proj")
    Aw = check_weights(p, c, ops, z, label + "-refine")      # (the weights of the last call that formed any: sample_paths_refine)
    pts, flat, who = _records(rb, live.shape[0])
    D = live.shape[0]
    check_evaluator(label, "observe.after.path_refine", c, Aw, dr[who], 1.0, pts, flat[:, 2 * D], flat[:, D:2 * D].T)
    _check_rule("observe.after.path_refine", rb, lo, hi, None, OPTS)
    return ops


def observed(s, monkeypatch):
    """the problem of a state on routes A - D, and the bits route D has to give back"""
    p = opened(s, monkeypatch)
    targets, has_training = s.variant != "model-only", s.variant != "loaded"
    try:
        before = None
        if s.route == "B":
            downstream(p, s.c, targets, has_training)
        if s.route == "D":
            before = downstream(p, s.c, targets, has_training)
            p.posterior_save()
        total = 0
        for Xn, yn in OA.rows_of(s):
            p.observe(Xn, yn if targets else None)
            total += Xn.shape[1]
        assert p.observed_count == total
        if s.route == "D":
            downstream(p, s.c, targets, has_training)
            p.posterior_restore()
            assert p.observed_count == 0
    except Exception:
        p.close()
        raise
    return p, before


def refusals(p, c):
    """status of every call that needs means, None where it is served"""
    Xt = OA.live(c)
    lo, hi = box_of(c)
    calls = dict(pgrad=lambda: p.predict_input_grad(Xt), mean=lambda: p.predict(Xt),
                 acquire=lambda: p.acquire(Xt, "ei", maximise=True, best=0.1),
                 paths=lambda: p.sample_paths(Xt, OA.draws(c)),
                 refine=lambda: p.acquire_refine(Xt[:, :4], "ei", lower=lo, upper=hi, maximise=True, best=0.1, **OPTS),
                 path_refine=lambda: p.sample_paths_refine(Xt[:, :4], OA.draws(c), np.zeros(4, np.int32), lower=lo, upper=hi, **OPTS),
                 stats=lambda: p.train_stats())
    out = {}
    for name, call in calls.items():
        try:
            call()
            out[name] = None
        except gpr_amd.GprHipError as e:
            out[name] = e.status
    return out


ABCD = [s for s in OA.STATES if s.route in "ABCD"]


@gpu
@pytest.mark.parametrize("s", ABCD, ids=OA.state_id)
def test_every_call_on_the_state_against_its_own_operands(s, monkeypatch):
    targets, has_training = s.variant != "model-only", s.variant != "loaded"
    if not targets:
        q = opened(s, monkeypatch)
        try:
            expected = refusals(q, s.c)
        finally:
            q.close()
        assert any(v is not None for v in expected.values()), expected
    p, before = observed(s, monkeypatch)
    try:
        if not targets:
            assert refusals(p, s.c) == expected, (refusals(p, s.c), expected)
        U0, cond0 = None, None
        if s.route == "A":      # chol_km and cond_km keep their bits across the observation
            q = opened(s, monkeypatch)
            try:
                U0, cond0 = q.co_variance_coeffs()[0], (q.condition() if has_training else None)
            finally:
                q.close()
        ops = pin(p, s, targets, has_training)
        if U0 is not None:
            assert np.array_equal(p.co_variance_coeffs()[0], U0) and (cond0 is None or p.condition() == cond0)
        if s.route == "D":      # the bits of the calls made before the save
            assert equal_bits(downstream(p, s.c, targets, has_training), before)
        if s.route == "C":      # the refit of the n + 64 + 3 rows from scratch in 80 bits, at TOL_POST (tests/test_gpu_observe.py)
            X, y, _, _, Z, args = split(s.c, 1)
            rows = OA.rows_of(s)
            Xall = np.asfortranarray(np.hstack([X] + [r[0] for r in rows]))
            yall = np.concatenate([y] + [r[1] for r in rows])
            Xt = OA.live(s.c)
            ref = O.posterior_from_scratch(Xall, yall, Z, Xt, SIGMA2, **OA.kernel_of(s.c))
            mean, var = p.predict(Xt, predictive=False)
            M.check_vec("observe.after.refit_c.mean", mean, ref["means"].astype(np.float64), TOL_POST)
            M.check_vec("observe.after.refit_c.variance", var, ref["variances"].astype(np.float64), TOL_POST)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("s", [s for s in OA.STATES if s.route == "A" and s.variant == "base" and s.c.m in OA.REFIT_MS
                               and s.c.d == 3 and not s.c.forced], ids=OA.state_id)
def test_route_a_against_the_refit_of_all_rows_from_scratch(s, monkeypatch):
    """Gradients at TOL_GRAD and values at TOL_POST (tests/test_gpu_predict_grad.py against predict_grad_ref), sample paths at
    TOL_POST per draw (tests/test_gpu_sample_paths.py against sample_paths_ref), acquisition values within the bound of
    tests/test_gpu_acquire.py::test_values_end_to_end around the criterion at the 80-bit posterior of the n + k rows."""
    c = s.c
    X, y, _, _, Z, args = split(c, 1)
    Xn, yn = OA.rows_of(s)[0]
    Xall, yall = np.asfortranarray(np.hstack([X, Xn])), np.concatenate([y, yn])
    Xt = OA.live(c)
    ok = OA.oracle_kernel(c)
    p, _ = observed(s, monkeypatch)
    try:
        got = p.predict_input_grad(Xt, predictive=False)
        paths = p.sample_paths(Xt, OA.draws(c))["samples"]
        ref = predict_grad_ref(ok, Z, Xall, yall, SIGMA2, Xt, predictive=False)
        M.note(kind=c.kind, n=N, m=c.m, d=c.d, k=s.k, route=s.route)
        for name, tol in OA.PGRAD_TOL.items():
            M.check_vec("observe.after.refit.pgrad." + name, got[name], ref[name], tol)
        sref = SPR.sample_paths_ref(ok, Z, Xall, yall, SIGMA2, Xt, OA.draws(c))["samples"]
        for j in range(OA.NS):
            M.check_vec("observe.after.refit.paths", paths[:, j], sref[:, j], TOL_POST)
        mu_max, var_max = float(np.max(np.abs(ref["means"]))), float(np.max(ref["variances"]))
        best = float(np.median(ref["means"]))
        for kind in AR.KINDS:
            name = AR.KIND_NAMES[kind]
            kw = _kw(kind, True, 0.0, best, 1e-10 * np.exp(args["log_sf2"]))
            vals = p.acquire(Xt, kind, want=("values",), **kw)["values"]
            a, cmu, cv, us = AR.evaluate(kind, ref["means"], ref["variances"], **_ref_kw(kw))
            worst = 0.0
            for r in range(Xt.shape[1]):
                f = 1 + us[r] * us[r]
                sigma = float(np.sqrt(ref["variances"][r]))
                layer_a = C[name] * EPS * f * ((1 + abs(np.log(sigma))) if kind == AR.LOG_EI else abs(a[r]))
                bound = abs(cmu[r]) * TOL_POST * mu_max + abs(cv[r]) * TOL_POST * var_max + layer_a
                worst = max(worst, float(abs(float(vals[r]) - a[r]) / bound))
            M.record("observe.after.refit.acquire." + name, worst, 1.0, m=c.m, k=s.k)
            assert worst <= 1.0, (name, worst)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("s", [s for s in OA.STATES if s.route == "E"], ids=OA.state_id)
def test_the_export_of_an_observed_state_loaded_into_a_fresh_problem(s, monkeypatch):
    c = s.c
    X, y, _, _, Z, args = split(c, 1)
    donor, _ = observed(s._replace(route="A"), monkeypatch)
    q = problem(c)
    try:
        Xt = OA.points_at(c, OA.NT)[0]
        mean, var = donor.predict(Xt)
        q.load_predictor(sigma2=SIGMA2, inducing=Z, coeffs=donor.debug_fetch("t"), co_variance_coeffs=donor.co_variance_coeffs(), **args)
        assert q.observed_count == 0
        pin(q, s, True, has_training=False)
        m2, v2 = q.predict(Xt)
        M.check_vec("observe.after.export.mean", m2, mean, TOL_POST)
        M.check_vec("observe.after.export.variance", v2, var, TOL_POST)
    finally:
        donor.close()
        q.close()


@gpu
@pytest.mark.parametrize("s", [s for s in OA.STATES if s.route == "F"], ids=OA.state_id)
def test_a_reusing_evaluation_after_an_observation_is_the_refit_of_the_first_rows(s, monkeypatch):
    c = s.c
    X, y, _, _, Z, args = split(c, 1)
    outs = []
    for observe in (True, False):
        p = opened(s, monkeypatch)
        try:
            if observe:
                p.observe(*OA.rows_of(s)[0])
            ev = p.eval(sigma2=OA.SIGMA2_F, inducing=Z, want_grad=False, reuse_v=True, **args)
            assert p.observed_count == 0
            dev = Device(p)
            outs.append(dict(downstream(p, c), l=np.array([ev.l]), coeffs=ev.coeffs, **dev.fetch()))
        finally:
            p.close()
    assert equal_bits(outs[0], outs[1]), [k for k in outs[0] if not np.array_equal(outs[0][k], outs[1][k], equal_nan=True)]
