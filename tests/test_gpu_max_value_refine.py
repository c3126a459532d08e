"""gprhip_acquire_max_value_refine on the device, checked from its trace alone (no replay), as tests/test_gpu_refine.py checks
gprhip_acquire_refine -- its _check runs here unchanged, with the criterion's part answered by max-value entropy search:

1. every record's (a_y, g_y) is the criterion at the traced y -- tests/test_gpu_max_value.py's _hold (mpmath at the device's own
   posterior at the traced points, the constants C of tests/max_value_ref.py), and Problem.acquire_max_value at the traced
   points bit for bit: asserted on route 2 (the same kernel binary runs); on route 1 recorded through tests/margins.py and,
   since it held in every call of the first full run (profiles/max_value_refine_margins.txt), asserted too (ROUTE_1_BITWISE);
2. every record obeys the rule of gpr_amd/csrc/refine_step.h given the previous state (_check of tests/test_gpu_refine.py: y
   within 2 ulp, alpha exact, the Armijo flag on the traced numbers with its tie band, at most 2 % of a shape's records skipped);
3. accepted values never decrease, x / values / dvalues are the last accepted record bit for bit, evals / accepted / status are
   those of the trace;
4. independence and determinism; 5. the refined top 16 of a coarse grid beat a 64 x finer grid; 6. the edges;
7. Problem.max_value_search(refine_top_k=...) end to end.

Route 1 is the persistent kernel (m <= 64, d <= 16, no projection), route 2 the library-side loop.  The extremes of a case
are fixed by the rule of tests/max_value_refine_cases.py from the posterior over the case's box; tools/max_value_refine_precheck.py
runs the trace cases on the CPU (profiles/max_value_refine_precheck.txt)."""
import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import margins as M
from tests import max_value_ref as R
from tests import max_value_refine_cases as MC
from tests import refine_cases as RC
from tests import refine_ref as RR
from tests import test_gpu_max_value as MV
from tests import test_gpu_refine as TR

gpu = pytest.mark.gpu
EPS = 2.0 ** -53
FLOOR = MC.VAR_FLOOR
ALL = ("values", "dvalues", "means", "variances")
NAMES = gpr_amd.Problem.REFINE_OUTPUTS
# 8 evaluations per start: the rule's every branch (first step, grow, shrink, the two ends) within the first few, and the
# mpmath check of every record stays within seconds
OPTS = dict(TR.OPTS, max_evals=8)
OPTS_64 = dict(TR.OPTS, max_evals=4)   # S = 64: sixteen extremes per lane, 64 mpmath terms per record
# Whether a route 1 trace is ASSERTED to equal Problem.acquire_max_value at the traced points bit for bit (it is recorded in
# either case).  In the first full run on the device it held in every call of both routes, the edges included
# (profiles/max_value_refine_margins.txt): asserted.
ROUTE_1_BITWISE = True
COMBOS = [(True, False), (False, True), (True, True), (False, False)]   # (maximise, with scale)


class _AsAcquire:
    """What TR._check asks of a problem, answered by the max-value calls: the posterior at the traced points, and `acquire`
    at them -- Problem.acquire_max_value.  Where the bit-for-bit comparison is recorded and not asserted (route 1 before the
    first full run), `acquire` hands the trace itself back after recording what the comparison gave."""

    def __init__(self, p, what, ext, maximise, floor, assert_bits):
        self.p, self.what, self.ext, self.maximise, self.floor, self.assert_bits = p, what, ext, maximise, floor, assert_bits
        self.m, self.d = p.m, p.d
        self.traced = None

    def predict_input_grad(self, pts, **kw):
        return self.p.predict_input_grad(pts, **kw)

    def acquire(self, pts, kind, **kw):
        direct = self.p.acquire_max_value(pts, self.ext, maximise=self.maximise, var_floor=self.floor)
        same = np.array_equal(direct["values"], self.traced[0]) and np.array_equal(direct["dvalues"], self.traced[1])
        print("%s: trace equals Problem.acquire_max_value at the traced points bit for bit: %s" % (self.what, same))
        M._record("%s.bitwise_max_value" % self.what, 0.0 if same else 1.0, 1.0)
        return direct if self.assert_bits else dict(values=self.traced[0], dvalues=self.traced[1])


def _check(monkeypatch, p, what, out, ext, maximise, floor, lo, hi, scale, opts, route, tproj=None):
    """checks 1 - 3 on one call's outputs through TR._check; returns (records, skipped)"""
    D, ns = out["x"].shape
    key = ("proj",) if tproj is not None else ("iso",)

    def hold(what_, kind, kw, post, got, proj=False):
        MV._hold(what_, key, post, got, ext, maximise, floor, signs=False)
    monkeypatch.setattr(TR, "_layer_a", hold)
    monkeypatch.setattr(TR, "Problem_kind", lambda kind: kind)
    monkeypatch.setattr(MV, "_case", lambda *k: (None, None, None, dict(tproj=tproj)))
    q = _AsAcquire(p, what, ext, maximise, floor, route == 2 or ROUTE_1_BITWISE)
    flat = np.concatenate([out["trace"][i, :out["evals"][i]] for i in range(ns)])
    q.traced = (flat[:, 2 * D].copy(), np.asfortranarray(flat[:, D:2 * D].T))
    return TR._check(q, what, out, "max_value", {}, lo, hi, scale, opts, proj=tproj is not None)


def _extremes(p, lo, hi, S, maximise):
    post = p.predict_input_grad(MC.box_points(lo, hi), predictive=False, want=("means", "variances"))
    return MC.extremes(post["means"], post["variances"], S, maximise)


def _calls(ns_list, S):
    """every shape maximising and minimising, with and without scale: the four combinations cycled over the shape's ns; at
    S = 64, where a record costs 64 mpmath terms, the first two -- maximising without and minimising with scale"""
    combos = COMBOS[:2] if S == 64 else COMBOS
    n = max(len(ns_list), len(combos))
    return [(ns_list[j % len(ns_list)],) + combos[j % len(combos)] for j in range(n)]


def _run_shape(monkeypatch, m, d, ns_list, S, D=None, route=None):
    X, y, Z, args = RC.data(m, d, D)
    p = TR._problem(X, y, Z, args)
    Dd = X.shape[0]
    lo, hi = MC.box(Dd)
    opts = OPTS_64 if S == 64 else OPTS
    total = skipped = 0
    try:
        ext = {mx: _extremes(p, lo, hi, S, mx) for mx in (True, False)}
        p.set_timing(2)
        for ci, (ns, maximise, scaled) in enumerate(_calls(ns_list, S)):
            scale = np.linspace(0.5, 1.5, Dd) if scaled else None
            St = TR._starts(Dd, ns, lo, hi, 7 * ns + ci)
            kw = dict(lower=lo, upper=hi, scale=scale, maximise=maximise, var_floor=FLOOR)
            out = p.acquire_max_value_refine(St, ext[maximise], want=NAMES, **kw, **opts)
            stages = p.last_timings()
            assert ("rf_small" in stages) == (route == 1) and ("rf_step" in stages) == (route == 2), stages
            what = "mvrefine.r%d.m%d_d%d_ns%d_S%d.%s%s" % (route, m, d, ns, S, "max" if maximise else "min", ".scaled" if scaled else "")
            r, s = _check(monkeypatch, p, what, out, ext[maximise], maximise, FLOOR, lo, hi, scale, opts, route, tproj=args.get("tproj"))
            total += r
            skipped += s
            # two runs give the same bits; without the trace all other outputs have the same bits
            again = p.acquire_max_value_refine(St, ext[maximise], **kw, **opts)
            assert all(np.array_equal(again[k], out[k]) for k in again), what
        print("mvrefine.r%d.m%d_d%d_S%d: %d records, %d skipped as ties" % (route, m, d, S, total, skipped))
        assert skipped <= 0.02 * max(total, 1), (total, skipped)
    finally:
        p.close()


ROUTE_1 = [(50, 3, (1, 16, 17, 64, 65, 130), 5), (5, 1, (17, 130), 5), (64, 16, (1, 65), 5), (50, 16, (17,), 5), (64, 1, (64,), 5),
           (50, 3, (65,), 1), (50, 3, (65,), 64)]
ROUTE_2 = [(65, 3, None, (1, 17), 5), (130, 2, None, (130,), 5), (50, 17, None, (17,), 5), (20, 2, 5, (1, 17, 130), 5),
           (65, 3, None, (17,), 64)]


@gpu
@pytest.mark.parametrize("m,d,ns_list,S", ROUTE_1, ids=str)
def test_route_1_trace_obeys_the_rule_and_the_criterion(monkeypatch, m, d, ns_list, S):
    _run_shape(monkeypatch, m, d, ns_list, S, route=1)


@gpu
@pytest.mark.parametrize("m,d,D,ns_list,S", ROUTE_2, ids=str)
def test_route_2_trace_obeys_the_rule_and_the_criterion(monkeypatch, m, d, D, ns_list, S):
    _run_shape(monkeypatch, m, d, ns_list, S, D=D, route=2)


@gpu
@pytest.mark.parametrize("m,d", [(50, 3), (65, 3)], ids=str)
def test_independence_permutation_lanes_and_device_buffers(m, d):
    import torch
    p, D, _, X = TR._model(m, d)
    lo, hi = np.zeros(D), np.ones(D)
    names = NAMES

    def col(out, i):
        return {k: (out[k][:, i] if k in ("x", "dvalues") else out[k][i]) for k in names}

    def same(a, b):
        return all(np.array_equal(a[k], b[k], equal_nan=(k == "trace")) for k in names)
    try:
        ext = _extremes(p, lo, hi, 5, True)
        kw = dict(lower=lo, upper=hi, maximise=True, var_floor=FLOOR, want=names, **TR.OPTS)
        S = TR._starts(D, 130, lo, hi, 5)
        full = p.acquire_max_value_refine(S, ext, **kw)
        assert np.any(full["accepted"] > 0)
        perm = np.random.default_rng(1).permutation(130)
        shuffled = p.acquire_max_value_refine(np.asfortranarray(S[:, perm]), ext, **kw)
        for j, i in enumerate(perm):
            assert same(col(shuffled, j), col(full, i)), (i, j)
        for i in (0, 63, 64, 129):   # alone, and as lane 0 / lane 63 of a full workgroup of other starts
            alone = p.acquire_max_value_refine(np.asfortranarray(S[:, [i]]), ext, **kw)
            assert same(col(alone, 0), col(full, i)), i
            others = [j for j in range(64) if j != i][:63]
            for pos in (0, 63):
                cols = others[:pos] + [i] + others[pos:]
                wg = p.acquire_max_value_refine(np.asfortranarray(S[:, cols]), ext, **kw)
                assert same(col(wg, pos), col(full, i)), (i, pos)
        # two runs; without the trace the other outputs have the same bits
        again = p.acquire_max_value_refine(S, ext, **dict(kw, want=names[:-1]))
        assert all(np.array_equal(again[k], full[k]) for k in again) and "trace" not in again
        # device buffers
        dev = torch.device("cuda:0")
        st = torch.tensor(np.ascontiguousarray(S.T), device=dev)
        shapes = dict(x=(130, D), dvalues=(130, D), values=(130,), evals=(130,), accepted=(130,), status=(130,),
                      trace=(130, TR.OPTS["max_evals"], 2 * D + 3))
        outs = {k: (torch.full(shapes[k], -1, dtype=torch.int32, device=dev) if k in ("evals", "accepted", "status")
                    else torch.full(shapes[k], float("nan"), dtype=torch.float64, device=dev)) for k in names}
        torch.cuda.synchronize()
        assert p.acquire_max_value_refine(st.data_ptr(), ext, out_device_ptrs={k: v.data_ptr() for k, v in outs.items()}, ns=130,
                                          **kw) == {}
        for k in names:
            g = outs[k].cpu().numpy()
            assert np.array_equal(g.T if k in ("x", "dvalues") else g, full[k], equal_nan=(k == "trace")), k
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("d", [1, 2])
def test_refined_top_16_of_a_coarse_grid_beats_a_64_times_finer_grid(d):
    """The bump model of tests/refine_cases.py with the extremes of tests/max_value_refine_cases.py's rule (S = 5) from the
    coarse grid: tests/test_max_value_refine_host.py shows on the CPU that the criterion's maximiser lies inside the box and
    off the coarse grid, and that the refined top 16 beat both grids.  Here: the best refined value >= the best of a grid 64 x
    finer per axis, less the bound of the value R.C["a"] 2^-53 (1 + gamma_max^2) a there; it strictly beats the coarse grid;
    and it lies strictly inside."""
    X, y, Z, args = RC.bump(d)
    p = TR._problem(X, y, Z, args)
    lo, hi = np.zeros(d), np.ones(d)
    nc = RC.COARSE[d]
    coarse, fine = RC.grid(d, nc), RC.grid(d, 64 * (nc - 1) + 1)
    try:
        post = p.predict_input_grad(coarse, predictive=False, want=("means", "variances"))
        ext = MC.extremes(post["means"], post["variances"], 5, True)
        kw = dict(maximise=True, var_floor=FLOOR)
        top = p.acquire_max_value(coarse, ext, top_k=16, want=(), **kw)
        starts = np.asfortranarray(coarse[:, top["top_index"]])
        out = p.acquire_max_value_refine(starts, ext, lower=lo, upper=hi, max_evals=40, **kw)
        fv = p.acquire_max_value(fine, ext, want=("values", "means", "variances"), **kw)
        jf = int(np.argmax(fv["values"]))
        fine_best = float(fv["values"][jf])
        ref = R.point(float(fv["means"][jf]), float(fv["variances"][jf]), ext, maximise=True, var_floor=FLOOR)
        bound = float(R.C["a"] * R.unit(ref) * ref[0])
        j = int(np.argmax(out["values"]))
        got, coarse_best = float(out["values"][j]), float(top["top_values"][0])
        print("mvrefine.does_its_job.d%d: refined %.12g at %s, fine grid %.12g, coarse %.12g" % (d, got, out["x"][:, j], fine_best, coarse_best))
        assert got >= fine_best - bound and got > coarse_best
        assert np.all(out["x"][:, j] > 0.0) and np.all(out["x"][:, j] < 1.0)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("m,d", [(50, 3), (65, 3)], ids=str)
def test_edges(monkeypatch, m, d):
    route = 1 if m <= 64 else 2
    p, D, _, X = TR._model(m, d)
    lo, hi = np.zeros(D), np.ones(D)
    box = dict(lower=lo, upper=hi, var_floor=FLOOR, want=NAMES)
    Xt = TR._starts(D, 9, lo, hi, 2)
    try:
        before = p.predict(Xt)
        ext = _extremes(p, lo, hi, 5, True)
        # a start outside the box is clipped; max_evals = 1 returns it with the value of acquire_max_value there
        S = np.asfortranarray(np.array([[-2.0] * D, [3.0] * D, [0.5] * D]).T)
        one = p.acquire_max_value_refine(S, ext, maximise=True, **box, **dict(OPTS, max_evals=1))
        assert np.array_equal(one["x"], np.clip(S, 0.0, 1.0)) and np.all(one["evals"] == 1) and np.all(one["accepted"] == 0)
        assert one["status"][2] == RR.MAX_EVALS and np.all((one["status"] == RR.MAX_EVALS) | (one["status"] == RR.CONVERGED))
        direct = p.acquire_max_value(np.asfortranarray(np.clip(S, 0.0, 1.0)), ext, maximise=True, var_floor=FLOOR)
        if route == 2 or ROUTE_1_BITWISE:
            assert np.array_equal(one["values"], direct["values"]) and np.array_equal(one["dvalues"], direct["dvalues"])
        assert np.allclose(one["values"], direct["values"], rtol=1e-12, atol=0) and np.array_equal(one["trace"][:, 0, :D].T, one["x"])
        # a clamped variance (var_floor = 10 sf2): c_v = 0, the gradient is c_mu dmu alone, the rule still holds
        Xc = Xt.copy()
        Xc[:, 0] = X[:, 0]  # (a start on a training point)
        for maximise in (True, False):
            e = _extremes(p, lo, hi, 5, maximise)
            cl = p.acquire_max_value_refine(Xc, e, maximise=maximise, lower=lo, upper=hi, var_floor=10.0, want=NAMES, **OPTS)
            _check(monkeypatch, p, "mvrefine.clamped.m%d.%s" % (m, "max" if maximise else "min"), cl, e, maximise, 10.0, lo, hi, None,
                   OPTS, route)
            post = p.predict_input_grad(np.asfortranarray(cl["x"]), predictive=False)
            assert np.all(post["variances"] < 10.0)
            for i in range(Xc.shape[1]):                    # c_v = 0: a start's gradient is one multiple of dmu
                dm, row = post["dmeans"][:, i], cl["dvalues"][:, i]
                j0 = int(np.argmax(np.abs(dm)))
                assert np.allclose(row, (row[j0] / dm[j0]) * dm, rtol=1e-9, atol=1e-9 * abs(row[j0])), (i, row, dm)
        # an extreme 45 sigma beyond every mean on either side, with one in between: values and gradient stay finite and
        # nonzero and the starts move; the far extreme alone on the side of negative gamma likewise (psi ~ gamma^2 / 2)
        postt = p.predict_input_grad(Xt, predictive=False, want=("means", "variances"))
        for maximise in (True, False):
            for e in (MV._extremes(postt, 3, maximise), MV._extremes(postt, 3, not maximise)[:1]):
                far = p.acquire_max_value_refine(Xt, e, maximise=maximise, **box, **OPTS)
                assert np.all(np.isfinite(far["values"])) and np.all(far["values"] > 0.0), (maximise, e)
                assert np.all(np.isfinite(far["dvalues"])) and np.all(np.any(far["dvalues"] != 0.0, axis=0))
                moved = far["accepted"] >= 1    # (a start clipped into a corner that the gradient points out of ends at once)
                assert np.sum(moved) >= 7 and np.all(moved | (far["evals"] == 1)), (far["accepted"], far["evals"])
                assert np.all(far["values"][moved] > far["trace"][moved, 0, 2 * D])
                _check(monkeypatch, p, "mvrefine.far.m%d.S%d.%s" % (m, len(e), "max" if maximise else "min"), far, e, maximise, FLOOR,
                       lo, hi, None, OPTS, route)
        # the far extreme alone on the side of positive gamma (>= 45 at every point): the criterion is below 2^-1074 there --
        # no double holds it, 2^128 carried or not; everything stays finite and the starts end at once
        lone = p.acquire_max_value_refine(Xt, MV._extremes(postt, 3, True)[:1], maximise=True, **box, **OPTS)
        assert np.all(lone["values"] == 0.0) and np.all(lone["dvalues"] == 0.0)
        assert np.all(lone["status"] == RR.CONVERGED) and np.all(lone["evals"] == 1)
        # where phi has left the normal range but the carried 2^128 phi has not (gamma about 37.6 .. 38.6 at the start):
        # value and gradient are nonzero
        x0 = np.asfortranarray(np.clip(Xt[:, :1], 0.0, 1.0))
        q0 = p.predict_input_grad(x0, predictive=False, want=("means", "variances"))
        e38 = np.array([float(q0["means"][0]) + 38.0 * float(np.sqrt(q0["variances"][0]))])
        tiny = p.acquire_max_value_refine(x0, e38, maximise=True, **box, **dict(OPTS, max_evals=1))
        assert 0.0 < tiny["values"][0] < 2.0 ** -1000 and np.any(tiny["dvalues"] != 0.0) and np.all(np.isfinite(tiny["dvalues"]))
        # the refusals leave a following acquire_max_value bit-identical; the predictor state is unchanged
        ref = p.acquire_max_value(Xt, ext, maximise=True, var_floor=FLOOR, want=ALL)
        good = dict(maximise=True, **box, **OPTS)
        for b in (dict(step0=0.0), dict(max_evals=0), dict(shrink=1.0), dict(grow=0.5), dict(c1=1.0), dict(xtol=-1.0),
                  dict(var_floor=0.0), dict(var_floor=float("inf")), dict(lower=hi, upper=lo), dict(upper=np.full(D, np.inf)),
                  dict(scale=np.zeros(D)), dict(scale=np.full(D, np.nan))):
            with pytest.raises(gpr_amd.GprHipError) as err:
                p.acquire_max_value_refine(Xt, ext, **dict(good, **b))
            assert err.value.status == _lib.EBADARG, b
        nan_start = Xt.copy()
        nan_start[0, 3] = np.nan
        for starts, e in ((nan_start, ext), (Xt, np.array([0.3, np.nan])), (Xt, np.zeros(0)), (Xt, np.zeros(65))):
            with pytest.raises(gpr_amd.GprHipError) as err:
                p.acquire_max_value_refine(starts, e, **good)
            assert err.value.status == _lib.EBADARG
        after = p.acquire_max_value(Xt, ext, maximise=True, var_floor=FLOOR, want=ALL)
        assert all(np.array_equal(ref[k], after[k]) for k in ALL)
        now = p.predict(Xt)
        assert np.array_equal(before[0], now[0]) and np.array_equal(before[1], now[1])
        empty = gpr_amd.Problem(gpr_amd.COV_SE_ISO, TR.N, D, D, m)
        try:
            with pytest.raises(gpr_amd.GprHipError) as err:
                empty.acquire_max_value_refine(Xt, ext, **good)
            assert err.value.status == _lib.ESTATE
        finally:
            empty.close()
        after = p.acquire_max_value(Xt, ext, maximise=True, var_floor=FLOOR, want=ALL)
        assert all(np.array_equal(ref[k], after[k]) for k in ALL)
        # after gprhip_observe the updated posterior is used: the trace is the criterion at the new posterior
        was = p.acquire_max_value_refine(Xt, ext, maximise=True, **box, **OPTS)
        p.observe(np.asfortranarray(Xt[:, :4]), postt["means"][:4] + 0.5)
        obs = p.acquire_max_value_refine(Xt, ext, maximise=True, **box, **OPTS)
        assert not np.array_equal(obs["values"], was["values"])
        _check(monkeypatch, p, "mvrefine.observed.m%d" % m, obs, ext, True, FLOOR, lo, hi, None, OPTS, route)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("maximise", [True, False], ids=["max", "min"])
def test_max_value_search_refines_its_best_candidates_end_to_end(maximise):
    p, D, _, X = TR._model(50, 3)
    m, nd, k = 50, 4, 3
    lo, hi = MC.box(D)
    grid = np.asfortranarray(lo[:, None] + (hi - lo)[:, None] * np.random.default_rng(3).uniform(size=(D, 130)))
    z = np.asfortranarray(np.random.default_rng(11).normal(size=(m, nd)))
    opts, copts = dict(max_evals=30), dict(max_evals=20, xtol=1e-7)
    try:
        out = p.max_value_search(z, lo, hi, grid, k, opts, maximise=maximise, want=ALL, acquire_top_k=2, refine_top_k=4,
                                 candidate_refine_options=copts)
        assert len(out["top_index"]) == 4 and np.all(out["top_index"] >= 0)
        # (a start that accepts no step keeps the persistent kernel's own value of the grid point)
        slack = 0.0 if ROUTE_1_BITWISE else 1e-12
        assert np.all(out["refined_values"] >= out["top_values"] * (1.0 - slack)) and np.all(out["refined_status"] != RR.NAN)
        assert np.any(out["refined_values"] > out["top_values"])
        assert np.all(out["refined_x"] >= lo[:, None]) and np.all(out["refined_x"] <= hi[:, None])
        direct = p.acquire_max_value_refine(grid[:, out["top_index"]], out["extremes"], lower=lo, upper=hi, maximise=maximise,
                                            want=("x", "values", "dvalues", "status"), **copts)
        for name in direct:
            assert np.array_equal(direct[name], out["refined_" + name]), name
        # refine_top_k = 0: the dict of the method as it was -- acquire_max_value's on the extremes, plus the two extremes keys
        plain = p.max_value_search(z, lo, hi, grid, k, opts, maximise=maximise, want=ALL, acquire_top_k=2, refine_top_k=0)
        default = p.max_value_search(z, lo, hi, grid, k, opts, maximise=maximise, want=ALL, acquire_top_k=2)
        assert np.array_equal(plain["extremes"], out["extremes"])
        old = p.acquire_max_value(grid, plain["extremes"], maximise=maximise, want=ALL, top_k=2)
        assert set(plain) == set(default) == set(old) | {"extremes", "extreme_x"}
        for name in old:
            assert np.array_equal(old[name], plain[name], equal_nan=True) and np.array_equal(old[name], default[name], equal_nan=True)
        assert np.array_equal(plain["extreme_x"], default["extreme_x"]) and np.array_equal(plain["extreme_x"], out["extreme_x"])
    finally:
        p.close()
