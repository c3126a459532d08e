"""gprhip_acquire_refine on the device, checked from its trace alone (no replay):

1. every record's (a_y, g_y) is the criterion at the traced y -- the layer-A check of tests/test_gpu_acquire.py (_layer_a, its
   constants C) against the device's own posterior at the traced points, and Problem.acquire at the traced points;
2. every record obeys the rule of gpr_amd/csrc/refine_step.h given the previous state: y = clip(x + alpha dir) within 2 ulp
   (FMA contraction), y inside the box, alpha by grow / shrink exactly, the accepted flag the Armijo inequality on the traced
   numbers -- a record is skipped only when the two sides differ by less than 8 2^-53 (|a| + |a_y| + c1 sum |g_k delta_k|), and
   at most 2 % of the records are;
3. accepted values never decrease, x / values / dvalues are the last accepted record bit for bit, evals / accepted / status are
   those of the trace, CONVERGED means the stated condition on the traced numbers;
4. independence and determinism; 5. the refined top-16 of a coarse grid beats a 64 x finer grid; 6. the edges.

Route 1 is the persistent kernel (m <= 64, d <= 16, no projection), route 2 the library-side loop."""
import math

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import acquire_ref as R
from tests import margins as M
from tests import refine_cases as RC
from tests import refine_ref as RR
from tests.test_gpu_acquire import ALL, C, _layer_a

gpu = pytest.mark.gpu
N, SIGMA2 = RC.N, RC.SIGMA2
OPTS = dict(max_evals=12, step0=0.1, c1=1e-4, shrink=0.5, grow=2.0, xtol=1e-7)
EPS = 2.0 ** -53
KINDS = [("ei", True, {}), ("log_ei", False, {}), ("pi", True, {}), ("bound", False, dict(kappa=2.0)), ("bound", True, dict(kappa=0.0))]


def _problem(X, y, Z, args):
    D, d, m = X.shape[0], Z.shape[0], Z.shape[1]
    p = gpr_amd.Problem(gpr_amd.COV_SE_FAT if "tproj" in args else gpr_amd.COV_SE_ISO, N, D, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(want_grad=False, sigma2=SIGMA2, inducing=Z, **args)
    return p


def _model(m, d, D=None, seed=0):
    """the ridge model of tests/refine_cases.py on the device: (problem, D, (min y, max y), X)"""
    X, y, Z, args = RC.data(m, d, D, seed)
    return _problem(X, y, Z, args), X.shape[0], (float(np.min(y)), float(np.max(y))), X


def _kw(kind, maximise, best, extra):
    """the incumbent is the best target seen, as a user of the criteria would set it: PI and EI do not saturate"""
    best = best[1] if maximise else best[0]
    return dict(maximise=maximise, best=best, xi=0.0, kappa=extra.get("kappa", 0.0), var_floor=1e-10, predictive=False)


def _ulps(a, b):
    return abs(a - b) / (np.spacing(max(abs(a), abs(b))) or 1.0)


def _check(p, what, out, kind, kw, lo, hi, scale, opts, proj=False):
    """checks 1 - 3 on one call's outputs; returns (records, skipped)"""
    D, ns = out["x"].shape
    tr = out["trace"]
    sc = np.ones(D) if scale is None else scale
    w = hi - lo
    pts = np.asfortranarray(np.concatenate([tr[i, :out["evals"][i], :D] for i in range(ns)]).T)
    assert np.all(np.isfinite(pts)) and np.all(pts >= lo[:, None]) and np.all(pts <= hi[:, None]), what
    # 1: the criterion at the traced points, by the check of tests/test_gpu_acquire.py
    flat = np.concatenate([tr[i, :out["evals"][i]] for i in range(ns)])
    post = p.predict_input_grad(pts, predictive=False)
    got = dict(values=flat[:, 2 * D].copy(), dvalues=np.asfortranarray(flat[:, D:2 * D].T), means=post["means"],
               variances=post["variances"])
    M.note(kind="refine", n=N, m=p.m, d=p.d, D=D, nt=pts.shape[1])
    _layer_a(what, Problem_kind(kind), kw, post, got, proj=proj)
    direct = p.acquire(pts, kind, **kw)
    same = np.array_equal(direct["values"], got["values"]) and np.array_equal(direct["dvalues"], got["dvalues"])
    print("%s: trace equals Problem.acquire at the traced points bit for bit: %s" % (what, same))
    M._record("%s.bitwise_acquire" % what, 0.0 if same else 1.0, 1.0)
    # (profiles/refine_margins.txt: equal in every call on both routes -- route 2 runs the very kernels of acquire, route 1
    #  the same body text)
    assert same, what
    records = skipped = 0
    for i in range(ns):
        ev, acc, st = int(out["evals"][i]), int(out["accepted"][i]), int(out["status"][i])
        assert 1 <= ev <= opts["max_evals"] and np.all(np.isnan(tr[i, ev:])), (what, i)
        x, g, a = tr[i, 0, :D], tr[i, 0, D:2 * D], tr[i, 0, 2 * D]
        assert tr[i, 0, 2 * D + 1] == 0.0 and tr[i, 0, 2 * D + 2] == 1.0
        alpha, nacc = None, 0

        def dirs(x, g):
            return np.array([RR.direction(g[k], sc[k], x[k], lo[k], hi[k]) for k in range(D)])
        d = dirs(x, g)
        if np.max(np.abs(d)) > 0:
            alpha = (opts["step0"] * np.min(w)) / np.max(np.abs(d))
        for j in range(1, ev):
            y, gy, ay, al, flag = tr[i, j, :D], tr[i, j, D:2 * D], tr[i, j, 2 * D], tr[i, j, 2 * D + 1], tr[i, j, 2 * D + 2]
            records += 1
            assert al == alpha, (what, i, j, al, alpha)
            for k in range(D):
                want = RR.trial(x[k], al, d[k], lo[k], hi[k])
                assert _ulps(y[k], want) <= 2.0, (what, i, j, k, y[k], want)
            delta = y - x
            assert np.max(np.abs(delta) / w) > opts["xtol"], (what, i, j)
            lhs, rhs = ay, a + opts["c1"] * float(np.dot(g, delta))
            if abs(lhs - rhs) < 8 * EPS * (abs(a) + abs(ay) + opts["c1"] * float(np.sum(np.abs(g * delta)))):
                skipped += 1
            else:
                assert (flag == 1.0) == (lhs >= rhs), (what, i, j, lhs, rhs, flag)
            if flag == 1.0:
                assert ay >= a, (what, i, j)  # 3: accepted values never decrease (c1 >= 0, g . delta >= 0)
                x, g, a = y, gy, ay
                nacc += 1
                d = dirs(x, g)
                alpha = al * opts["grow"]
            else:
                assert flag == 0.0
                alpha = al * opts["shrink"]
        assert nacc == acc, (what, i)
        assert np.array_equal(out["x"][:, i], x) and np.array_equal(out["dvalues"][:, i], g) and out["values"][i] == a, (what, i)
        if st == RR.CONVERGED:
            if np.max(np.abs(d)) > 0:
                y = np.array([RR.trial(x[k], alpha, d[k], lo[k], hi[k]) for k in range(D)])
                assert np.max(np.abs(y - x) / w) <= opts["xtol"] * (1 + 8 * EPS), (what, i)
        else:
            assert st == RR.MAX_EVALS and ev == opts["max_evals"], (what, i, st, ev)
    return records, skipped


def Problem_kind(kind):
    return gpr_amd.Problem.ACQUIRE_KINDS[kind]


def _starts(D, ns, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(lo[:, None] + (hi - lo)[:, None] * rng.uniform(-0.05, 1.05, size=(D, ns)))


def _run_shape(m, d, ns_list, D=None, route=None, kinds=KINDS):
    p, Dd, best, _ = _model(m, d, D)
    lo, hi = np.full(Dd, 0.05), np.linspace(0.9, 1.1, Dd)
    total = skipped = 0
    try:
        p.set_timing(2)
        for ns in ns_list:
            for ki, (kind, maximise, extra) in enumerate(kinds):
                kw = _kw(kind, maximise, best, extra)
                scale = None if ki % 2 == 0 else np.linspace(0.5, 1.5, Dd)
                S = _starts(Dd, ns, lo, hi, 7 * ns + ki)
                out = p.acquire_refine(S, kind, lower=lo, upper=hi, scale=scale, want=gpr_amd.Problem.REFINE_OUTPUTS,
                                       **{k: v for k, v in kw.items()}, **OPTS)
                stages = p.last_timings()
                assert ("rf_small" in stages) == (route == 1) and ("rf_step" in stages) == (route == 2), stages
                if kind == "bound" and extra["kappa"] == 0.0:
                    assert not {"pg_m", "pg_gemm", "pg_cov"} & set(stages), stages
                what = "refine.r%d.m%d_d%d_ns%d.%s.%s" % (route, m, d, ns, kind, "max" if maximise else "min")
                r, s = _check(p, what, out, kind, kw, lo, hi, scale, OPTS, proj=D is not None)
                total += r
                skipped += s
                # 4: two runs give the same bits; without the trace all other outputs have the same bits
                again = p.acquire_refine(S, kind, lower=lo, upper=hi, scale=scale, **kw, **OPTS)
                assert all(np.array_equal(again[k], out[k]) for k in again), what
        print("refine.r%d.m%d_d%d: %d records, %d skipped as ties" % (route, m, d, total, skipped))
        assert skipped <= 0.02 * max(total, 1), (total, skipped)
    finally:
        p.close()


# (tools/refine_precheck.py runs these cases on the CPU over the 80-bit evaluator: profiles/refine_precheck.txt)
ROUTE_1 = [(50, 3, (1, 16, 17, 64, 65, 130)), (5, 1, (17, 130)), (64, 16, (1, 65)), (5, 16, (16,)), (64, 1, (64,)), (50, 1, (65,)),
           (5, 3, (1,)), (64, 3, (130,)), (50, 16, (17,))]
ROUTE_2 = [(65, 3, None, (1, 17)), (130, 2, None, (130,)), (50, 17, None, (17,)), (20, 2, 5, (1, 17, 130))]


@gpu
@pytest.mark.parametrize("m,d,ns_list", ROUTE_1, ids=str)
def test_route_1_trace_obeys_the_rule_and_the_criterion(m, d, ns_list):
    _run_shape(m, d, ns_list, route=1)


@gpu
@pytest.mark.parametrize("m,d,D,ns_list", ROUTE_2, ids=str)
def test_route_2_trace_obeys_the_rule_and_the_criterion(m, d, D, ns_list):
    _run_shape(m, d, ns_list, D=D, route=2)


@gpu
@pytest.mark.parametrize("m,d", [(50, 3), (65, 3)], ids=str)
def test_independence_permutation_lanes_and_device_buffers(m, d):
    import torch
    p, D, best, X = _model(m, d)
    best = best[1]
    lo, hi = np.zeros(D), np.ones(D)
    kw = dict(lower=lo, upper=hi, maximise=True, best=best, var_floor=1e-10, want=gpr_amd.Problem.REFINE_OUTPUTS, **OPTS)
    names = gpr_amd.Problem.REFINE_OUTPUTS

    def col(out, i):
        return {k: (out[k][:, i] if k in ("x", "dvalues") else out[k][i]) for k in names}

    def same(a, b):
        return all(np.array_equal(a[k], b[k], equal_nan=(k == "trace")) for k in names)
    try:
        S = _starts(D, 130, lo, hi, 5)
        full = p.acquire_refine(S, "log_ei", **kw)
        perm = np.random.default_rng(1).permutation(130)
        shuffled = p.acquire_refine(np.asfortranarray(S[:, perm]), "log_ei", **kw)
        for j, i in enumerate(perm):
            assert same(col(shuffled, j), col(full, i)), (i, j)
        for i in (0, 63, 64, 129):   # alone, and as lane 0 / lane 63 of a full workgroup of other starts
            alone = p.acquire_refine(np.asfortranarray(S[:, [i]]), "log_ei", **kw)
            assert same(col(alone, 0), col(full, i)), i
            others = [j for j in range(64) if j != i][:63]
            for pos in (0, 63):
                cols = others[:pos] + [i] + others[pos:]
                wg = p.acquire_refine(np.asfortranarray(S[:, cols]), "log_ei", **kw)
                assert same(col(wg, pos), col(full, i)), (i, pos)
        # device buffers
        dev = torch.device("cuda:0")
        st = torch.tensor(np.ascontiguousarray(S.T), device=dev)
        shapes = dict(x=(130, D), dvalues=(130, D), values=(130,), evals=(130,), accepted=(130,), status=(130,),
                      trace=(130, OPTS["max_evals"], 2 * D + 3))
        outs = {k: (torch.full(shapes[k], -1, dtype=torch.int32, device=dev) if k in ("evals", "accepted", "status")
                    else torch.full(shapes[k], float("nan"), dtype=torch.float64, device=dev)) for k in names}
        torch.cuda.synchronize()
        assert p.acquire_refine(st.data_ptr(), "log_ei", out_device_ptrs={k: v.data_ptr() for k, v in outs.items()}, ns=130, **kw) == {}
        for k in names:
            g = outs[k].cpu().numpy()
            assert np.array_equal(g.T if k in ("x", "dvalues") else g, full[k], equal_nan=(k == "trace")), k
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("d", [1, 2])
def test_refined_top_16_of_a_coarse_grid_beats_a_64_times_finer_grid(d):
    """The bump model of tests/refine_cases.py, the bound mu + sigma: tests/test_refine_host.py shows on the CPU (80-bit
    posterior, tests/refine_ref.py) that its maximiser lies inside the box and off the coarse grid, and that the refined top 16
    beat both grids.  Here: the best refined value >= the best of a grid 64 x finer per axis, less the layer-A bound of the
    value (C["bound"] 2^-53 (1 + u^2) |a| with u = 0 for the bound), it strictly beats the coarse grid, and it lies inside."""
    X, y, Z, args = RC.bump(d)
    p = _problem(X, y, Z, args)
    lo, hi = np.zeros(d), np.ones(d)
    nc = RC.COARSE[d]
    coarse, fine = RC.grid(d, nc), RC.grid(d, 64 * (nc - 1) + 1)
    try:
        kw = dict(maximise=True, kappa=RC.BOUND_KAPPA, var_floor=1e-10)
        top = p.acquire(coarse, "bound", top_k=16, want=(), **kw)
        starts = np.asfortranarray(coarse[:, top["top_index"]])
        out = p.acquire_refine(starts, "bound", lower=lo, upper=hi, max_evals=40, **kw)
        fine_best = float(np.max(p.acquire(fine, "bound", want=("values",), **kw)["values"]))
        j = int(np.argmax(out["values"]))
        got, coarse_best = float(out["values"][j]), float(top["top_values"][0])
        bound = C["bound"] * EPS * abs(fine_best)
        print("refine.does_its_job.d%d: refined %.12g at %s, fine grid %.12g, coarse %.12g" % (d, got, out["x"][:, j], fine_best, coarse_best))
        assert got >= fine_best - bound and got > coarse_best
        assert np.all(out["x"][:, j] > 0.0) and np.all(out["x"][:, j] < 1.0)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("m,d", [(50, 3), (65, 3)], ids=str)
def test_edges(m, d):
    p, D, best, X = _model(m, d)
    best = best[1]
    lo, hi = np.zeros(D), np.ones(D)
    box = dict(lower=lo, upper=hi, var_floor=1e-10, want=gpr_amd.Problem.REFINE_OUTPUTS)
    Xt = _starts(D, 9, lo, hi, 2)
    try:
        before = p.predict(Xt)
        # a start outside the box is clipped; max_evals = 1 returns it
        S = np.asfortranarray(np.array([[-2.0] * D, [3.0] * D, [0.5] * D]).T)
        one = p.acquire_refine(S, "ei", maximise=True, best=best, **box, **dict(OPTS, max_evals=1))
        assert np.array_equal(one["x"], np.clip(S, 0.0, 1.0)) and np.all(one["evals"] == 1) and np.all(one["accepted"] == 0)
        # (a clipped start in a corner the gradient points out of has a zero direction: CONVERGED comes before MAX_EVALS)
        assert one["status"][2] == RR.MAX_EVALS and np.all((one["status"] == RR.MAX_EVALS) | (one["status"] == RR.CONVERGED))
        direct = p.acquire(np.asfortranarray(np.clip(S, 0.0, 1.0)), "ei", maximise=True, best=best, var_floor=1e-10)
        assert np.allclose(one["values"], direct["values"], rtol=1e-12, atol=0) and np.array_equal(one["trace"][:, 0, :D].T, one["x"])
        # the maximiser on a face and in a corner: the bound with kappa = 0 of a box where the mean rises along every axis ...
        g = p.acquire(np.asfortranarray(np.full((D, 1), 0.5)), "bound", maximise=True, kappa=0.0)["dvalues"][:, 0]
        tiny_lo, tiny_hi = np.full(D, 0.5 - 1e-3), np.full(D, 0.5 + 1e-3)
        corner = p.acquire_refine(np.asfortranarray(np.full((D, 1), 0.5)), "bound", maximise=True, kappa=0.0, lower=tiny_lo,
                                  upper=tiny_hi, var_floor=1e-10, **dict(OPTS, max_evals=40))
        assert np.array_equal(corner["x"][:, 0], np.where(g > 0, tiny_hi, tiny_lo)) and corner["status"][0] == RR.CONVERGED
        face_hi = tiny_hi.copy()
        face_hi[0] = 0.5 + 0.45 if g[0] > 0 else face_hi[0]
        face_lo = tiny_lo.copy()
        face_lo[0] = 0.5 - 0.45 if g[0] <= 0 else face_lo[0]
        face = p.acquire_refine(np.asfortranarray(np.full((D, 1), 0.5)), "bound", maximise=True, kappa=0.0, lower=face_lo,
                                upper=face_hi, var_floor=1e-10, **dict(OPTS, max_evals=40))
        assert np.array_equal(face["x"][1:, 0], np.where(g > 0, tiny_hi, tiny_lo)[1:])
        # ... and along the long axis the start ends on the bound or, inside, where the gradient has all but vanished
        x0, g0 = face["x"][0, 0], face["dvalues"][0, 0]
        assert x0 in (face_lo[0], face_hi[0]) or (face_lo[0] < x0 < face_hi[0] and abs(g0) <= 1e-4 * abs(g[0])), (x0, g0, g[0])
        # a clamped variance (var_floor = 10 sf2): the gradient is c_mu dmu alone, the rule still holds
        Xc = Xt.copy()
        Xc[:, 0] = X[:, 0]  # (a start on a training point)
        cl = p.acquire_refine(Xc, "ei", maximise=True, best=best, lower=lo, upper=hi, var_floor=10.0,
                              want=gpr_amd.Problem.REFINE_OUTPUTS, **OPTS)
        kwc = dict(maximise=True, best=best, xi=0.0, kappa=0.0, var_floor=10.0, predictive=False)
        _check(p, "refine.clamped.m%d" % m, cl, "ei", kwc, lo, hi, None, OPTS)
        # EI 40 standard deviations into the tail: a zero gradient, no step; log EI from the same start moves
        mu, var = p.predict(Xt, predictive=False)
        far = float(np.max(mu)) + 45.0 * float(np.sqrt(np.max(var)))
        ei = p.acquire_refine(Xt, "ei", maximise=True, best=far, **box, **OPTS)
        assert np.all(ei["status"] == RR.CONVERGED) and np.all(ei["evals"] == 1) and np.all(ei["dvalues"] == 0.0)
        lei = p.acquire_refine(Xt, "log_ei", maximise=True, best=far, **box, **OPTS)
        assert np.all(lei["accepted"] >= 1) and np.all(lei["values"] > lei["trace"][:, 0, 2 * D])
        # a refused call leaves a following acquire bit-identical; the predictor state is unchanged
        ref = p.acquire(Xt, "ei", maximise=True, best=best, var_floor=1e-10, want=ALL)
        bad = [dict(step0=0.0), dict(max_evals=0), dict(shrink=1.0), dict(grow=0.5), dict(c1=1.0), dict(xtol=-1.0)]
        for b in bad:
            with pytest.raises(gpr_amd.GprHipError) as e:
                p.acquire_refine(Xt, "ei", maximise=True, best=best, **box, **dict(OPTS, **b))
            assert e.value.status == _lib.EBADARG
        for kwb in (dict(lower=hi, upper=lo), dict(lower=lo, upper=np.full(D, np.inf)), dict(scale=np.zeros(D)),
                    dict(scale=np.full(D, np.nan))):
            with pytest.raises(gpr_amd.GprHipError) as e:
                p.acquire_refine(Xt, "ei", maximise=True, best=best, **dict(dict(lower=lo, upper=hi, var_floor=1e-10), **kwb), **OPTS)
            assert e.value.status == _lib.EBADARG
        nan_start = Xt.copy()
        nan_start[0, 3] = np.nan
        with pytest.raises(gpr_amd.GprHipError) as e:
            p.acquire_refine(nan_start, "ei", maximise=True, best=best, **box, **OPTS)
        assert e.value.status == _lib.EBADARG
        after = p.acquire(Xt, "ei", maximise=True, best=best, var_floor=1e-10, want=ALL)
        assert all(np.array_equal(ref[k], after[k]) for k in ALL)
        now = p.predict(Xt)
        assert np.array_equal(before[0], now[0]) and np.array_equal(before[1], now[1])
        empty = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N, D, D, m)
        try:
            with pytest.raises(gpr_amd.GprHipError) as e:
                empty.acquire_refine(Xt, "ei", maximise=True, best=best, **box, **OPTS)
            assert e.value.status == _lib.ESTATE
        finally:
            empty.close()
    finally:
        p.close()
