"""gprhip_sample_paths_refine on the device, checked from its trace alone (no replay):

1. every record's (a_y, g_y) is s f_j and s grad f_j at the traced y against the 80-bit reference of tests/sample_paths_ref.py,
   grouped by draw: values within TOL_POST of the draw's largest absolute value, gradients within TOL_GRAD of its largest
   gradient entry -- the project's constants with no conditioning allowance (cond <= COND_MAX asserted);
2. every record obeys the rule of gpr_amd/csrc/refine_step.h given the previous state (the check of tests/test_gpu_refine.py:
   alpha exact, y within 2 ulp and inside the box, the flag the Armijo inequality outside the tie band, at most 2 % of the
   records inside it), accepted values never decrease, x / values / dvalues are the last accepted record bit for bit, evals /
   accepted / status follow from the trace, CONVERGED means the stated condition;
3. z = 0 is the mean; 4. independence and determinism; 5. the refined winners of a coarse grid beat a 64 x finer grid, per
   draw; 6. the edges.

Route 1 is the persistent kernel (no projection, any m), route 2 the library-side loop (with a projection)."""
import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import margins as M
from tests import path_refine_cases as PC
from tests import refine_cases as RC
from tests import refine_ref as RR
from tests.test_gpu_parity import TOL_GRAD, TOL_POST
from tests.test_gpu_predict_grad import COND_MAX
from tests.test_gpu_refine import OPTS, _ulps

gpu = pytest.mark.gpu
EPS = 2.0 ** -53
NAMES = gpr_amd.Problem.REFINE_OUTPUTS


def _problem(key):
    Xs, y, Zs, args, ok, cond = PC.model(key)
    assert cond <= COND_MAX, (key, cond)
    D, d, m = Xs.shape[0], Zs.shape[0], Zs.shape[1]
    p = gpr_amd.Problem(gpr_amd.COV_SE_FAT if key[0] != "iso" else gpr_amd.COV_SE_ISO, PC.N, D, d, m)
    p.set_inputs(Xs)
    p.set_targets(y)
    p.eval(want_grad=False, sigma2=PC.SIGMA2, inducing=Zs, **args)
    return p


def _records(out, D):
    """(points D x nrec, flat records, start of each record)"""
    ns = out["x"].shape[1]
    flat = np.concatenate([out["trace"][i, :out["evals"][i]] for i in range(ns)])
    who = np.concatenate([np.full(out["evals"][i], i) for i in range(ns)])
    return np.asfortranarray(flat[:, :D].T), flat, who


def _check_objective(p, key, what, out, z, dr, s):
    """check 1; returns nothing"""
    D = out["x"].shape[0]
    pts, flat, who = _records(out, D)
    cond = PC.model(key)[5]
    M.note(cond=cond, kind=key[0], n=PC.N, m=p.m, d=p.d, D=D, nt=pts.shape[1])
    direct = p.sample_paths(pts, z)["samples"]
    same = True
    for j in sorted(set(int(v) for v in dr)):
        sel = np.nonzero(dr[who] == j)[0]
        f, g = PC.paths_at(key, pts[:, sel], z[:, j])
        ev = float(np.max(np.abs(s * flat[sel, 2 * D] - f)) / max(np.max(np.abs(f)), 1e-300))
        eg = float(np.max(np.abs(s * flat[sel, D:2 * D].T - g)) / max(np.max(np.abs(g)), 1e-300))
        print("%s.draw%d: values %.3e of the largest (bound %.0e), gradients %.3e (bound %.0e)" % (what, j, ev, TOL_POST, eg, TOL_GRAD))
        M.record("%s.values" % what, ev, TOL_POST, draw=j)
        M.record("%s.dvalues" % what, eg, TOL_GRAD, draw=j)
        assert ev <= TOL_POST and eg <= TOL_GRAD, (what, j, ev, eg)
        same = same and np.array_equal(s * flat[sel, 2 * D], direct[sel, j])
    print("%s: values equal Problem.sample_paths at the traced points bit for bit: %s" % (what, same))
    M.record("%s.bitwise_sample_paths" % what, 0.0 if same else 1.0, 1.0)


def _check_rule(what, out, lo, hi, scale, opts):
    """check 2; returns (records, skipped)"""
    D, ns = out["x"].shape
    tr = out["trace"]
    sc = np.ones(D) if scale is None else scale
    w = hi - lo
    records = skipped = 0
    for i in range(ns):
        ev, acc, st = int(out["evals"][i]), int(out["accepted"][i]), int(out["status"][i])
        assert 1 <= ev <= opts["max_evals"] and np.all(np.isnan(tr[i, ev:])), (what, i)
        assert np.all(tr[i, :ev, :D] >= lo) and np.all(tr[i, :ev, :D] <= hi), (what, i)
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
            if abs(lhs - rhs) < PC.tie_band(a, ay, opts["c1"], g, delta):
                skipped += 1
            else:
                assert (flag == 1.0) == (lhs >= rhs), (what, i, j, lhs, rhs, flag)
            if flag == 1.0:
                assert ay >= a, (what, i, j)
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


def _run_shape(key, nd, ns, form, route):
    p = _problem(key)
    lo, hi = PC.box(key)
    D = len(lo)
    z = PC.draws(p.m, nd)
    dr = PC.draw_of(ns, nd, form)
    total = skipped = 0
    try:
        p.set_timing(2)
        for ci, (maximise, scaled) in enumerate([(True, False), (False, True), (True, True), (False, False)]):
            scale = np.linspace(0.5, 1.5, D) if scaled else None
            S = PC.starts(key, ns, 7 * ns + ci)
            kw = dict(lower=lo, upper=hi, maximise=maximise, scale=scale, **OPTS)
            out = p.sample_paths_refine(S, z, dr, want=NAMES, **kw)
            stages = p.last_timings()
            assert ("prf_kernel" in stages) == (route == 1), stages
            assert ("prf_eval" in stages and "rf_step" in stages) == (route == 2), stages
            assert "sp_coeff" in stages and "pg_m" not in stages, stages
            what = "path_refine.r%d.m%d_d%d_nd%d_ns%d%s.%s%s" % (route, p.m, p.d, nd, ns, form, "max" if maximise else "min",
                                                                 ".scale" if scaled else "")
            _check_objective(p, key, what, out, z, dr, 1.0 if maximise else -1.0)
            r, s = _check_rule(what, out, lo, hi, scale, OPTS)
            total += r
            skipped += s
            # two runs give the same bits; without the trace all other outputs have the same bits
            again = p.sample_paths_refine(S, z, dr, **kw)
            assert all(np.array_equal(again[k], out[k]) for k in again), what
        print("path_refine.r%d.m%d_d%d_nd%d_ns%d%s: %d records, %d skipped as ties" % (route, p.m, p.d, nd, ns, form, total, skipped))
        assert skipped <= 0.02 * max(total, 1), (total, skipped)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("m,d,nd,ns,form", PC.ROUTE_1, ids=str)
def test_route_1_trace_obeys_the_rule_and_the_draw(m, d, nd, ns, form):
    _run_shape(PC.key_of(m, d), nd, ns, form, 1)


@gpu
@pytest.mark.parametrize("m,d,D,nd,ns,form", PC.ROUTE_2, ids=str)
def test_route_2_trace_obeys_the_rule_and_the_draw(m, d, D, nd, ns, form):
    _run_shape(PC.key_of(m, d, D), nd, ns, form, 2)


@gpu
@pytest.mark.parametrize("m,d,D", [(50, 3, None), (20, 2, 5)], ids=str)
def test_zero_draws_climb_the_mean(m, d, D):
    """z = 0: a_j = t exactly, so every record is the bound with kappa = 0 of Problem.acquire at the traced points, within
    2 TOL_POST / 2 TOL_GRAD of the largest entry (both sides carry their own error against the same truth)"""
    key = PC.key_of(m, d, D)
    p = _problem(key)
    lo, hi = PC.box(key)
    Dd = len(lo)
    try:
        for maximise in (True, False):
            out = p.sample_paths_refine(PC.starts(key, 17, 3), np.zeros((p.m, 3)), PC.draw_of(17, 3, "i"), lower=lo, upper=hi,
                                        maximise=maximise, want=NAMES, **OPTS)
            pts, flat, _ = _records(out, Dd)
            ref = p.acquire(pts, "bound", kappa=0.0, maximise=maximise, var_floor=1e-10)
            M.note(kind=key[0], n=PC.N, m=m, d=d, D=Dd, nt=pts.shape[1])
            M.check_vec("path_refine.zero_z.values", flat[:, 2 * Dd], ref["values"], 2 * TOL_POST)
            M.check_vec("path_refine.zero_z.dvalues", flat[:, Dd:2 * Dd].T, ref["dvalues"], 2 * TOL_GRAD)
    finally:
        p.close()


def _col(out, i):
    return {k: (out[k][:, i] if k in ("x", "dvalues") else out[k][i]) for k in NAMES}


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=(k == "trace")) for k in NAMES)


@gpu
@pytest.mark.parametrize("m,d,D", [(65, 3, None), (20, 2, 5)], ids=str)
def test_independence_permutation_lanes_and_device_buffers(m, d, D):
    import torch
    key = PC.key_of(m, d, D)
    p = _problem(key)
    lo, hi = PC.box(key)
    Dd, nd = len(lo), 17
    z = PC.draws(m, nd)
    kw = dict(lower=lo, upper=hi, maximise=True, want=NAMES, **OPTS)
    try:
        S, dr = PC.starts(key, 130, 5), PC.draw_of(130, nd, "i")
        full = p.sample_paths_refine(S, z, dr, **kw)
        perm = np.random.default_rng(1).permutation(130)
        shuffled = p.sample_paths_refine(np.asfortranarray(S[:, perm]), z, dr[perm], **kw)
        for j, i in enumerate(perm):
            assert _same(_col(shuffled, j), _col(full, i)), (i, j)
        for i in (0, 63, 129):   # alone, and as lane 0 / lane 63 of a full workgroup of other starts
            alone = p.sample_paths_refine(np.asfortranarray(S[:, [i]]), z, dr[[i]], **kw)
            assert _same(_col(alone, 0), _col(full, i)), i
            others = [j for j in range(64) if j != i][:63]
            for pos in (0, 63):
                cols = others[:pos] + [i] + others[pos:]
                wg = p.sample_paths_refine(np.asfortranarray(S[:, cols]), z, dr[cols], **kw)
                assert _same(_col(wg, pos), _col(full, i)), (i, pos)
        # The other draws present: the weights of a draw come from gprhip_sample_paths' weight kernel, which splits its sums
        # over the lanes by the number of draws -- a draw's bits are those of equal nd.  At equal nd the result
        # of a start does not depend on the other columns of z, nor on where its own column stands.
        z2 = PC.draws(m, nd, seed=1)
        z2[:, 5] = z[:, 3]
        for i in np.nonzero(dr == 3)[0][:3]:
            moved = p.sample_paths_refine(np.asfortranarray(S[:, [i]]), z2, np.array([5], dtype=np.int32), **kw)
            assert _same(_col(moved, 0), _col(full, i)), i
        # device buffers
        dev = torch.device("cuda:0")
        st = torch.tensor(np.ascontiguousarray(S.T), device=dev)
        shapes = dict(x=(130, Dd), dvalues=(130, Dd), values=(130,), evals=(130,), accepted=(130,), status=(130,),
                      trace=(130, OPTS["max_evals"], 2 * Dd + 3))
        outs = {k: (torch.full(shapes[k], -1, dtype=torch.int32, device=dev) if k in ("evals", "accepted", "status")
                    else torch.full(shapes[k], float("nan"), dtype=torch.float64, device=dev)) for k in NAMES}
        torch.cuda.synchronize()
        assert p.sample_paths_refine(st.data_ptr(), z, dr, out_device_ptrs={k: v.data_ptr() for k, v in outs.items()}, ns=130, **kw) == {}
        for k in NAMES:
            g = outs[k].cpu().numpy()
            assert np.array_equal(g.T if k in ("x", "dvalues") else g, full[k], equal_nan=(k == "trace")), k
    finally:
        p.close()


BUMP_DRAWS = 4
BUMP_SEED = 0


def _bump_problem(d):
    X, y, Z, args = RC.bump(d)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, RC.N, d, d, RC.BUMP_M)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(want_grad=False, sigma2=RC.SIGMA2, inducing=Z, **args)
    return p


@gpu
@pytest.mark.parametrize("d", [1, 2])
def test_refined_winners_of_a_coarse_grid_beat_a_64_times_finer_grid_per_draw(d):
    """The bump model of tests/refine_cases.py, 4 draws: the starts of draw j are its 16 best points of the coarse grid
    (Problem.sample_paths, top_k = 16).  After refining, each draw's best value >= the best of that draw on the 64 x finer grid
    less TOL_POST max |f_j|, strictly above the coarse grid's best, and inside the box (tests/test_path_refine_host.py shows
    the same on the CPU)."""
    p = _bump_problem(d)
    lo, hi = np.zeros(d), np.ones(d)
    nc = RC.COARSE[d]
    coarse, fine = RC.grid(d, nc), RC.grid(d, 64 * (nc - 1) + 1)
    z = PC.draws(RC.BUMP_M, BUMP_DRAWS, BUMP_SEED)
    try:
        top = p.sample_paths(coarse, z, top_k=16, want_samples=False)
        starts = np.asfortranarray(np.concatenate([coarse[:, top["top_index"][:, j]] for j in range(BUMP_DRAWS)], axis=1))
        dr = np.repeat(np.arange(BUMP_DRAWS), 16).astype(np.int32)
        out = p.sample_paths_refine(starts, z, dr, lower=lo, upper=hi, max_evals=40)
        F = p.sample_paths(fine, z)["samples"]
        for j in range(BUMP_DRAWS):
            sel = np.nonzero(dr == j)[0]
            b = sel[int(np.argmax(out["values"][sel]))]
            got, fine_best, coarse_best = float(out["values"][b]), float(np.max(F[:, j])), float(top["top_values"][0, j])
            print("path_refine.does_its_job.d%d.draw%d: refined %.12g at %s, fine grid %.12g, coarse %.12g"
                  % (d, j, got, out["x"][:, b], fine_best, coarse_best))
            assert got >= fine_best - TOL_POST * float(np.max(np.abs(F[:, j]))) and got > coarse_best, (d, j)
            assert np.all(out["x"][:, b] > 0.0) and np.all(out["x"][:, b] < 1.0), (d, j)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("m,d,D", [(65, 3, None), (20, 2, 5)], ids=str)
def test_edges(m, d, D):
    key = PC.key_of(m, d, D)
    p = _problem(key)
    lo, hi = PC.box(key)
    Dd, nd = len(lo), 4
    z = PC.draws(m, nd)
    box = dict(lower=lo, upper=hi, want=NAMES)
    Xt = PC.starts(key, 9, 2)
    dr9 = PC.draw_of(9, nd, "i")
    try:
        before = p.predict(Xt)
        paths0 = p.sample_paths(Xt, z)["samples"]
        acq0 = p.acquire(Xt, "bound", kappa=1.0, maximise=True, var_floor=1e-10)
        # a start outside the box is clipped; max_evals = 1 returns it; ns = 1
        S = np.asfortranarray(np.array([lo - 2.0, hi + 3.0, 0.5 * (lo + hi)]).T)
        one = p.sample_paths_refine(S, z, np.array([0, 1, 2], dtype=np.int32), **box, **dict(OPTS, max_evals=1))
        assert np.array_equal(one["x"], np.clip(S, lo[:, None], hi[:, None])) and np.all(one["evals"] == 1) and np.all(one["accepted"] == 0)
        assert np.all((one["status"] == RR.MAX_EVALS) | (one["status"] == RR.CONVERGED))
        assert np.array_equal(one["trace"][:, 0, :Dd].T, one["x"])
        single = p.sample_paths_refine(np.asfortranarray(S[:, [2]]), z, np.array([2], dtype=np.int32), **box, **OPTS)
        assert single["evals"][0] >= 1 and single["values"][0] >= single["trace"][0, 0, 2 * Dd]
        # a zero gradient component on an active bound: from the corner the gradient points out of, nothing moves
        mid = np.asfortranarray((0.5 * (lo + hi)).reshape(-1, 1))
        g = p.sample_paths_refine(mid, z, np.array([1], dtype=np.int32), **box, **dict(OPTS, max_evals=1))["dvalues"][:, 0]
        tiny_lo, tiny_hi = mid[:, 0] - 1e-3 * (hi - lo), mid[:, 0] + 1e-3 * (hi - lo)
        corner = p.sample_paths_refine(mid, z, np.array([1], dtype=np.int32), lower=tiny_lo, upper=tiny_hi, want=NAMES,
                                       **dict(OPTS, max_evals=40))
        assert np.array_equal(corner["x"][:, 0], np.where(g > 0, tiny_hi, tiny_lo)) and corner["status"][0] == RR.CONVERGED
        # a NaN column of z: its starts end with ST_NAN, the others keep their bits
        ref = p.sample_paths_refine(Xt, z, dr9, **box, **OPTS)
        zn = z.copy()
        zn[:, 2] = np.nan
        bad = p.sample_paths_refine(Xt, zn, dr9, **box, **OPTS)
        for i in range(9):
            if dr9[i] == 2:
                assert bad["status"][i] == _lib.REFINE_ST_NAN and bad["evals"][i] == 1, i
            else:
                assert _same(_col(bad, i), _col(ref, i)), i
        # refusals leave the predictor as it was
        for b in (dict(step0=0.0), dict(max_evals=0), dict(shrink=1.0), dict(grow=0.5), dict(c1=1.0), dict(xtol=-1.0)):
            with pytest.raises(gpr_amd.GprHipError) as e:
                p.sample_paths_refine(Xt, z, dr9, **box, **dict(OPTS, **b))
            assert e.value.status == _lib.EBADARG
        for kwb in (dict(lower=hi, upper=lo), dict(upper=np.full(Dd, np.inf)), dict(scale=np.zeros(Dd)), dict(scale=np.full(Dd, np.nan))):
            with pytest.raises(gpr_amd.GprHipError) as e:
                p.sample_paths_refine(Xt, z, dr9, **dict(dict(lower=lo, upper=hi), **kwb), **OPTS)
            assert e.value.status == _lib.EBADARG
        nan_start = Xt.copy()
        nan_start[0, 3] = np.nan
        for args in ((nan_start, z, dr9), (Xt, z, np.full(9, nd, dtype=np.int32)), (Xt, z, np.full(9, -1, dtype=np.int32)),
                     (Xt, np.zeros((m, 65)), dr9)):
            with pytest.raises(gpr_amd.GprHipError) as e:
                p.sample_paths_refine(*args, **box, **OPTS)
            assert e.value.status == _lib.EBADARG
        now = p.predict(Xt)
        assert np.array_equal(before[0], now[0]) and np.array_equal(before[1], now[1])
        assert np.array_equal(paths0, p.sample_paths(Xt, z)["samples"])
        acq1 = p.acquire(Xt, "bound", kappa=1.0, maximise=True, var_floor=1e-10)
        assert all(np.array_equal(acq0[k], acq1[k]) for k in acq0)
        empty = gpr_amd.Problem(gpr_amd.COV_SE_FAT if D else gpr_amd.COV_SE_ISO, PC.N, Dd, d, m)
        try:
            with pytest.raises(gpr_amd.GprHipError) as e:
                empty.sample_paths_refine(Xt, z, dr9, **box, **OPTS)
            assert e.value.status == _lib.ESTATE
        finally:
            empty.close()
    finally:
        p.close()
