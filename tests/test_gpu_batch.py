"""gprhip_batch_*: several hyper-parameter sets against one resident data set in one chain of launches.

The contract is bit identity: lane j of a batch evaluation equals a plain `Problem.eval` with the same hyper-parameters on a
plain problem of the same shape and data, compared with numpy.array_equal on the raw float64 -- for any count, any lane
position, and with a refused lane beside it.  Every sweep case is also held against the CPU oracle at the bounds the parity
suite uses for these shapes (imported from tests/test_gpu_parity.py, not restated)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from oracle import fitc_oracle as O
from tests import margins as M
from tests.test_gpu_factors import HYP_MINOR, N_MINOR, _minor_data, minor_reference
from tests.test_gpu_parity import TOL_COEFF, TOL_DS2, TOL_GRAD, TOL_L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- data, hyper-parameter sets, single evaluations ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(n, D, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + D)
    X = np.asfortranarray(rng.normal(size=(D, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    return X, y


def _hypers(kind, n, D, d, m, count, proj=False, het=False, ms=False, variational=False, model_only=False, seed=0):
    """`count` distinct keyword sets of Problem.eval: every per-lane quantity differs from lane to lane."""
    rng = np.random.default_rng(77 + 13 * seed + n + 3 * m + 5 * d)
    X, _ = _data(n, D)
    out = []
    for j in range(count):
        # (the jitter stays the reference's default, which the oracle uses: the lane-isolation test varies it)
        kw = dict(log_sf2=0.05 * (j % 9) - 0.1, sigma2=0.1 + 0.01 * j, variational=variational, model_only=model_only)
        pts = X
        if kind == gpr_amd.COV_SE_ISO:
            kw["log_ell"] = 0.5 * np.log(d) + 0.03 * (j % 11)
        if proj:
            kw["tproj"] = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D))
            pts = kw["tproj"].T @ X
        kw["inducing"] = np.asfortranarray(pts[:, rng.integers(0, n, size=m)] + 0.3 * rng.normal(size=(d, m)))
        if het:
            kw["log_hetero_skedasticity"] = -3.0 + 0.2 * rng.normal(size=m)
        if ms:
            kw["log_multiscales_m05"] = np.asfortranarray(0.2 * rng.normal(size=(d, m)))
        out.append(kw)
    return out


def _problem(kind, n, D, d, m, chunk_rows=0, targets=True):
    X, y = _data(n, D)
    p = gpr_amd.Problem(kind, n, D, d, m, chunk_rows=chunk_rows)
    p.set_inputs(X)
    if targets:
        p.set_targets(y)
    return p


def _singles(kind, n, D, d, m, hyps, want_grad=True, chunk_rows=0, y=None):
    """Plain evaluations, one after the other on one plain problem."""
    q = _problem(kind, n, D, d, m, chunk_rows)
    if y is not None:
        q.set_targets(y)
    try:
        return [q.eval(want_grad=want_grad, **kw) for kw in hyps]
    finally:
        q.close()


def _same(a, b):
    """Bit identity of two evaluations: scalars, gradient, coefficients."""
    bits = lambda x: np.float64(x).tobytes()
    if not (bits(a.l1) == bits(b.l1) and bits(a.l2) == bits(b.l2) and bits(a.l) == bits(b.l)):
        return False
    if (a.grad is None) != (b.grad is None):
        return False
    if a.grad is not None and not (bits(a.dl_dsigma2) == bits(b.dl_dsigma2) and np.array_equal(a.grad, b.grad)):
        return False
    return np.array_equal(a.coeffs, b.coeffs)


def _assert_lanes_equal_singles(evs, sts, singles, what=""):
    assert sts == [_lib.OK] * len(singles), (what, sts)
    bad = [j for j, (a, b) in enumerate(zip(evs, singles)) if not _same(a, b)]
    assert not bad, "%s: lanes %s differ from their single evaluations" % (what, bad)


# ---- 1. the premise ------------------------------------------------------------------------------------------------------
def test_two_plain_evaluations_agree_bit_for_bit():
    kind, n, D, d, m = gpr_amd.COV_SE_ISO, 2000, 3, 3, 50
    hyps = _hypers(kind, n, D, d, m, 1)
    a = _singles(kind, n, D, d, m, hyps)[0]
    b = _singles(kind, n, D, d, m, hyps)[0]
    assert _same(a, b)


# ---- 2. bit identity with single evaluations, one sweep per axis --------------------------------------------------------
ISO, FAT = gpr_amd.COV_SE_ISO, gpr_amd.COV_SE_FAT
DEF = dict(kind=ISO, n=200, D=3, d=3, m=10, count=2)


def _case(**kw):
    c = dict(DEF)
    c.update(kw)
    if c["kind"] == ISO:
        c["D"] = c["d"]
    return c


SWEEP = (
    [_case(count=c) for c in (1, 2, 7, 64)]
    + [_case(m=m) for m in (1, 50, 64)]
    + [_case(n=n, count=3) for n in (1, 63, 64, 65, 2000)]
    + [_case(d=d) for d in (1, 8, 9, 16)]
    + [_case(kind=FAT), _case(kind=FAT, D=5, d=3, proj=True), _case(kind=FAT, D=40, d=4, proj=True),
       _case(kind=FAT, het=True), _case(kind=FAT, ms=True), _case(kind=FAT, D=8, d=8, ms=True),
       _case(kind=FAT, D=5, d=3, proj=True, het=True, ms=True), _case(kind=FAT, D=16, d=16), _case(kind=FAT, D=9, d=9, het=True)]
    + [_case(variational=True), _case(model_only=True), _case(want_grad=False), _case(variational=True, want_grad=False),
       _case(kind=FAT, D=5, d=3, proj=True, variational=True), _case(n=2000, m=50, count=8),
       _case(kind=FAT, D=5, d=3, proj=True, model_only=True), _case(kind=FAT, ms=True, want_grad=False)]
)


def _case_id(c):
    return "_".join("%s%s" % (k, v) for k, v in c.items() if DEF.get(k) != v or k in ("n", "m", "d", "count"))


def _oracle_kernel(kind, d, kw):
    if kind == ISO:
        return O.SeIsoKernel(kw["log_ell"], kw["log_sf2"])
    return O.SeFatKernel(d, kw["log_sf2"], kw.get("tproj"), kw.get("log_hetero_skedasticity"), kw.get("log_multiscales_m05"))


@pytest.mark.parametrize("c", SWEEP, ids=_case_id)
def test_lanes_equal_single_evaluations(c):
    kind, n, D, d, m, count = c["kind"], c["n"], c["D"], c["d"], c["m"], c["count"]
    flags = {k: c.get(k, False) for k in ("proj", "het", "ms", "variational", "model_only")}
    want_grad = c.get("want_grad", True)
    hyps = _hypers(kind, n, D, d, m, count, **flags)
    singles = _singles(kind, n, D, d, m, hyps, want_grad)
    p = _problem(kind, n, D, d, m)
    b = p.batch(count)
    try:
        evs, sts = b.eval(hyps, want_grad)
        _assert_lanes_equal_singles(evs, sts, singles, _case_id(c))
        # ... and against the oracle, at the parity suite's bounds for these shapes
        X, y = _data(n, D)
        fams = M.families("iso" if kind == ISO else "fat", d, m, D, flags["proj"], flags["het"], flags["ms"])
        for j in sorted({0, count - 1}):
            kw = hyps[j]
            ref = O.evaluate_fast(_oracle_kernel(kind, d, kw), kw["inducing"], X, y, kw["sigma2"], flags["variational"])
            cond = b.lane(j).condition()[0]
            M.check_rel("l1", evs[j].l1, ref["l1"], TOL_L)
            if flags["model_only"]:
                continue
            M.check_rel("l", evs[j].l, ref["l"], TOL_L)
            M.check_vec("coeffs", evs[j].coeffs, ref["coeffs"], TOL_COEFF, cond=cond)
            if want_grad:
                M.check_rel("dl_dsigma2", evs[j].dl_dsigma2, ref["dl_dsigma2"], TOL_DS2, floor=1.0)
                M.check_grad(evs[j].grad, ref["grad"], fams, TOL_GRAD, cond=cond)
    finally:
        b.close()
        p.close()


# ---- 3. several blocks per workgroup, several chunks ------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk_rows", [(16449, 0), (32833, 0), (2000, 512)], ids=["n16449", "n32833", "n2000_chunk512"])
def test_several_blocks_per_workgroup(n, chunk_rows):
    kind, D, d, m, count = ISO, 3, 3, 64, 3
    hyps = _hypers(kind, n, D, d, m, count)
    singles = _singles(kind, n, D, d, m, hyps, chunk_rows=chunk_rows)
    p = _problem(kind, n, D, d, m, chunk_rows)
    b = p.batch(count)
    try:
        _assert_lanes_equal_singles(*b.eval(hyps), singles)
    finally:
        b.close()
        p.close()


# ---- 4. lane position and count do not matter ----------------------------------------------------------------------------------
def test_lane_position_and_count_do_not_matter():
    kind, n, D, d, m = ISO, 200, 3, 3, 10
    hyps = _hypers(kind, n, D, d, m, 64)
    the = hyps[0]
    Xt = np.asfortranarray(np.random.default_rng(5).normal(size=(D, 33)))
    p = _problem(kind, n, D, d, m)
    b = p.batch(64)
    try:
        alone = b.eval([the])[0][0]
        fifth = b.eval(hyps[1:6] + [the] + hyps[6:7])[0][5]
        evs64, sts = b.eval(hyps[1:64] + [the])
        assert sts == [_lib.OK] * 64
        assert _same(alone, fifth) and _same(alone, evs64[63])
        assert _same(alone, _singles(kind, n, D, d, m, [the])[0])
        # a shorter evaluation leaves the other lanes' state alone
        before = b.lane(10).predict(Xt)
        evs3, _ = b.eval(hyps[20:23])
        after = b.lane(10).predict(Xt)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert _same(evs3[0], _singles(kind, n, D, d, m, [hyps[20]])[0])
    finally:
        b.close()
        p.close()


# ---- 5. lane isolation ------------------------------------------------------------------------------------------------------
def test_a_refused_lane_does_not_disturb_the_others():
    case = (50, (17,), -1e-3)
    m, orders, jitter = case
    Zbad, info, _ = minor_reference(m, orders, jitter)
    X, Y, Xt, Zg = _minor_data(m)

    def fresh():
        q = gpr_amd.Problem(ISO, N_MINOR, 2, 2, m)
        q.set_inputs(X)
        q.set_targets(Y[:, 0])
        return q

    good = [dict(HYP_MINOR, inducing=Zg, log_sf2=0.1 * j) for j in range(5)]
    hyps = list(good)
    hyps[2] = dict(HYP_MINOR, inducing=Zbad, jitter=jitter)
    q = fresh()
    singles = [q.eval(**kw) for j, kw in enumerate(good)]
    with pytest.raises(gpr_amd.NotPositiveDefinite) as e:
        q.eval(**hyps[2])
    single_msg = str(e.value)
    q.close()
    assert ("leading minor of order %d of K_m" % info) in single_msg
    p = fresh()
    b = p.batch(5)
    try:
        evs, sts = b.eval(hyps)
        assert sts == [_lib.OK, _lib.OK, _lib.ENOTPOSDEF, _lib.OK, _lib.OK]
        assert b.last_error == single_msg
        assert evs[2] is None
        for j in (0, 1, 3, 4):
            assert _same(evs[j], singles[j]), j
        with pytest.raises(gpr_amd.GprHipError) as e1:
            b.lane(2).predict(Xt, want_variances=False)
        assert e1.value.status == _lib.ESTATE
        b.lane(1).predict(Xt)
        _assert_lanes_equal_singles(*b.eval(good), singles)
    finally:
        b.close()
        p.close()


# ---- 6. the parent problem is untouched ---------------------------------------------------------------------------------------
def test_the_parent_problem_is_untouched():
    kind, n, D, d, m = ISO, 300, 3, 3, 20
    hyps = _hypers(kind, n, D, d, m, 4)
    Xt = np.asfortranarray(np.random.default_rng(6).normal(size=(D, 40)))
    re = dict(hyps[0], sigma2=0.3, reuse_v=True)

    def run(with_batch):
        p = _problem(kind, n, D, d, m)
        b = p.batch(3) if with_batch else None
        try:
            first = p.eval(**hyps[0])
            if b:
                b.eval(hyps[1:4])
            pred = p.predict(Xt)
            again = p.eval(**re)
            return first, pred, again
        finally:
            if b:
                b.close()
            p.close()

    f0, p0, a0 = run(False)
    f1, p1, a1 = run(True)
    assert _same(f0, f1) and _same(a0, a1)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])


# ---- 7. lane problems serve predictions ---------------------------------------------------------------------------------------
def test_lane_problems_serve_predictions():
    kind, n, D, d, m = FAT, 300, 5, 3, 20
    hyps = _hypers(kind, n, D, d, m, 3, proj=True)
    Xt = np.asfortranarray(np.random.default_rng(7).normal(size=(D, 70)))
    p = _problem(kind, n, D, d, m)
    b = p.batch(3)
    q = _problem(kind, n, D, d, m)
    try:
        b.eval(hyps)
        for j in (2, 0, 1):
            q.eval(**hyps[j])
            mq, vq = q.predict(Xt)
            ml, vl = b.lane(j).predict(Xt)
            assert np.array_equal(mq, ml) and np.array_equal(vq, vl), j
            uq, rq = q.co_variance_coeffs()
            ul, rl = b.lane(j).co_variance_coeffs()
            assert np.array_equal(uq, ul) and np.array_equal(rq, rl), j
            assert np.array_equal(q.train_stats()[0], b.lane(j).train_stats()[0]), j
    finally:
        q.close()
        b.close()
        p.close()


# ---- 8. targets are borrowed ----------------------------------------------------------------------------------------------------
def test_targets_are_borrowed():
    kind, n, D, d, m = ISO, 300, 3, 3, 20
    hyps = _hypers(kind, n, D, d, m, 3)
    X, y = _data(n, D)
    y2 = np.cos(X[0]) - 0.5 * y
    p = _problem(kind, n, D, d, m)
    b = p.batch(3)
    try:
        _assert_lanes_equal_singles(*b.eval(hyps), _singles(kind, n, D, d, m, hyps))
        p.set_targets(y2)
        evs, sts = b.eval(hyps)
        new = _singles(kind, n, D, d, m, hyps, y=y2)
        _assert_lanes_equal_singles(evs, sts, new)
        assert all(a.l2 != c.l2 for a, c in zip(new, _singles(kind, n, D, d, m, hyps)))
    finally:
        b.close()
        p.close()


# ---- 9. refusals evaluate nothing -----------------------------------------------------------------------------------------------
def _refused(call, status):
    with pytest.raises(gpr_amd.GprHipError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))


@pytest.mark.parametrize("shape", [dict(kind=ISO, D=3, d=3, m=65), dict(kind=ISO, D=17, d=17, m=10),
                                   dict(kind=ISO, D=3, d=3, m=10, precision=gpr_amd.F32_BULK)], ids=["m65", "d17", "f32"])
def test_create_refuses_what_the_small_path_never_takes(shape):
    p = gpr_amd.Problem(shape["kind"], 200, shape["D"], shape["d"], shape["m"], precision=shape.get("precision", gpr_amd.F64))
    try:
        _refused(lambda: p.batch(2), _lib.EBADARG)
    finally:
        p.close()


def test_create_refuses_a_disabled_small_path():
    """GPRHIP_SMALL_PATH is read when a problem is created: a child process with it set to 0."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gpr_amd\nfrom gpr_amd import _lib\n"
            "p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, 200, 3, 3, 10)\n"
            "try:\n    p.batch(2)\n    print('CREATED')\n"
            "except gpr_amd.GprHipError as e:\n    print('STATUS', e.status)\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, GPRHIP_SMALL_PATH="0"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "STATUS %d" % _lib.EBADARG in out.stdout, out.stdout


def test_eval_refusals_enqueue_nothing():
    kind, n, D, d, m = ISO, 200, 3, 3, 10
    hyps = _hypers(kind, n, D, d, m, 3)
    singles = _singles(kind, n, D, d, m, hyps)
    p = _problem(kind, n, D, d, m)
    _refused(lambda: p.batch(65), _lib.EBADARG)
    _refused(lambda: p.batch(0), _lib.EBADARG)
    b = p.batch(3)
    try:
        _assert_lanes_equal_singles(*b.eval(hyps), singles)
        bad = [
            ([], _lib.EBADARG),
            (hyps + hyps[:1], _lib.EBADARG),
            ([hyps[0], dict(hyps[1], reuse_v=True)], _lib.EBADARG),
            ([hyps[0], dict(hyps[1], sigma2=-0.1)], _lib.EBADARG),
            ([hyps[0], dict(hyps[1], variational=True)], _lib.EBADARG),
            ([hyps[0], dict(hyps[1], model_only=True)], _lib.EBADARG),
        ]
        for hs, st in bad:
            _refused(lambda: b.eval(hs), st)
            # the lanes kept their state, and a correct evaluation follows
            assert np.array_equal(b.lane(1).debug_fetch("t"), singles[1].coeffs)
        _assert_lanes_equal_singles(*b.eval(hyps), singles)
    finally:
        b.close()
        p.close()


def test_eval_refuses_mixed_option_arrays_and_wide_multiscales():
    kind, n, D, d, m = FAT, 200, 9, 9, 10
    plain = _hypers(kind, n, D, d, m, 2)
    het = _hypers(kind, n, D, d, m, 2, het=True)
    ms = _hypers(kind, n, D, d, m, 2, ms=True)
    p = _problem(kind, n, D, d, m)
    b = p.batch(2)
    try:
        _refused(lambda: b.eval([plain[0], het[1]]), _lib.EBADARG)
        _refused(lambda: b.eval(ms), _lib.EBADARG)  # multiscales with d = 9
        _assert_lanes_equal_singles(*b.eval(plain), _singles(kind, n, D, d, m, plain))
    finally:
        b.close()
        p.close()


def test_missing_targets_are_a_state_error():
    kind, n, D, d, m = ISO, 200, 3, 3, 10
    hyps = _hypers(kind, n, D, d, m, 2)
    p = _problem(kind, n, D, d, m, targets=False)
    b = p.batch(2)
    try:
        _refused(lambda: b.eval(hyps), _lib.ESTATE)
        mo = [dict(kw, model_only=True) for kw in hyps]
        evs, sts = b.eval(mo)
        assert sts == [_lib.OK, _lib.OK]
        p.set_targets(_data(n, D)[1])
        _assert_lanes_equal_singles(*b.eval(hyps), _singles(kind, n, D, d, m, hyps))
    finally:
        b.close()
        p.close()


def test_either_order_of_destruction_is_clean():
    kind, n, D, d, m = ISO, 200, 3, 3, 10
    hyps = _hypers(kind, n, D, d, m, 2)
    p = _problem(kind, n, D, d, m)
    b = p.batch(2)
    b.eval(hyps)
    b.close()
    p.close()
    p = _problem(kind, n, D, d, m)
    b = p.batch(2)
    b.eval(hyps)
    p.close()
    _refused(lambda: b.eval(hyps), _lib.ESTATE)  # a batch without its problem can only be destroyed
    b.close()
    # ... and the device is still in order
    _assert_lanes_equal_singles([_singles(kind, n, D, d, m, hyps)[0]], [_lib.OK], [_singles(kind, n, D, d, m, hyps)[0]])


# ---- 10. repeatability ---------------------------------------------------------------------------------------------------------
def test_a_batch_repeats_bit_for_bit():
    kind, n, D, d, m = ISO, 2000, 3, 3, 50
    hyps = _hypers(kind, n, D, d, m, 8)
    p = _problem(kind, n, D, d, m)
    b = p.batch(8)
    try:
        first, _ = b.eval(hyps)
        second, _ = b.eval(hyps)
        assert all(_same(x, y) for x, y in zip(first, second))
    finally:
        b.close()
        p.close()


def test_batched_stages_are_timed_under_their_own_names():
    kind, n, D, d, m = ISO, 200, 3, 3, 10
    hyps = _hypers(kind, n, D, d, m, 2)
    p = _problem(kind, n, D, d, m)
    p.set_timing(2)
    p.eval(**hyps[0])
    own = p.last_timings()
    b = p.batch(2)
    try:
        b.lane(0).set_timing(2)
        b.eval(hyps)
        names = set(b.lane(0).last_timings())
        assert {"batch_km_chol", "batch_p1", "batch_b_chol", "batch_p2", "batch_finish"} <= names, names
        assert p.last_timings() == own
    finally:
        b.close()
        p.close()
