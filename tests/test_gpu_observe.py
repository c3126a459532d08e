"""gprhip_observe, gprhip_posterior_save and gprhip_posterior_restore on the device, against tests/observe_ref.py.

The entry-wise bound is column-wise, in Higham's form for Householder QR: C (k + 1) (c + 1) u |(R~[:, c]; W[:, c])|_2 with the
b | eta column as column m.  C = 4: at most 10 x the worst ratio seen -- 0.66 by tests/cpp/tp_reflect_check.cpp in double
against long double, 0.45 on the device over the cases below (profiles/observe_margins.txt).  The reference is the 80-bit update
BY DEFINITION (a Cholesky factor of R~^T R~ + W^T W) of the device's own pre-state; R~^-1 and t go through running-error
bounds against 80-bit contractions of the device's own R~' and b'.

Shapes: m = 50 (one block, padded columns), 64 / 65 (the threshold of the row paths), 128 (a full block), 129 (two blocks, the
second almost all identity), 300 (three blocks: a trailing launch that has itself a trailing block), each with k = 1, 3, 64;
the variants (d = 1, 16; Cov_se_fat with a 5 -> 3 projection and heteroskedastic noise; inputs offset by 1e3; a loaded
predictor; a model-only state) with every m at k = 3 and with k = 1, 64 at m = 129.  n = 300 training rows, up to 64 new ones."""
import ctypes as C

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from oracle import fitc_oracle as FO
from tests import margins as M
from tests import observe_ref as O
from tests import posterior_ref as PR
from tests.test_gpu_input_grad import _case
from tests.test_gpu_input_grads import Case, case_id, data, hypers_of
from tests.test_gpu_parity import TOL_L, TOL_POST

gpu = pytest.mark.gpu
SIGMA2 = 0.1
N = 300
C_BOUND = 4.0
MS = (50, 64, 65, 128, 129, 300)
KS = (1, 3, 64)
LD = np.longdouble


def _variants(m):
    return [("d1", Case("iso", N + 64, m, 1)), ("d16", Case("iso", N + 64, m, 16)), ("fat-proj-het", Case("proj", N + 64, m, 3, 5, True)),
            ("offset", Case("iso", N + 64, m, 3, offset=1e3)), ("loaded", Case("iso", N + 64, m, 3)), ("model-only", Case("iso", N + 64, m, 3))]


CASES = [("base", Case("iso", N + 64, m, 3), k) for m in MS for k in KS] + \
    [(v, c, 3) for m in MS for v, c in _variants(m)] + [(v, c, k) for v, c in _variants(129) for k in (1, 64)]


def ident(v):
    return case_id(v) if isinstance(v, Case) else str(v)


def split(c, k):
    """the n training rows, the k new ones, the inducing points, the keyword arguments of Problem.eval"""
    X, y, Z, args = data(c)
    return np.asfortranarray(X[:, :N]), y[:N].copy(), np.asfortranarray(X[:, N:N + k]), y[N:N + k].copy(), Z, args


def problem(c, n=N):
    D = data(c)[0].shape[0]
    return gpr_amd.Problem(gpr_amd.COV_SE_ISO if c.kind == "iso" else gpr_amd.COV_SE_FAT, n, D, c.d, c.m)


def prepared(variant, c, k=3, variational=False):
    """a problem in the state the variant names, and whether that state has targets"""
    X, y, Xn, yn, Z, args = split(c, k)
    p = problem(c)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, model_only=variant == "model-only", variational=variational, **args)
    if variant == "loaded":
        q = problem(c)
        q.load_predictor(sigma2=SIGMA2, inducing=Z, coeffs=ev.coeffs, co_variance_coeffs=p.co_variance_coeffs(), **args)
        p.close()
        p = q
    return p, variant != "model-only", ev


def fetch(p, targets=True):
    out = dict(rtil=p.debug_fetch_matrix("rtil"), rinv=p.debug_fetch_matrix("rinv"), uinv=p.debug_fetch_matrix("uinv"))
    if targets:
        out.update(bvec=p.debug_fetch("bvec"), t=p.debug_fetch("t"))
    return out


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a) and a.keys() == b.keys()


def hold(what, got, ref, bound):
    r, at = PR.ratio(got, ref, bound)
    print("%s: worst error / bound %.3g" % (what, r))
    M.record(what, r, 1.0)
    assert r <= 1.0, (what, r, at)


@gpu
@pytest.mark.parametrize("variant,c,k", CASES, ids=ident)
def test_every_entry_against_the_80_bit_update_of_the_device_pre_state(variant, c, k):
    X, y, Xn, yn, Z, args = split(c, k)
    p, targets, _ = prepared(variant, c, k)
    try:
        pre = fetch(p, targets)
        dl = p.observe(Xn, yn if targets else None, want_dlog_evidence=True)
        post = fetch(p, targets)
        assert p.observed_count == k
    finally:
        p.close()
    rw = O.rows(Xn, Z, pre["uinv"], SIGMA2, yn if targets else None, **hypers_of(c, args))
    b0 = pre["bvec"] if targets else None
    ref = O.update_definition(pre["rtil"], b0, rw["W"], rw["eta"])
    assert all(np.all(np.isfinite(v)) for v in post.values())
    ratios = O.column_ratios(post["rtil"], ref["R"], pre["rtil"], rw["W"], post.get("bvec"), ref.get("b"), b0, rw["eta"])
    print("worst column ratio %.3g at column %d of %d (C = %g)" % (ratios.max(), ratios.argmax(), c.m, C_BOUND))
    M.record("observe.column_ratio", float(ratios.max()), C_BOUND, m=c.m, k=k, variant=variant)
    assert ratios.max() <= C_BOUND
    assert np.all(np.diag(post["rtil"]) > 0) and np.array_equal(post["rtil"], np.triu(post["rtil"]))
    assert np.array_equal(post["uinv"], pre["uinv"])
    # R~'^-1 and t from the device's own R~' and b'
    Xl = O.inv_upper(np.asarray(post["rtil"], LD))
    hold("observe.rinv", post["rinv"], Xl, O.inverse_bound(np.asarray(post["rtil"], LD), Xl))
    assert np.array_equal(post["rinv"], np.triu(post["rinv"]))
    if targets:
        tref = np.triu(np.asarray(post["uinv"], LD)) @ (np.triu(np.asarray(post["rinv"], LD)) @ np.asarray(post["bvec"], LD))
        hold("observe.t", post["t"], tref, O.coeff_bound(post["rinv"], post["uinv"], post["bvec"]))
    # dlog_evidence against the reference: the sums of k + m logarithms and of k squares
    dref = O.dlog_evidence(rw["s"], rw["r"], ref["logdet"], ref.get("rho2"), False)
    scale = float(np.abs(np.log(np.asarray(rw["s"], np.float64))).sum() + k * 1.84 + 2 * abs(float(ref["logdet"])) + float(ref.get("rho2", 0)))
    err = abs(dl - float(dref))
    print("dlog_evidence %.15g, reference %.15g, error %.3g of the terms' sum" % (dl, float(dref), err / scale))
    M.record("observe.dlog_ref", err / scale, 1e-12)
    assert err <= 1e-12 * scale


def oracle_kernel(c):
    return _case(c.kind, c.n, c.m, c.d, c.D, c.het, c.offset)[4]


REFIT = [("base", Case("iso", N + 64, m, 3), k, var) for m in MS for k in (3, 64) for var in (False, True)] + \
    [(v, c, 3, False) for v, c in _variants(129)[:4]]


@gpu
@pytest.mark.parametrize("variant,c,k,variational", REFIT, ids=ident)
def test_eval_plus_observe_equals_the_refit_end_to_end(variant, c, k, variational):
    """Means and variances after eval on n rows + observe on k rows against the 80-bit posterior of the n + k problem (3e-10 of
    the largest entry, the bound of tests/test_gpu_predict_grad.py for values), k points at once and one call at a time; and
    dlog_evidence against the oracle's evidence difference at the evidence parity bound times |l(n + k)|."""
    X, y, Xn, yn, Z, args = split(c, k)
    Xall, yall = np.asfortranarray(np.hstack([X, Xn])), np.concatenate([y, yn])
    Xt = np.asfortranarray(data(c)[0][:, N + 64 - 40:N + 64] * 0.9)
    ref = O.posterior_from_scratch(Xall, yall, Z, Xt, SIGMA2, log_het=args.get("log_hetero_skedasticity"), **hypers_of(c, args))
    ok = oracle_kernel(c)
    l0 = FO.evaluate_fast(ok, Z, X, y, SIGMA2, variational=variational)["l"]
    l1 = FO.evaluate_fast(ok, Z, Xall, yall, SIGMA2, variational=variational)["l"]
    for mode in ("at once", "one at a time"):
        p, _, _ = prepared(variant, c, k, variational)
        try:
            if mode == "at once":
                dl = p.observe(Xn, yn, want_dlog_evidence=True)
            else:
                dl = sum(p.observe(Xn[:, i:i + 1], yn[i:i + 1], want_dlog_evidence=True) for i in range(k))
            mean, var = p.predict(Xt, predictive=False)
        finally:
            p.close()
        print(mode, "means %.3e variances %.3e of the largest entry; dl %.12g, oracle difference %.12g" % (
            M.relinf(mean, ref["means"].astype(np.float64)), M.relinf(var, ref["variances"].astype(np.float64)), dl, l1 - l0))
        M.check_vec("observe.refit.mean", mean, ref["means"].astype(np.float64), TOL_POST)
        M.check_vec("observe.refit.variance", var, ref["variances"].astype(np.float64), TOL_POST)
        err = abs(dl - (l1 - l0)) / abs(l1)
        M.record("observe.dlog_oracle", err, TOL_L)
        assert err <= TOL_L, (mode, dl, l1 - l0)


@gpu
@pytest.mark.parametrize("m", [50, 129])
def test_derived_state_is_formed_again_after_an_observation(m, monkeypatch):
    """predict_input_grad with variances (forms M) and sample_paths (forms the weights) BEFORE observe; the same calls AFTER it
    equal a fresh problem's that went the same way without them, bit for bit; acquire's variance equals predict's."""
    monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")  # (M is kept in memory on the engine path only)
    monkeypatch.setenv("GPRHIP_MID_PATH", "0")
    c = Case("iso", N + 64, m, 3)
    X, y, Xn, yn, Z, args = split(c, 3)
    Xt = np.asfortranarray(data(c)[0][:, N + 10:N + 50])
    z = np.asfortranarray(np.random.default_rng(3).normal(size=(m, 5)))
    outs = []
    for warm in (True, False):
        p, _, _ = prepared("base", c)
        try:
            if warm:
                p.predict_input_grad(Xt)
                p.sample_paths(Xt, z)
                p.debug_fetch_matrix("pg_m")
            p.observe(Xn, yn)
            if warm:
                for name in ("pg_m", "sp_a"):
                    with pytest.raises(gpr_amd.GprHipError):
                        p.debug_fetch_matrix(name)
            g = p.predict_input_grad(Xt)
            s = p.sample_paths(Xt, z)
            mean, var = p.predict(Xt, predictive=True)
            a = p.acquire(Xt, "ei", maximise=True, best=0.1, predictive=True, want=("values", "variances"))
            outs.append(dict(g, samples=np.asarray(s["samples"] if isinstance(s, dict) else s), pm=p.debug_fetch_matrix("pg_m")))
            assert np.array_equal(a["variances"], g["variances"])
            M.check_vec("observe.stale.var", g["variances"], var, 1e-12)
        finally:
            p.close()
    assert same_bits(outs[0], outs[1])


@gpu
@pytest.mark.parametrize("variant,m", [("base", 50), ("base", 300), ("loaded", 129), ("model-only", 129)])
def test_save_observe_restore_gives_the_bits_back(variant, m):
    c = Case("iso", N + 64, m, 3)
    X, y, Xn, yn, Z, args = split(c, 3)
    Xt = np.asfortranarray(data(c)[0][:, N + 10:N + 50])
    p, targets, _ = prepared(variant, c)
    try:
        with pytest.raises(gpr_amd.GprHipError) as e:
            p.posterior_restore()
        assert e.value.status == _lib.ESTATE
        pre, pred = fetch(p, targets), p.predict(Xt, want_variances=True)
        p.posterior_save()
        p.observe(Xn, yn if targets else None)
        assert p.observed_count == 3 and not same_bits(pre, fetch(p, targets))
        for _ in range(2):
            p.posterior_restore()
            assert p.observed_count == 0 and same_bits(pre, fetch(p, targets))
            again = p.predict(Xt, want_variances=True)
            assert np.array_equal(pred[1], again[1]) and (not targets or np.array_equal(pred[0], again[0]))
            p.observe(Xn[:, :1], yn[:1] if targets else None)
        if variant == "base":
            p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
            assert p.observed_count == 0
            with pytest.raises(gpr_amd.GprHipError) as e:
                p.posterior_restore()
            assert e.value.status == _lib.ESTATE
    finally:
        p.close()


def _raw_observe(p, x, ld, y, k, on_device=0):
    xp = C.c_void_p(x.ctypes.data) if isinstance(x, np.ndarray) else x
    yp = None if y is None else C.c_void_p(y.ctypes.data)
    return p._lib.gprhip_observe(p._handle(), xp, ld, yp, k, None, on_device)



@gpu
def test_refusals_leave_every_bit_of_the_state():
    """Every GPRHIP_EBADARG and GPRHIP_ESTATE case of the header text: the status, the fetched state bit for bit where the
    state can be fetched at all, and a clean call afterwards."""
    torch = pytest.importorskip("torch")
    c = Case("iso", N + 64, 65, 3)
    X, y, Xn, yn, Z, args = split(c, 3)

    def refused(p, call, status, targets=True, fetchable=True):
        pre = fetch(p, targets) if fetchable else None
        count = p.observed_count
        assert call() == status, (status, _lib.load().gprhip_last_error())
        assert p.observed_count == count
        if fetchable:
            assert same_bits(pre, fetch(p, targets))

    p, _, _ = prepared("base", c)
    try:
        bad = Xn.copy()
        bad[1, 2] = np.inf
        ybad = yn.copy()
        ybad[0] = np.nan
        big = np.zeros((3, 65), order="F")
        for call in (lambda: _raw_observe(p, Xn, 3, yn, 0), lambda: _raw_observe(p, big, 3, np.zeros(65), 65),
                     lambda: _raw_observe(p, Xn, 2, yn, 3), lambda: _raw_observe(p, bad, 3, yn, 3),
                     lambda: _raw_observe(p, Xn, 3, ybad, 3), lambda: _raw_observe(p, Xn, 3, None, 3),
                     lambda: _raw_observe(p, Xn, 4, yn, 3, 1)):
            refused(p, call, _lib.EBADARG)
        p.observe(Xn, yn)  # a clean call follows
        assert p.observed_count == 3
        # an evaluation in flight (stage != 0): nothing can be fetched either; the finished evaluation serves again
        ar1 = torch.zeros(p.ar1_len(), dtype=torch.float64, device="cuda")
        ar2 = torch.zeros(p.ar2_len(), dtype=torch.float64, device="cuda")
        p.eval_pass1(ar1.data_ptr(), N, sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
        refused(p, lambda: _raw_observe(p, Xn, 3, yn, 3), _lib.ESTATE, fetchable=False)
        p.eval_pass2(ar1.data_ptr(), ar2.data_ptr())
        refused(p, lambda: _raw_observe(p, Xn, 3, yn, 3), _lib.ESTATE, fetchable=False)
        p.eval_finish(ar2.data_ptr())
        assert p.observed_count == 0
        p.observe(Xn, yn)
        assert p.observed_count == 3
    finally:
        p.close()
    q = problem(c)
    try:
        refused(q, lambda: _raw_observe(q, Xn, 3, yn, 3), _lib.ESTATE, fetchable=False)           # no model
        q.set_inputs(X)
        q.set_targets(y)
        ev = q.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
        q.load_predictor(sigma2=SIGMA2, inducing=Z, coeffs=ev.coeffs, **args)
        refused(q, lambda: _raw_observe(q, Xn, 3, yn, 3), _lib.ESTATE, fetchable=False)           # no factors
        mean = q.predict(Xn, want_variances=False)[0]
        q.set_targets_many(np.asfortranarray(np.stack([y, 2 * y], axis=1)))
        q.eval_targets(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
        refused(q, lambda: _raw_observe(q, Xn, 3, yn, 3), _lib.ESTATE, targets=False)              # after eval_targets
        # a model-only state takes no targets
        q.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, model_only=True, **args)
        refused(q, lambda: _raw_observe(q, Xn, 3, yn, 3), _lib.EBADARG, targets=False)
        assert _raw_observe(q, Xn, 3, None, 3) == _lib.OK and q.observed_count == 3 and np.all(np.isfinite(mean))
    finally:
        q.close()
    f = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N, 3, 3, 65, precision=gpr_amd.F32_BULK)
    try:
        f.set_inputs(X)
        f.set_targets(y)
        f.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
        before = f.predict(Xn)
        refused(f, lambda: _raw_observe(f, Xn, 3, yn, 3), _lib.EBADARG, targets=False)             # fp32-bulk
        after = f.predict(Xn)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        f.close()
    cm = Case("fat", N + 64, 65, 3, 3)
    Xm, ym, Xnm, ynm, Zm, am = split(cm, 3)
    g = problem(cm)
    try:
        g.set_inputs(Xm)
        g.set_targets(ym)
        g.eval(sigma2=SIGMA2, inducing=Zm, want_grad=False, log_multiscales_m05=np.full((3, 65), -0.7, order="F"), **am)
        refused(g, lambda: _raw_observe(g, Xnm, 3, ynm, 3), _lib.EBADARG)                          # multiscales
        g.eval(sigma2=SIGMA2, inducing=Zm, want_grad=False, **am)
        g.observe(Xnm, ynm)
        assert g.observed_count == 3
    finally:
        g.close()
    cw = Case("iso", N + 64, 65, 65)
    Xw, yw, Xnw, ynw, Zw, aw = split(cw, 3)
    w = problem(cw)
    try:
        w.set_inputs(Xw)
        w.set_targets(yw)
        w.eval(sigma2=SIGMA2, inducing=Zw, want_grad=False, **aw)
        before = w.predict(Xnw)
        refused(w, lambda: _raw_observe(w, Xnw, 65, ynw, 3), _lib.EBADARG)                         # d > 64
        after = w.predict(Xnw)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        w.close()


@gpu
def test_not_positive_definite_comes_back_before_anything_is_written():
    """A state in which s <= 0 is certain, not left to rounding: a predictor loaded with 0.9 U in the place of U = chol_km, so
    that |K_xm U^-1|^2 = sf2 (1 - O(jitter)) / 0.81 at a point ON an inducing point and s = sf2 (1 - 1 / 0.81) + sigma2 =
    -0.13.  The second of three new points is that one and the third has s = 0.34: GPRHIP_ENOTPOSDEF, every bit of the state as
    it was (the third point alone would have been folded in), and a clean call with the points of positive s follows."""
    c = Case("iso", N + 64, 65, 3)
    X, y, Xn, yn, Z, args = split(c, 3)
    p, _, ev = prepared("base", c)
    q = problem(c)
    try:
        u, r = p.co_variance_coeffs()
        q.load_predictor(sigma2=SIGMA2, inducing=Z, coeffs=ev.coeffs, co_variance_coeffs=(np.asfortranarray(0.9 * u), r), **args)
        pre = fetch(q)
        on = Xn.copy()
        on[:, 1] = Z[:, 7]
        rw = O.rows(on, Z, pre["uinv"], SIGMA2, None, **hypers_of(c, args))
        print("s of the three new points in 80 bits:", np.asarray(rw["s"], np.float64))
        good = [i for i in range(3) if rw["s"][i] > 0.05]      # (far from the sign change: the device agrees)
        assert rw["s"][1] < -0.1 and good and good[-1] == 2
        assert _raw_observe(q, on, 3, yn, 3) == _lib.ENOTPOSDEF
        assert same_bits(pre, fetch(q)) and q.observed_count == 0
        q.observe(np.asfortranarray(on[:, good]), yn[good].copy())
        assert q.observed_count == len(good) and not same_bits(pre, fetch(q))
    finally:
        p.close()
        q.close()


@gpu
def test_two_runs_repeat_and_a_greedy_batch_comes_back_to_its_start():
    c = Case("iso", N + 64, 129, 3)
    X, y, Xn, yn, Z, args = split(c, 64)
    # candidates ON inducing points and an exploring criterion (mean + 10 sigma): FITC learns about a point only through the
    # inducing points that see it -- beyond their reach the variance stays sf2 whatever is observed there, and a greedy batch
    # would name that one candidate again and again.  In 80 bits this batch is [33, 18, 46, 25], the gaps 4e-2 and more.
    cand = np.asfortranarray(Z[:, :64].copy())
    runs = []
    for _ in range(2):
        p, _, _ = prepared("base", c)
        try:
            p.observe(Xn, yn)
            runs.append(fetch(p))
        finally:
            p.close()
    assert same_bits(runs[0], runs[1])
    p, _, _ = prepared("base", c)
    try:
        start = fetch(p)
        p.posterior_save()
        chosen = []
        for _ in range(4):
            a = p.acquire(cand, "bound", maximise=True, kappa=10.0, predictive=False, want=("values", "means"), top_k=1)
            i = int(a["top_index"][0])
            chosen.append(i)
            p.observe(cand[:, i:i + 1], a["means"][i:i + 1])   # the fantasy: the posterior mean (kriging believer)
        assert p.observed_count == 4 and len(set(chosen)) == 4, chosen
        p.posterior_restore()
        assert same_bits(start, fetch(p)) and p.observed_count == 0
    finally:
        p.close()


@gpu
def test_device_buffers_give_the_bits_of_host_buffers():
    torch = pytest.importorskip("torch")
    c = Case("proj", N + 64, 129, 3, 5, True)
    X, y, Xn, yn, Z, args = split(c, 3)
    outs = []
    for dev in (False, True):
        p, _, _ = prepared("base", c)
        try:
            if dev:
                xd = torch.tensor(np.ascontiguousarray(Xn.T), device="cuda")
                yd = torch.tensor(yn, device="cuda")
                torch.cuda.synchronize()
                dl = p.observe(None, want_dlog_evidence=True, device_ptrs=(xd.data_ptr(), yd.data_ptr(), 3))
            else:
                dl = p.observe(Xn, yn, want_dlog_evidence=True)
            outs.append(dict(fetch(p), dl=np.array([dl])))
        finally:
            p.close()
    assert same_bits(outs[0], outs[1])
