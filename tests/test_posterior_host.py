"""The CPU half of tests/test_gpu_posterior.py: the 80-bit reference of tests/posterior_ref.py and its bounds are pinned here,
before any device is involved, on the oracle's own t, U^-1 and R~^-1 (U = chol_km, R~^-1 = U r_mat^-1, inverted in 80 bits):
  1. the reference reproduces the oracle's means, variances, FITC / FIC covariances, sampler draws and statistics;
  2. on every model of every GPU list (predict, covariances, statistics, loaded predictors, target columns), plain float64
     restatements of each formula -- means, target-column means, variances, FITC / FIC, training means and sums, samples;
     two summation orders, left to right and pairwise in blocks of 16 -- and a float32 restatement of the fp32-bulk form,
     the shifted expansion of its training means included, stay inside every bound;
  3. planted defects miss the bound of the output they touch by at least 100 x, so no bound is vacuous;
  4. the gap this file closes: a small variance perturbed by 1e-9 max |var| passes the max-norm assertion and fails the bound.
Worst ratios, miss factors and the size of each bound against the largest reference entry and sf2 go through tests/margins.py.
"""
import functools

import numpy as np
import pytest

from oracle import fitc_oracle as O
from tests import margins as M
from tests import posterior_ref as R
from tests.test_gpu_factors import factor_ratio
from tests.test_gpu_posterior import HOST_CASES, STATS, STATS_F32, Case, N, _factor_case, case_id, data, geometry, hypers_of, points, stats_shift
from tests.util import _ld_triu_inverse

TOL_POST = 3e-10       # as tests/test_gpu_parity.py
TOL_COV = 1e-8
POWER = 100.0
NT = 129


def model_key(c):
    """The case less what the CPU half does not see (path, environment, chunks)"""
    return c._replace(path="", env=(), chunk=0)


MODELS = sorted(set(model_key(c) for c in HOST_CASES), key=case_id)


@functools.lru_cache(maxsize=4)
def _oracle(c):
    """The oracle's model of a case and its operands: dict(model, ok, t, uinv, rinv)"""
    X, y, Z, args = data(c)
    if c.kind == "iso":
        ok = O.SeIsoKernel(args["log_ell"], args["log_sf2"])
    else:
        ok = O.SeFatKernel(c.d, args["log_sf2"], args.get("tproj"), args.get("log_hetero_skedasticity"), args.get("log_multiscales_m05"))
    ref = O.evaluate(ok, Z, X, y, c.sigma2, variational=c.variational, want_grad=False, keep=True)
    model = ref["model"]
    U = np.triu(model["inducing"]["chol_km"]).astype(R.LD)
    uinv = _ld_triu_inverse(U)
    rinv = np.triu(U @ _ld_triu_inverse(np.triu(model["r_mat"]).astype(R.LD)))
    return dict(model=model, ok=ok, t=ref["coeffs"], uinv=uinv.astype(np.float64), rinv=rinv.astype(np.float64), l=ref["l"])


def _operands(c):
    o = _oracle(c)
    if c.f32:
        return o["t"], o["uinv"].astype(np.float32), o["rinv"].astype(np.float32)
    return o["t"], o["uinv"], o["rinv"]


# ---- 1. the reference against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in MODELS if not c.f32], ids=case_id)
def test_the_reference_reproduces_the_oracle(c):
    X, y, Z, args = data(c)
    o = _oracle(c)
    ok, model = o["ok"], o["model"]
    Xt, far = points(c, 65)
    g = geometry(c, 65)
    mu, _ = R.mean(g, o["t"])
    M.check_vec("host.mean", mu.astype(np.float64), O.predict_means(ok, Z, o["t"], Xt), TOL_POST)
    ch = R.chain(g, o["uinv"], o["rinv"])
    for predictive in (False, True):
        var, _ = R.variance(g, ch, c.sigma2 if predictive else 0.0)
        M.check_vec("host.variance", var.astype(np.float64), O.predict_variances(ok, Z, model, Xt, predictive=predictive), TOL_COV)
    fitc, _ = R.covariances(g, ch, "FITC", 0.0)
    fic, _ = R.covariances(g, ch, "FIC", 0.0)
    M.check_vec("host.fitc", np.triu(fitc.astype(np.float64)), O.fitc_covariances(ok, Z, model, Xt), TOL_COV)
    M.check_vec("host.fic", np.triu(fic.astype(np.float64)), O.fic_covariances(ok, Z, model, Xt), TOL_COV)
    # sampler: the oracle's factor as the given operand
    near = ~far
    cov = np.triu(fitc.astype(np.float64))[np.ix_(near, near)]
    smp = O.cov_sampler_calc(mu.astype(np.float64)[near], cov, c.sigma2, predictive=True)
    z = np.random.default_rng(5).normal(size=(int(near.sum()), 5))
    s, _ = R.samples(np.triu(smp["cov_chol"]).T, smp["means"], z)
    M.check_vec("host.samples", s.astype(np.float64), O.cov_sampler_samples(smp, z), TOL_POST)
    # statistics from the training means
    gt = R.geometry(X, Z, **hypers_of(c, args))
    tm = R.mean(gt, o["t"])[0].astype(np.float64)
    st, ref = R.train_stats(y, tm), O.stats_calc(y, tm, o["l"])
    n = c.n
    assert st["maxad"] == ref["maxad"]
    M.check_vec("host.stats", [float(st["sums"][0]), float(st["sums"][1]) / n, float(st["sums"][3]) / n],
                [ref["sse"], ref["mad"], ref["target_variance"]], TOL_POST)


# ---- 2. float64 / float32 restatements inside the bounds ----------------------------------------------------------------------
def _sum_lr(terms):
    """left to right over the last axis"""
    acc = np.zeros(terms.shape[:-1], dtype=terms.dtype)
    for c in range(terms.shape[-1]):
        acc = acc + terms[..., c]
    return acc


def _sum_pw(terms):
    """pairwise in blocks of 16 over the last axis: blocks left to right, then the blocks' sums left to right"""
    n = terms.shape[-1]
    parts = [_sum_lr(terms[..., lo:lo + 16]) for lo in range(0, n, 16)]
    return _sum_lr(np.stack(parts, axis=-1))


def _matmul(A, B, order):
    out = np.empty((A.shape[0], B.shape[1]), dtype=np.result_type(A, B))
    for j in range(B.shape[1]):
        out[:, j] = order(A * B[:, j][None, :])
    return out


def kernel64(Xt, Z, *, iso, log_sf2, log_ell=0.0, tproj=None, log_ms=None, bulk32=False, plain=False):
    """K in float64 as the direct-difference kernels form it (plain: between the projected points, no multiscales)"""
    P = Xt if tproj is None else tproj.T @ Xt
    Zz = P if plain else Z
    ms = None if (log_ms is None or plain) else np.exp(log_ms) + 0.5
    ie2h = -0.5 * np.exp(-2.0 * log_ell) if iso else -0.5
    acc = np.zeros((P.shape[1], Zz.shape[1]))
    for k in range(P.shape[0]):
        diff = P[k][:, None] - Zz[k][None, :]
        acc = acc + diff * diff if ms is None else (acc + diff * (diff / ms[k][None, :])) + np.log(ms[k][None, :])
    return P, np.exp(log_sf2 + ie2h * acc)


def restate(c, Xt, t, uinv, rinv, order, add=0.0, defect=None):
    """Every posterior output in float64 (c.f32: the n x m operands and products in float32), with one planted defect"""
    X, y, Z, args = data(c)
    hyp = hypers_of(c, args)
    sf2 = np.exp(hyp["log_sf2"])
    P, K = kernel64(Xt, Z, **hyp)
    m, nt = c.m, Xt.shape[1]
    if defect == "column":
        K[:, m - 1] = 0.0
    T = np.float32 if c.f32 else np.float64
    Kb = K.astype(T)
    mu = order(Kb.astype(np.float64) * (t if defect != "stale_t" else np.r_[t[:m // 2], 1.25 * t[m // 2], t[m // 2 + 1:]])[None, :])
    Ui, Ri = np.triu(uinv).astype(T), np.triu(rinv).astype(T)
    V = _matmul(Kb, Ri if defect == "ri_for_ui" else Ui, order).astype(T)
    Q = _matmul(V, Ri, order).astype(T)
    V64, Q64 = V.astype(np.float64), Q.astype(np.float64)
    k, b = order(V64 * V64), order(Q64 * Q64)
    var = (sf2 - ((k + b) if defect == "k_plus_b" else (k - b))) + (0.0 if defect == "no_add" else add)
    if defect == "row":          # the last row of the second 4-row block
        mu[7], var[7] = 0.0, sf2 + add
    out = dict(mean=mu, variance=var, target_means=_matmul(Kb.astype(np.float64), _target_columns(t), order))
    if not c.f32:
        Ktt = kernel64(Xt, Z, **dict(hyp, log_ms=None), plain=True)[1]
        if defect == "ms_in_ktt" and hyp["log_ms"] is not None:
            ms = np.exp(hyp["log_ms"]) + 0.5
            Ktt = Ktt * np.exp(-0.5 * np.log(ms[:, :1]).sum())
        QQ, VV = _matmul(Q64, Q64.T, order), _matmul(V64, V64.T, order)
        out["FITC"] = (Ktt - VV) + QQ + add * np.eye(nt)
        dg = sf2 - (k if defect == "fic_from_v" else order(K * K))
        out["FIC"] = QQ + np.diag(dg + add)
    return out


def _target_columns(t):
    """Three coefficient columns (the coefficients are linear in the targets): given operands of the target-column means"""
    return np.asfortranarray(np.outer(t, [1.0, 1.25, -0.5]))


def reference(c, Xt, g, t, uinv, rinv, add):
    ch = R.chain(g, uinv, rinv)
    out = dict(mean=R.mean(g, t), variance=R.variance(g, ch, add), target_means=R.mean(g, _target_columns(t)))
    if not c.f32:
        out["FITC"], out["FIC"] = R.covariances(g, ch, "FITC", add), R.covariances(g, ch, "FIC", add)
    return out


@functools.lru_cache(maxsize=2)
def _reference(c, add):
    t, uinv, rinv = _operands(c)
    return reference(c, points(c, NT)[0], geometry(c, NT), t, uinv, rinv, add)


@pytest.mark.parametrize("c", MODELS, ids=case_id)
def test_float_restatements_stay_inside_every_bound(c):
    t, uinv, rinv = _operands(c)
    Xt, far = points(c, NT)
    ref = _reference(c, c.sigma2)
    sf2 = float(geometry(c, NT)["sf2"])
    for name, order in (("left_to_right", _sum_lr), ("pairwise16", _sum_pw)):
        got = restate(c, Xt, t, uinv, rinv, order, add=c.sigma2)
        for what, (val, bound) in ref.items():
            r, at = R.ratio(got[what], val, bound)
            M.record("host.%s.%s" % (what, name), r, 1.0, case=case_id(c))
            assert r <= 1.0, (case_id(c), what, name, r, at)
            if what in ("mean", "variance"):       # far points: nothing but the underflow allowance
                assert np.all(got[what][far] == (0.0 if what == "mean" else (sf2 - 0.0) + c.sigma2))
    for what, (val, bound) in ref.items():           # how large the bound is: a record, the power test is the condition
        scale = float(np.max(np.abs(val)))
        M.record("host.bound_over_scale.%s" % what, float(np.max(bound)) / scale, 1.0, case=case_id(c),
                 over_sf2=float(np.max(bound)) / sf2)


def train_kernel64(c, X, Z, hyp, shift):
    """K_nm as gprhip_train_stats builds it: direct differences, or with a shift the expansion of cov_cross_mfma_kernel"""
    if shift is None:
        return kernel64(X, Z, **hyp)[1]
    Pt, Zt = X - shift[:, None], Z - shift[:, None]
    dist = np.maximum((Pt * Pt).sum(0)[:, None] + (Zt * Zt).sum(0)[None, :] - 2.0 * (Pt.T @ Zt), 0.0)
    return np.exp(hyp["log_sf2"] - 0.5 * np.exp(-2.0 * hyp["log_ell"]) * dist)


@pytest.mark.parametrize("c", sorted(set(model_key(c) for c in STATS + STATS_F32), key=case_id), ids=case_id)
def test_training_means_and_sums_restated_stay_inside_their_bounds(c):
    X, y, Z, args = data(c)
    hyp = hypers_of(c, args)
    t = _operands(c)[0]
    shift = stats_shift(c, Z)
    mu_ref, mu_b = R.mean(R.geometry(X, Z, **hyp, shift=shift), t)
    K = train_kernel64(c, X, Z, hyp, shift)
    K = K.astype(np.float32).astype(np.float64) if c.f32 else K
    for name, order in (("left_to_right", _sum_lr), ("pairwise16", _sum_pw)):
        mu = order(K * t[None, :])
        r, at = R.ratio(mu, mu_ref, mu_b)
        M.record("host.train_means.%s" % name, r, 1.0, case=case_id(c))
        assert r <= 1.0, (case_id(c), name, r, at)
        st = R.train_stats(y, mu)
        res = y - mu
        assert np.max(np.abs(res)) == st["maxad"]
        for i, terms in ((0, res * res), (1, np.abs(res)), (3, y * y)):
            rel = abs(float((R.LD(order(terms)) - st["sums"][i]) / st["sums"][i]))
            M.record("host.train_sums.%s" % name, rel / st["rel"], 1.0, case=case_id(c))
            assert rel <= st["rel"], (case_id(c), name, i, rel)
    if shift is not None:      # the expansion's bound is no wider than the store's rounding allows: K off by 1e-4 misses it
        bad = order(train_kernel64(c, X, Z, dict(hyp, log_sf2=hyp["log_sf2"] + 1e-4), shift) * t[None, :])
        miss = R.ratio(bad, mu_ref, mu_b)[0]
        M.record("host.defect.expansion_k_off_1e-4.train_means", miss, POWER, case=case_id(c))
        assert miss >= POWER, miss


# ---- 3. planted defects -------------------------------------------------------------------------------------------------------
SMALLEST = Case("", "iso", N, 17, 3)
DEFECTS = [("column", Case("", "iso", N, 65, 3), ("mean", "variance", "FITC", "FIC")), ("row", SMALLEST, ("mean", "variance")),
           ("k_plus_b", SMALLEST, ("variance",)), ("no_add", SMALLEST, ("variance",)), ("stale_t", SMALLEST, ("mean",)),
           ("ri_for_ui", SMALLEST, ("variance", "FITC")), ("ms_in_ktt", Case("", "fat_ms", N, 17, 3), ("FITC",)),
           ("fic_from_v", SMALLEST, ("FIC",))]


@pytest.mark.parametrize("defect,c,outputs", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defects_miss_the_bound_by_100(defect, c, outputs):
    assert model_key(c) in MODELS, c
    t, uinv, rinv = _operands(c)
    Xt, far = points(c, NT)
    ref = _reference(c, c.sigma2)
    got = restate(c, Xt, t, uinv, rinv, _sum_pw, add=c.sigma2, defect=defect)
    for what in outputs:
        val, bound = ref[what]
        r, at = R.ratio(got[what], val, bound)
        M.record("host.defect.%s.%s" % (defect, what), r, POWER, case=case_id(c))
        assert r >= POWER, (defect, what, r)


def test_planted_defects_of_the_sampler_miss_by_100():
    c = SMALLEST
    t, uinv, rinv = _operands(c)
    g = geometry(c, NT)
    near = ~points(c, NT)[1]
    cov = R.covariances(g, R.chain(g, uinv, rinv), "FITC", 0.0)[0].astype(np.float64)[np.ix_(near, near)]
    nt = cov.shape[0]
    A = np.triu(cov).astype(R.LD)
    A[np.diag_indices(nt)] += R.LD(0.05) + R.LD(1e-6)
    U = np.linalg.cholesky(np.asarray(A + np.triu(A, 1).T, np.float64)).T
    assert factor_ratio(U, A)[0] <= 4.0
    bad = U.copy()                       # one 16 x 16 sub-tile of the diagonal block transposed
    bad[0:16, 16:32] = U[0:16, 16:32].T
    miss = factor_ratio(bad, A)[0] / 4.0
    M.record("host.defect.subtile_transposed", miss, POWER)
    assert miss >= POWER, miss
    rng = np.random.default_rng(8)
    means, z = rng.normal(size=nt), rng.normal(size=(nt, 5))
    s, bound = R.samples(U.T, means, z)
    for name, order in (("left_to_right", _sum_lr), ("pairwise16", _sum_pw)):
        ok = means[:, None] + _matmul(np.ascontiguousarray(U.T), z, order)
        r = R.ratio(ok, s, bound)[0]
        M.record("host.samples.%s" % name, r, 1.0, case=case_id(c))
        assert r <= 1.0, (name, r)
    ok[:, 3] += means                    # one column added the mean twice
    miss = R.ratio(ok, s, bound)[0]
    M.record("host.defect.mean_twice", miss, POWER)
    assert miss >= POWER, miss


# ---- 4. the gap ---------------------------------------------------------------------------------------------------------------
def test_a_small_variance_off_in_its_fourth_digit_passes_the_max_norm_and_fails_the_bound():
    c = model_key(Case("small", "iso", N, 17, 3, sigma2=1e-4))
    t, uinv, rinv = _operands(c)
    Xt, far = points(c, NT)
    g = geometry(c, NT)
    var, bound = R.variance(g, R.chain(g, uinv, rinv), 0.0)
    ref = var.astype(np.float64)
    i = int(np.argmin(ref))
    assert ref[i] <= 2e-3 * float(g["sf2"]), ref[i]         # a test point next to the data
    got = restate(c, Xt, t, uinv, rinv, _sum_lr)["variance"]
    got[i] += 1e-9 * np.max(np.abs(ref))
    assert np.max(np.abs(got - ref)) <= 1e-8 * np.max(np.abs(ref))         # the existing assertion passes
    r, at = R.ratio(got, var, bound)
    M.record("host.gap", r, 1.0, case=case_id(c), smallest=float(ref[i]))
    assert r > 1.0 and at == i, (r, at, i)                              # the new one fails, at that entry
