"""The two Cholesky factorisations of an evaluation, U = chol(K_m + jitter) and R~ = chol(B~), against their definition on
every path of gpr_amd/csrc/chol.hip, and the `potrf info` status against LAPACK's at every micro-panel and block edge.

1. Factor residuals.  The device's own K_m (debug_fetch_matrix("km")) isolates the factorisation from the covariance
   kernels.  With A = triu(km) + (jitter + exp(log_hetero)) I and P = U^T U formed in numpy longdouble, every entry of the
   upper triangle obeys
       |P - A|_ij <= 4 gamma_{m+1} (|U|^T |U|)_ij + 2 u |A_ij|,    gamma_k = k u / (1 - k u), u = 2^-53
   (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3: gamma_{m+1} |U|^T |U| holds for any summation order;
   the factor 4 covers the reciprocal-square-root pivots and the device's rounding of the diagonal sum, 2 u |A_ij| the
   rounding of A itself).  The bound carries no condition number.  R = R~ U does: it is compared with the oracle's r_mat at
   TOL_FACTOR on inducing points whose cond(K_m + jitter I) <= 1e6 is asserted on the CPU, and R~ alone through the
   residual of R^T R against U^T U + K_mn S^-1 K_nm.
2. The inverse-only pass (flags & 1) over imported factors of 1 .. 3 blocks with identity padding.
3. A failing minor: inducing point c sits at (100 c, 0), so every off-diagonal entry of K_m underflows, the jitter is
   -1e-3 and the points of a defect are exact copies of earlier ones -- every pivot before the defect is 0.999, the pivot
   at the copy -0.002.  Nothing depends on a cancellation to exactly zero.  The order in the message must be dpotrf's info.

The reference halves (_factor_reference, minor_reference) are plain CPU functions; test_minor_references_hold_on_the_cpu
checks the second without a device.
"""
import functools
import os

import numpy as np
import pytest
import scipy.linalg
from scipy.linalg import lapack

import gpr_amd
from gpr_amd import _lib
from oracle import fitc_oracle as O
from tests import margins as M
from tests.util import factor_case
from tests.util import oracle_km_full as _oracle_km_full
from tests.util import taken as _taken

gpu = pytest.mark.gpu

TOL_L = 7e-10          # as tests/test_gpu_parity.py
TOL_POST = 3e-10
TOL_FACTOR = 1e-11
TOL_SHARD = 2e-14
TOL_SHARD_GRAD = 1e-9

LD = np.longdouble
U64 = 2.0 ** -53
SIGMA2 = 0.1
COND_MAX = 1e6
ENGINE_ENV = {"GPRHIP_SMALL_PATH": "0", "GPRHIP_MID_PATH": "0"}


def _path_of(m):
    return "small" if m <= 64 else ("mid" if m <= 256 else "engine")


# ---- 1. factor residuals ---------------------------------------------------------------------------------------------------
M_SMALL = [1, 2, 15, 16, 17, 33, 48, 49, 63, 64]
M_MID = [65, 80, 81, 127, 128, 129, 255, 256]
M_ENGINE = [257, 272, 273, 383, 384, 385, 641]
M_PARTLY_LIVE = [17, 50, 64, 100]
M_INVERSE = [49, 64, 65, 129, 273]
N_TRAIN = 800


@functools.lru_cache(maxsize=None)
def _factor_case(kind, m):
    """Inputs, targets, inducing points, Problem.eval arguments, the oracle's kernel, cond(K_m + jitter I).  The tests
    assert cond <= COND_MAX = 1e6, the bound the comparison of R relies on; the length scale is CHOSEN a decade inside it,
    as the largest of 0.8^k at which the oracle's K_m + jitter I has a condition number of at most 1e5 (asserted in
    tests/util.py::factor_case: the search may not run out).  How far from the identity the factors then are -- the share
    of entries above the diagonal of U beyond 1e-8, the largest of them -- is recorded with every factor_U figure
    (profiles/factor_margins.txt)."""
    return factor_case("iso" if kind == "iso" else "fat_het", N_TRAIN, m)


@functools.lru_cache(maxsize=None)
def _factor_reference(kind, m, variational=False):
    """The CPU half: the oracle's model (r_mat, K_nm, 1/s, coefficients) and the asserted conditioning."""
    X, y, Z, _, ok, cond = _factor_case(kind, m)
    assert cond <= COND_MAX, (kind, m, cond)
    ref = O.evaluate(ok, Z, X, y, SIGMA2, variational=variational, want_grad=False, keep=True)
    return ref


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def factor_ratio(U, A):
    """max over the upper triangle of (|U^T U - A|_ij - 2 u |A_ij| - eta) / (gamma_{m+1} (|U|^T |U|)_ij), the product in
    longdouble; A longdouble, upper triangle.  Returns (ratio, P).
    eta = (m + 1) 2^-1022: Thm 10.3 assumes that nothing underflows.  At the short length scales of the larger cases entries
    of K_m are down at 1e-300 and the products U_ki U_kj below the smallest fp64 number, for LAPACK as for the device; each
    of the at most m + 1 operations behind an entry is then off by less than the smallest normal number, whatever the
    underflow mode.  Where (|U|^T |U|)_ij itself underflows to zero, eta and the rounding of A are all the bound allows."""
    m = U.shape[0]
    Ul = np.triu(U).astype(LD)
    P = Ul.T @ Ul
    absU = np.abs(np.triu(U))
    scale = (gamma(m + 1) * (absU.T @ absU)).astype(LD)
    iu = np.triu_indices(m)
    eta = LD(m + 1) * LD(2.0 ** -1022)
    excess = np.maximum(np.abs(P - A)[iu] - LD(2.0 * U64) * np.abs(A)[iu] - eta, 0)
    sc = scale[iu]
    ratio = np.where(excess > 0, excess / np.where(sc > 0, sc, LD(1)), LD(0))
    ratio = np.where((excess > 0) & ~(sc > 0), LD(np.inf), ratio)
    return float(np.max(ratio)), P


def _device_matrix(km, jitter, het):
    """A = triu(km) + (jitter + exp(log_hetero)) I in longdouble"""
    A = np.triu(km).astype(LD)
    dg = LD(jitter) + (np.exp(np.asarray(het, LD)) if het is not None else LD(0.0))
    A[np.diag_indices(A.shape[0])] += dg
    return A


def _check_factors(p, kind, m, variational, label):
    """Checks (a), (b), (c) on the problem's last evaluation."""
    X, y, Z, args, ok, cond = _factor_case(kind, m)
    ref = _factor_reference(kind, m, variational)
    model = ref["model"]
    km = p.debug_fetch_matrix("km")
    U, R = p.co_variance_coeffs()
    # (b) structure
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(R)), label
    assert np.all(np.tril(U, -1) == 0.0) and np.all(np.tril(R, -1) == 0.0), label
    assert np.all(np.diag(U) > 0.0) and np.all(np.diag(R) > 0.0), label
    # (a) the definition of U
    A = _device_matrix(km, O.CHOLESKY_JITTER, args.get("log_hetero_skedasticity"))
    ratio, P = factor_ratio(U, A)
    off = np.abs(U[np.triu_indices(m, 1)])
    extra = dict(path=label, m=m, kind=kind, cond=cond, dense=float(np.mean(off > 1e-8)) if m > 1 else 0.0,
                 maxoff=float(np.max(off)) if m > 1 else 0.0)
    if os.environ.get("GPR_MARGINS_LOG"):  # LAPACK's figure on the same matrix, for profiles/factor_margins.txt
        c, info = lapack.dpotrf(np.triu(A).astype(np.float64), lower=0, clean=1)
        assert info == 0
        extra["lapack"] = factor_ratio(c, A)[0]
    print("factor_U %s %s m=%d: %.3f of gamma_{m+1} |U|^T |U| (bound 4)" % (label, kind, m, ratio))
    M._record("factor_U", ratio, 4.0, **extra)
    assert ratio <= 4.0, (label, kind, m, ratio)
    # (c) R against the oracle, and R~ alone: R^T R = U^T B~ U = U^T U + K_mn S^-1 K_nm
    M.check_vec("r_mat", np.triu(R), np.triu(model["r_mat"]), TOL_FACTOR)
    knm = model["knm"].astype(LD)
    G = knm.T @ (knm * model["is_vec"].astype(LD)[:, None])
    RtR = np.triu(R).T @ np.triu(R)      # (fp64: its rounding, m u relative, is far below the bound)
    err = float(np.max(np.abs(RtR - (P + G))) / np.max(np.abs(RtR)))
    M._record("factor_RtR", err, TOL_FACTOR, **extra)
    assert err <= TOL_FACTOR, (label, kind, m, err)
    return ratio


def _make_problem(kind, m, X):
    d = X.shape[0]
    return gpr_amd.Problem(gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT, X.shape[1], d, d, m)


def _evaluate_and_check(kind, m, variational, expect, label, targets=False):
    X, y, Z, args, ok, _ = _factor_case(kind, m)
    p = _make_problem(kind, m, X)
    p.set_inputs(X)
    p.set_timing(2)
    if targets:
        p.set_targets_many(np.asfortranarray(y[:, None]))
        p.eval_targets(sigma2=SIGMA2, inducing=Z, variational=variational, **args)
    else:
        p.set_targets(y)
        p.eval(sigma2=SIGMA2, inducing=Z, variational=variational, **args)
    stages = set(p.last_timings())
    assert _taken(stages) == expect and "km_chol" in stages and "b_chol" in stages, (label, stages)
    assert ("p1_targets" in stages) == targets, (label, stages)
    try:
        return _check_factors(p, kind, m, variational, label)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("kind", ["iso", "fat"])
@pytest.mark.parametrize("m", M_SMALL + M_MID + M_ENGINE)
def test_factors_on_the_default_path(m, kind):
    _evaluate_and_check(kind, m, False, _path_of(m), _path_of(m))


@gpu
@pytest.mark.parametrize("kind,m", [("iso", 49), ("fat", 129), ("iso", 385)], ids=["small", "mid", "engine"])
def test_factors_of_a_variational_evaluation(kind, m):
    _evaluate_and_check(kind, m, True, _path_of(m), _path_of(m) + "_variational")


@gpu
@pytest.mark.parametrize("entry", ["eval", "eval_targets"])
@pytest.mark.parametrize("kind", ["iso", "fat"])
@pytest.mark.parametrize("m", M_PARTLY_LIVE)
def test_factors_of_a_partly_live_block_through_the_blocked_kernels(m, kind, entry, monkeypatch):
    """m = 17, 50, 64, 100 through the engine path: potrf_upper_blocked over one 128-block with m_real < 128, with and
    without the carried inverse (k_end <= 64 / 112).  gprhip_eval_targets takes the engine path by contract; gprhip_eval
    with both one-kernel paths switched off (read when the problem is created)."""
    if entry == "eval":
        for k_, v_ in ENGINE_ENV.items():
            monkeypatch.setenv(k_, v_)
    _evaluate_and_check(kind, m, False, "engine", "engine_partly_live_" + entry, targets=entry == "eval_targets")


@gpu
@pytest.mark.parametrize("kind", ["iso", "fat"])
@pytest.mark.parametrize("m", M_INVERSE)
def test_the_carried_inverse_through_coefficients_and_variances(m, kind):
    """(d) U^-1 and R~^-1 are not exposed: the mean coefficients t = U^-1 R~^-1 R~^-T ... and the predicted variances
    sf2 - |K_tm U^-1|^2 + |K_tm R^-1|^2 are what they produce."""
    X, y, Z, args, ok, _ = _factor_case(kind, m)
    ref = _factor_reference(kind, m)
    Xt = np.asfortranarray(np.random.default_rng(3).normal(size=(X.shape[0], 200)) * (X.std() / 1.0))
    p = _make_problem(kind, m, X)
    p.set_inputs(X)
    p.set_targets(y)
    p.set_timing(2)
    p.eval(sigma2=SIGMA2, inducing=Z, **args)
    assert _taken(set(p.last_timings())) == _path_of(m)
    t = p.debug_fetch("t")
    _, var = p.predict(Xt, predictive=False)
    p.close()
    M.check_vec("t", t, ref["coeffs"], TOL_POST)
    M.check_vec("pred_var", var, O.predict_variances(ok, Z, ref["model"], Xt, predictive=False), TOL_POST)


# ---- 2. the inverse-only pass of an imported model ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["iso", "fat"])
@pytest.mark.parametrize("m", [17, 64, 65, 129, 300])
def test_imported_factors_through_the_inverse_only_pass(m, kind):
    X, y, Z, args, ok, cond = _factor_case(kind, m)
    assert cond <= COND_MAX
    ref = O.evaluate(ok, Z, X, y, SIGMA2, want_grad=False, keep=True)
    model = ref["model"]
    U = np.asfortranarray(scipy.linalg.cholesky(_oracle_km_full(ok, Z) + O.CHOLESKY_JITTER * np.eye(m), lower=False))
    assert np.max(np.abs(U - np.triu(model["inducing"]["chol_km"]))) <= 1e-13 * np.max(np.abs(U))
    r_mat = np.asfortranarray(np.triu(model["r_mat"]))
    model = dict(model, inducing=dict(model["inducing"], chol_km=U))
    D = X.shape[0]
    nt = 150
    Xt = np.asfortranarray(np.random.default_rng(4).normal(size=(D, nt)) * X.std())
    q = _make_problem(kind, m, Xt)          # a fresh problem that never sees training data
    q.load_predictor(coeffs=ref["coeffs"], co_variance_coeffs=(U, r_mat), sigma2=SIGMA2, inducing=Z, **args)
    means, var = q.predict(Xt, predictive=False)
    M.check_vec("pred_mean", means, O.predict_means(ok, Z, ref["coeffs"], Xt), TOL_POST)
    M.check_vec("pred_var", var, O.predict_variances(ok, Z, model, Xt, predictive=False), TOL_POST)
    for name, cref in (("FITC", O.fitc_covariances(ok, Z, model, Xt)), ("FIC", O.fic_covariances(ok, Z, model, Xt))):
        cov = q.covariances(Xt, kind=name, predictive=False)
        assert np.array_equal(cov, cov.T)
        M.check_vec("cov_" + name, np.triu(cov), cref, TOL_POST)
    u2, r2 = q.co_variance_coeffs()
    q.close()
    assert np.array_equal(u2, U)            # (uploaded and fetched: a copy)
    M.check_vec("r_mat", r2, r_mat, TOL_POST)   # (R~ U with R~ = R U^-1)
    assert np.all(np.tril(r2, -1) == 0.0)


# ---- 3. a failing minor is LAPACK's info ---------------------------------------------------------------------------------------
# (m, failing orders, jitter)
MINOR_SMALL = [(4, (2,), -1e-3), (50, (16,), -1e-3), (50, (17,), -1e-3), (50, (50,), -1e-3), (64, (64,), -1e-3),
               (50, (1,), -2.0), (50, (20, 40), -1e-3)]
MINOR_MID = [(65, (65,), -1e-3), (129, (129,), -1e-3), (200, (128,), -1e-3), (200, (129,), -1e-3), (200, (200,), -1e-3),
             (200, (70, 140), -1e-3)]
MINOR_ENGINE = [(300, (1,), -2.0), (300, (128,), -1e-3), (300, (129,), -1e-3), (300, (256,), -1e-3), (300, (257,), -1e-3),
                (300, (300,), -1e-3), (385, (385,), -1e-3), (300, (130, 260), -1e-3), (300, (100, 120), -1e-3)]
MINOR_ALL = MINOR_SMALL + MINOR_MID + MINOR_ENGINE
N_MINOR = 600
KERNEL_MINOR = O.SeIsoKernel(0.0, 0.0)


def _minor_id(c):
    return "m%d_o%s%s" % (c[0], "_".join(str(o) for o in c[1]), "" if c[2] == -1e-3 else "_j%g" % c[2])


def minor_inducing(m, orders=()):
    """Inducing point c at (100 c, 0); the point of a failing order k > 1 is an exact copy of point (k - 1) // 3, which
    is earlier and never itself a copy in the cases above."""
    Z = np.zeros((2, m), order="F")
    Z[0] = 100.0 * np.arange(m)
    for k in orders:
        if k > 1:
            Z[:, k - 1] = Z[:, (k - 1) // 3]
    return Z


def minor_reference(m, orders, jitter):
    """(Z, dpotrf's info on the oracle's K_m + jitter I, the pivots of a plain Cholesky loop up to and including the failing
    one).  Asserts the construction's margins: failing pivot <= -1e-3, every earlier one >= 0.5, info the intended order."""
    Z = minor_inducing(m, orders)
    km, _ = O.spec_calc_shared_upper(KERNEL_MINOR, Z)
    A = np.triu(np.nan_to_num(km, nan=0.0)) + jitter * np.eye(m)
    _, info = lapack.dpotrf(A, lower=0, clean=0, overwrite_a=0)
    Uc = np.zeros((m, m))
    pivots = []
    for j in range(m):
        piv = A[j, j] - float(np.dot(Uc[:j, j], Uc[:j, j]))
        pivots.append(piv)
        if piv <= 0.0:
            break
        Uc[j, j] = np.sqrt(piv)
        Uc[j, j + 1:] = (A[j, j + 1:] - Uc[:j, j] @ Uc[:j, j + 1:]) / Uc[j, j]
    if orders:
        assert info == min(orders), (m, orders, info)
        assert len(pivots) == info and pivots[-1] <= -1e-3 and all(pv >= 0.5 for pv in pivots[:-1]), (m, orders, pivots[-3:])
    else:
        assert info == 0 and len(pivots) == m and all(pv >= 0.5 for pv in pivots), (m, info)
    return Z, info, pivots


@pytest.mark.parametrize("case", MINOR_ALL, ids=_minor_id)
def test_minor_references_hold_on_the_cpu(case):
    """No device: for every listed case dpotrf's info is the intended order and the pivot margins hold."""
    m, orders, jitter = case
    minor_reference(m, orders, jitter)


@pytest.mark.parametrize("m", sorted({c[0] for c in MINOR_ALL}))
def test_the_inducing_points_without_copies_factorise_on_the_cpu(m):
    """... under the negative jitter too: every pivot is 0.999."""
    minor_reference(m, (), -1e-3)


@functools.lru_cache(maxsize=None)
def _minor_data(m):
    rng = np.random.default_rng(40 + m)
    Zg = minor_inducing(m)
    X = np.asfortranarray(Zg[:, np.arange(N_MINOR) % m] + 0.4 * rng.normal(size=(2, N_MINOR)))
    Y = np.asfortranarray(np.stack([np.sin(X[1] + 0.3 * c) + 0.01 * X[0] / m + 0.1 * rng.normal(size=N_MINOR)
                                    for c in range(3)], axis=1))
    Xt = np.asfortranarray(Zg[:, np.arange(40) % m] + 0.4 * rng.normal(size=(2, 40)))
    return X, Y, Xt, Zg


HYP_MINOR = dict(log_ell=0.0, log_sf2=0.0, sigma2=SIGMA2)


def _same_evaluation(a, b):
    return (a.l1 == b.l1 and a.l2 == b.l2 and a.dl_dsigma2 == b.dl_dsigma2 and np.array_equal(a.grad, b.grad)
            and np.array_equal(a.coeffs, b.coeffs))


def _same_targets_evaluation(a, b):
    return (a.l1 == b.l1 and np.array_equal(a.l2, b.l2) and a.dl_dsigma2_sum == b.dl_dsigma2_sum
            and np.array_equal(a.grad_sum, b.grad_sum) and np.array_equal(a.coeffs, b.coeffs))


def _refused_with_order(call, info):
    with pytest.raises(gpr_amd.NotPositiveDefinite) as e:
        call()
    assert e.value.status == _lib.ENOTPOSDEF
    assert ("leading minor of order %d of K_m" % info) in str(e.value), (info, str(e.value))


def _refusal_through_eval(case, precision=gpr_amd.F64):
    m, orders, jitter = case
    Zbad, info, _ = minor_reference(m, orders, jitter)
    X, Y, Xt, Zg = _minor_data(m)

    def fresh():
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N_MINOR, 2, 2, m, precision=precision)
        p.set_inputs(X)
        p.set_targets(Y[:, 0])
        p.set_timing(2)
        return p

    p = fresh()
    _refused_with_order(lambda: p.eval(inducing=Zbad, jitter=jitter, **HYP_MINOR), info)
    assert _taken(set(p.last_timings())) == _path_of(m), p.last_timings()
    with pytest.raises(gpr_amd.GprHipError, match="holds no V"):
        p.eval(inducing=Zbad, jitter=jitter, reuse_v=True, **HYP_MINOR)
    with pytest.raises(gpr_amd.GprHipError) as e1:
        p.predict(Xt, want_variances=False)
    assert e1.value.status == _lib.ESTATE
    with pytest.raises(gpr_amd.GprHipError) as e2:
        p.train_stats()
    assert e2.value.status == _lib.ESTATE
    after = p.eval(inducing=Zg, **HYP_MINOR)
    q = fresh()
    good = q.eval(inducing=Zg, **HYP_MINOR)
    p.close()
    q.close()
    assert np.isfinite(good.l) and np.all(np.isfinite(good.grad))
    assert _same_evaluation(after, good)


@gpu
@pytest.mark.parametrize("case", MINOR_ALL, ids=_minor_id)
def test_failing_minor_is_lapacks_info(case):
    _refusal_through_eval(case)


@gpu
@pytest.mark.parametrize("case", MINOR_ENGINE, ids=_minor_id)
def test_failing_minor_in_an_fp32_bulk_problem(case):
    """The m x m work of an fp32-bulk problem stays in fp64: the same orders."""
    _refusal_through_eval(case, precision=gpr_amd.F32_BULK)


@gpu
@pytest.mark.parametrize("case", MINOR_ENGINE, ids=_minor_id)
def test_failing_minor_through_eval_targets(case):
    m, orders, jitter = case
    Zbad, info, _ = minor_reference(m, orders, jitter)
    X, Y, Xt, Zg = _minor_data(m)

    def fresh():
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N_MINOR, 2, 2, m)
        p.set_inputs(X)
        p.set_targets_many(Y)
        p.set_timing(2)
        return p

    p = fresh()
    good = p.eval_targets(inducing=Zg, **HYP_MINOR)
    assert p.predict_targets(Xt).shape == (Xt.shape[1], 3)
    _refused_with_order(lambda: p.eval_targets(inducing=Zbad, jitter=jitter, **HYP_MINOR), info)
    stages = set(p.last_timings())
    assert _taken(stages) == "engine" and "p1_targets" in stages, stages
    with pytest.raises(gpr_amd.GprHipError) as e:       # never the coefficients of the earlier evaluation
        p.predict_targets(Xt)
    assert e.value.status == _lib.ESTATE
    with pytest.raises(gpr_amd.GprHipError, match="holds no V"):
        p.eval_targets(inducing=Zbad, jitter=jitter, reuse_v=True, **HYP_MINOR)
    with pytest.raises(gpr_amd.GprHipError) as e1:
        p.predict(Xt, want_variances=False)
    assert e1.value.status == _lib.ESTATE
    with pytest.raises(gpr_amd.GprHipError) as e2:
        p.train_stats()
    assert e2.value.status == _lib.ESTATE
    after = p.eval_targets(inducing=Zg, **HYP_MINOR)
    q = fresh()
    first = q.eval_targets(inducing=Zg, **HYP_MINOR)
    p.close()
    q.close()
    assert np.all(np.isfinite(first.l)) and np.all(np.isfinite(first.grad_sum))
    assert _same_targets_evaluation(after, first) and _same_targets_evaluation(good, first)


@gpu
@pytest.mark.parametrize("case", MINOR_ENGINE, ids=_minor_id)
def test_failing_minor_through_two_shards_of_one_device(case):
    m, orders, jitter = case
    Zbad, info, _ = minor_reference(m, orders, jitter)
    X, Y, Xt, Zg = _minor_data(m)
    q = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N_MINOR, 2, 2, m)
    q.set_inputs(X)
    q.set_targets(Y[:, 0])
    good = q.eval(inducing=Zg, **HYP_MINOR)
    q.close()
    ctx = gpr_amd.Context([0, 0])
    sp = gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, N_MINOR, 2, 2, m)
    try:
        sp.set_inputs(X)
        sp.set_targets(Y[:, 0])
        for i in range(2):
            sp.problem(i).set_timing(2)
        _refused_with_order(lambda: sp.eval(inducing=Zbad, jitter=jitter, **HYP_MINOR), info)
        for i in range(2):
            assert _taken(set(sp.problem(i).last_timings())) == "engine", sp.problem(i).last_timings()
        with pytest.raises(gpr_amd.GprHipError, match="holds no V"):
            sp.eval(inducing=Zbad, jitter=jitter, reuse_v=True, **HYP_MINOR)
        with pytest.raises(gpr_amd.GprHipError) as e1:
            sp.predict(Xt, want_variances=False)
        assert e1.value.status == _lib.ESTATE
        with pytest.raises(gpr_amd.GprHipError) as e2:
            sp.train_stats()
        assert e2.value.status == _lib.ESTATE
        after = sp.eval(inducing=Zg, **HYP_MINOR)
    finally:
        sp.close()
        ctx.close()
    assert M.rel_ok("l", after.l, good.l, TOL_SHARD) and M.rel_ok("dl_dsigma2", after.dl_dsigma2, good.dl_dsigma2, TOL_SHARD)
    assert M.grad_ok(after.grad, good.grad, M.families("iso", 2, m), TOL_SHARD_GRAD)
    assert M.vec_ok("coeffs", after.coeffs, good.coeffs, TOL_SHARD_GRAD)


@gpu
@pytest.mark.parametrize("m,orders", [(50, (17,)), (200, (129,))], ids=["m50", "m200"])
def test_heteroskedastic_noise_lifts_the_negative_jitter(m, orders, monkeypatch):
    """The inducing points of a failing case, jitter -1e-3 and log_hetero_skedasticity = log 0.01 on Cov_se_fat: the
    reference adds exp(.) to the diagonal, every pivot at a copy is 0.009 + 0.01 and the factorisation succeeds."""
    Zbad = minor_inducing(m, orders)
    X, Y, _, _ = _minor_data(m)
    het = np.full(m, np.log(0.01))
    monkeypatch.setattr(O, "CHOLESKY_JITTER", -1e-3)      # (inducing_calc_internal reads it when called)
    ref = O.evaluate(O.SeFatKernel(2, 0.0, None, het, None), Zbad, X, Y[:, 0], SIGMA2, want_grad=False)
    p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, N_MINOR, 2, 2, m)
    p.set_inputs(X)
    p.set_targets(Y[:, 0])
    p.set_timing(2)
    ev = p.eval(log_sf2=0.0, sigma2=SIGMA2, inducing=Zbad, jitter=-1e-3, log_hetero_skedasticity=het)
    assert _taken(set(p.last_timings())) == _path_of(m)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L) and np.all(np.isfinite(ev.grad))


@gpu
@pytest.mark.parametrize("m,orders", [(50, (17,)), (200, (129,)), (300, (257,))], ids=["small", "mid", "engine"])
def test_exact_copies_factorise_with_the_reference_jitter(m, orders):
    Zbad = minor_inducing(m, orders)
    X, Y, _, _ = _minor_data(m)
    ref = O.evaluate(KERNEL_MINOR, Zbad, X, Y[:, 0], SIGMA2, want_grad=False)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N_MINOR, 2, 2, m)
    p.set_inputs(X)
    p.set_targets(Y[:, 0])
    p.set_timing(2)
    ev = p.eval(inducing=Zbad, **HYP_MINOR)
    assert _taken(set(p.last_timings())) == _path_of(m)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L) and np.all(np.isfinite(ev.grad)) and np.all(np.isfinite(ev.coeffs))


@gpu
@pytest.mark.parametrize("nt,j", [(150, 130), (300, 257)])
def test_cov_samples_names_lapacks_order(nt, j):
    """cov = I with entry (j, j) = -1: the separate factorisation of gprhip_cov_samples fails at order j + 1, in the second /
    third 128-block (-np.eye in test_stats_covariances_and_samplers only proves order 1)."""
    cov = np.eye(nt)
    cov[j, j] = -1.0
    _, info = lapack.dpotrf(cov + gpr_amd.problem.CHOLESKY_JITTER * np.eye(nt), lower=0)
    assert info == j + 1
    X, Y, _, Zg = _minor_data(4)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N_MINOR, 2, 2, 4)
    z = np.random.default_rng(1).normal(size=(nt, 2))
    with pytest.raises(gpr_amd.NotPositiveDefinite) as e:
        p.cov_samples(cov, np.zeros(nt), z)
    assert ("leading minor of order %d " % info) in str(e.value), str(e.value)
    S = p.cov_samples(np.eye(nt), np.zeros(nt), z)      # the problem is still usable
    p.close()
    assert np.max(np.abs(S - np.sqrt(1.0 + gpr_amd.problem.CHOLESKY_JITTER) * z)) <= 1e-14 * np.max(np.abs(z))
