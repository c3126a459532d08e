"""Several target vectors on one model in one evaluation (gprhip_set_targets_many / gprhip_eval_targets /
gprhip_predict_targets, Problem.eval_targets, Deriv.Trained.calc_many, optim.train with an n x k target matrix) against
the CPU oracle run once per column.

Tolerances are those of tests/test_gpu_parity.py, restated.  The bound on the summed gradient is derived, not tuned: the
error of a sum is at most the sum of the errors, each within TOL_GRAD of its own family's largest entry, so a family of the
summed gradient is measured against the SUM over the targets of that family's largest entry -- dividing by the largest
entry of the sum would let cancellation between targets eat the margin.  No conditioning allowance: the shapes are the
well-conditioned ones of smoke() (Z = perturbed inputs, log_ell = 1/2 log d, sigma2 = 0.1).
"""
import functools

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib, cov_se_fat, cov_se_iso, fitc_gp
from oracle import fitc_oracle as O
from tests import margins as M
from tests.util import load_golden

pytestmark = pytest.mark.gpu

TOL_L = 7e-10       # as tests/test_gpu_parity.py
TOL_DS2 = 4e-10
TOL_GRAD = 1e-8
TOL_COEFF = 1e-7
TOL_POST = 3e-10

KMAX = 16
# (n, m, d, chunk_rows): the small, mid and engine regimes of smoke(), and smoke()'s first shape again in four row chunks
# (640 + 640 + 640 + 80 rows; 2000 is not a multiple of 128).  The chunked case has to be one of smoke()'s shapes because the
# bounds here carry no conditioning allowance: a denser choice tried first, (1111, 200, 3) in chunks of 384, has
# cond(K_m + jitter) = 1e8 by the library's own estimate -- the allowance of tests/margins.py would be 9e-8 there -- and the
# inducing family of its summed gradient measured 1.3e-8 at K = 1 and 2 (7e-9 at K = 5, 8e-10 at K = 16: the model part, whose
# share of the scale shrinks as targets are added), every other figure of it within its bound.
SHAPES = [(2000, 50, 3, 0), (3000, 150, 4, 0), (3000, 300, 4, 0), (2000, 50, 3, 640)]
SIGMA2 = 0.1


@functools.lru_cache(maxsize=None)
def _data(si, kind):
    """Inputs, inducing points, a 16-column target matrix (different functions of the inputs, different noise levels), the
    keyword arguments of Problem.eval and the oracle's kernel."""
    n, m, d, _ = SHAPES[si]
    rng = np.random.default_rng(100 + si)
    X = np.asfortranarray(rng.normal(size=(d, n)))
    s = X.sum(0)
    cols = []
    for k in range(KMAX):
        f = np.sin((0.4 + 0.15 * k) * s + 0.7 * k) + (0.3 * k / KMAX) * np.cos(X[k % d] * (1.0 + 0.1 * k)) + 0.05 * k
        cols.append(f + (0.03 + 0.02 * k) * rng.normal(size=n))
    Y = np.asfortranarray(np.stack(cols, axis=1))
    pick = rng.permutation(n)[:m]
    if kind == "iso":
        Z = np.asfortranarray(X[:, pick] + 0.01 * rng.normal(size=(d, m)))
        le = 0.5 * np.log(d)
        args = dict(log_ell=le, log_sf2=0.0)
        ok = O.SeIsoKernel(le, 0.0)
        fams = M.families("iso", d, m)
    else:
        if kind == "fat":
            # projection + heteroskedastic noise + multiscales, as create_default_kernel_params makes them
            prm = cov_se_fat.create_default_kernel_params(X, m, rng=np.random.default_rng(7 + si))
        else:
            # projection alone ("fat_proj": the row sums of E = X .* K that feed the `Proj gradient come from the row kernels,
            # and K_nm is kept from pass 1 for the matrix-core gradient kernel), or with heteroskedastic noise ("fat_proj_het").
            # The projection is a perturbed identity / sqrt(d), so that the kernel between projected points is the
            # Cov_se_iso one of the other cases (log_ell = 1/2 log d): same geometry, same conditioning.
            tp = (np.eye(d) + 0.1 * np.random.default_rng(7 + si).uniform(-1.0, 1.0, size=(d, d))) / np.sqrt(d)
            prm = cov_se_fat.Params.create(d, 0.0, tproj=tp, log_hetero_skedasticity=np.full(m, -5.0) if kind == "fat_proj_het" else None)
        kernel = cov_se_fat.Kernel.create(prm)
        Z = np.asfortranarray(cov_se_fat.project(kernel, X[:, pick]) + 0.01 * rng.normal(size=(prm.d, m)))
        args = {k: v for k, v in cov_se_fat.eval_args(kernel).items() if k != "log_ell"}
        ok = O.SeFatKernel(prm.d, prm.log_sf2, prm.tproj, prm.log_hetero_skedasticity, prm.log_multiscales_m05)
        fams = M.families("fat", prm.d, m, D=d, proj=True, het=prm.log_hetero_skedasticity is not None,
                          ms=prm.log_multiscales_m05 is not None)
    return X, Y, Z, args, ok, fams


@functools.lru_cache(maxsize=None)
def _oracle(si, kind, variational, col):
    X, Y, Z, _, ok, _ = _data(si, kind)
    return O.evaluate_fast(ok, Z, X, Y[:, col], SIGMA2, variational=variational)


def _problem(si, kind):
    n, m, d, chunk = SHAPES[si]
    X, _, Z, _, _, _ = _data(si, kind)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT, n, d, Z.shape[0], m, chunk_rows=chunk)
    p.set_inputs(X)
    return p


def _summed_family_errors(got, refs, fams):
    """{family: max-abs error against sum_k grad_k, divided by sum_k max|family of grad_k|}"""
    total = np.sum([r["grad"] for r in refs], axis=0)
    out = {}
    for name, sl in fams:
        scale = sum(float(np.max(np.abs(r["grad"][sl]))) for r in refs)
        out[name] = float(np.max(np.abs(got[sl] - total[sl]))) / max(scale, 1e-300)
    return out


@pytest.mark.parametrize("variational", [False, True], ids=["standard", "variational"])
@pytest.mark.parametrize("kind", ["iso", "fat"])
@pytest.mark.parametrize("K", [1, 2, 5, 16])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=["n%d_m%d_c%d" % (s[0], s[1], s[3]) for s in SHAPES])
def test_targets_against_the_oracle_per_column(si, K, kind, variational):
    _check_against_the_oracle(si, K, kind, variational)


@pytest.mark.parametrize("variational", [False, True], ids=["standard", "variational"])
@pytest.mark.parametrize("kind", ["fat_proj", "fat_proj_het"])
@pytest.mark.parametrize("si", [2, 3], ids=["engine", "chunks"])
def test_fat_options_one_at_a_time_against_the_oracle(si, kind, variational):
    """Cov_se_fat with a projection and no multiscales takes other branches of the row path than the all-options kernel
    above: the second term of the `Proj gradient comes from the per-row sums es = q - v (sf2 - r) - mean_k w_k (Q' b_k) of the
    row kernels (with multiscales the gradient kernel rebuilds them from X), and the matrix-core gradient kernel reads the
    K_nm kept from pass 1."""
    _check_against_the_oracle(si, 5, kind, variational)


def _check_against_the_oracle(si, K, kind, variational):
    X, Y, Z, args, _, fams = _data(si, kind)
    refs = [_oracle(si, kind, variational, c) for c in range(K)]
    p = _problem(si, kind)
    p.set_targets_many(Y[:, :K])
    p.set_timing(2)
    ev = p.eval_targets(sigma2=SIGMA2, inducing=Z, variational=variational, **args)
    stages = p.last_timings()
    assert "p1_trmm_V" in stages and "p1_targets" in stages and "p2_targets" in stages and "p2_xcorr" in stages, stages
    assert ev.l.shape == (K,) and ev.coeffs.shape == (Z.shape[1], K)
    err_l1 = abs(ev.l1 - refs[0]["l1"]) / abs(refs[0]["l1"])
    err_l = [abs(ev.l[c] - refs[c]["l"]) / abs(refs[c]["l"]) for c in range(K)]
    err_c = [M.relinf(ev.coeffs[:, c], refs[c]["coeffs"]) for c in range(K)]
    ds2_ref = sum(r["dl_dsigma2"] for r in refs)
    err_ds2 = abs(ev.dl_dsigma2_sum - ds2_ref) / abs(ds2_ref)
    errs = _summed_family_errors(ev.grad_sum, refs, fams)
    print("targets %s K=%d %s %s: l1 %.1e  l %.1e  coeffs %.1e  dl_dsigma2_sum %.1e  grad_sum %s  cond %.1e" % (
        SHAPES[si], K, kind, "variational" if variational else "standard", err_l1, max(err_l), max(err_c), err_ds2,
        {k: "%.1e" % v for k, v in errs.items()}, p.condition()[0]))
    assert err_l1 <= TOL_L
    assert max(err_l) <= TOL_L, err_l
    assert abs(ev.l_sum - sum(r["l"] for r in refs)) <= TOL_L * abs(sum(r["l"] for r in refs))
    for c in range(K):
        M.check_vec("coeffs[%d]" % c, ev.coeffs[:, c], refs[c]["coeffs"], TOL_COEFF)
    assert err_ds2 <= TOL_DS2
    assert ev.grad_sum.shape == refs[0]["grad"].shape
    bad = {k: v for k, v in errs.items() if not v <= TOL_GRAD}
    assert not bad, "summed gradient: families beyond %.1e: %s (all: %s)" % (TOL_GRAD, bad, errs)
    # evidence only
    ev0 = p.eval_targets(sigma2=SIGMA2, inducing=Z, variational=variational, want_grad=False, **args)
    assert ev0.grad_sum is None and max(abs(ev0.l[c] - refs[c]["l"]) / abs(refs[c]["l"]) for c in range(K)) <= TOL_L
    p.close()


@pytest.mark.parametrize("si", [0, 2, 3], ids=["small", "engine", "chunks"])
def test_one_target_agrees_with_eval(si):
    X, Y, Z, args, _, fams = _data(si, "iso")
    p = _problem(si, "iso")
    p.set_targets_many(Y[:, :1])
    a = p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
    q = _problem(si, "iso")
    q.set_targets(Y[:, 0])
    b = q.eval(sigma2=SIGMA2, inducing=Z, **args)
    assert M.rel_ok("l1", a.l1, b.l1, TOL_L) and M.rel_ok("l", a.l[0], b.l, TOL_L) and M.rel_ok("l_sum", a.l_sum, b.l, TOL_L)
    assert M.rel_ok("dl_dsigma2", a.dl_dsigma2_sum, b.dl_dsigma2, TOL_DS2)
    assert M.grad_ok(a.grad_sum, b.grad, fams, TOL_GRAD)
    assert M.vec_ok("coeffs", a.coeffs[:, 0], b.coeffs, TOL_COEFF)
    p.close()
    q.close()


@pytest.mark.parametrize("kind", ["iso", "fat"])
def test_identical_columns_repeat_runs_and_sigma2_update(kind):
    si, K = 2, 5
    X, Y, Z, args, _, fams = _data(si, kind)
    p = _problem(si, kind)
    p.set_targets_many(np.repeat(Y[:, 3:4], K, axis=1))
    a = p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
    assert np.all(a.l2 == a.l2[0])                                    # bit for bit
    assert np.all(a.coeffs == a.coeffs[:, :1])
    p.set_targets(Y[:, 3])
    one = p.eval(sigma2=SIGMA2, inducing=Z, **args)
    assert M.grad_ok(a.grad_sum, K * one.grad, fams, TOL_GRAD)
    assert M.rel_ok("dl_dsigma2", a.dl_dsigma2_sum, K * one.dl_dsigma2, TOL_DS2)
    assert M.rel_ok("l2", a.l2[0], one.l2, TOL_L)
    # two runs of the same call are bit-identical
    p.set_targets_many(Y[:, :K])
    r1 = p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
    r2 = p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
    assert r1.l1 == r2.l1 and np.array_equal(r1.l2, r2.l2) and np.array_equal(r1.grad_sum, r2.grad_sum)
    assert np.array_equal(r1.coeffs, r2.coeffs) and r1.dl_dsigma2_sum == r2.dl_dsigma2_sum
    # Model.update_sigma2: only sigma2 changed -> reuse_v matches a fresh evaluation
    u = p.eval_targets(sigma2=0.25, inducing=Z, reuse_v=True, **args)
    q = _problem(si, kind)
    q.set_targets_many(Y[:, :K])
    f = q.eval_targets(sigma2=0.25, inducing=Z, **args)
    assert M.rel_ok("l1", u.l1, f.l1, TOL_L) and M.vec_ok("l", u.l, f.l, TOL_L)
    assert M.rel_ok("dl_dsigma2", u.dl_dsigma2_sum, f.dl_dsigma2_sum, TOL_DS2)
    assert M.grad_ok(u.grad_sum, f.grad_sum, fams, TOL_GRAD) and M.vec_ok("coeffs", u.coeffs, f.coeffs, TOL_COEFF)
    p.close()
    q.close()


@pytest.mark.parametrize("si", [0, 1, 2], ids=["small", "mid", "engine"])
def test_eval_after_eval_targets_is_the_fresh_evaluation(si):
    """gprhip_set_targets / gprhip_eval interleave with the new calls: the single-target evaluation afterwards is bit for bit
    that of a problem that never saw a target matrix."""
    X, Y, Z, args, _, _ = _data(si, "iso")
    p = _problem(si, "iso")
    p.set_targets(Y[:, 1])
    p.set_targets_many(Y[:, :4])
    p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
    a = p.eval(sigma2=SIGMA2, inducing=Z, **args)
    q = _problem(si, "iso")
    q.set_targets(Y[:, 1])
    b = q.eval(sigma2=SIGMA2, inducing=Z, **args)
    assert a.l1 == b.l1 and a.l2 == b.l2 and a.dl_dsigma2 == b.dl_dsigma2
    assert np.array_equal(a.grad, b.grad) and np.array_equal(a.coeffs, b.coeffs)
    p.close()
    q.close()


@pytest.mark.parametrize("kind,si", [("iso", 0), ("iso", 3), ("fat", 2)])
def test_predict_targets(kind, si):
    K = 5
    X, Y, Z, args, ok, _ = _data(si, kind)
    rng = np.random.default_rng(5)
    nt = 1500  # (more than one test chunk where the training chunk is 640 rows)
    Xt = np.asfortranarray(rng.normal(size=(X.shape[0], nt)))
    p = _problem(si, kind)
    p.set_targets_many(Y[:, :K])
    ev = p.eval_targets(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
    means = p.predict_targets(Xt)
    assert means.shape == (nt, K)
    for c in range(K):
        ref = _oracle(si, kind, False, c)
        M.check_vec("pred_mean[%d]" % c, means[:, c], O.predict_means(ok, Z, ref["coeffs"], Xt), TOL_POST)
    # the model state is valid: variances, factors, condition
    model = O.evaluate(ok, Z, X, Y[:, 0], SIGMA2, want_grad=False, keep=True)["model"]
    var = np.empty(nt)
    _lib.check(p._lib.gprhip_predict(p._handle(), Xt.ctypes.data_as(_lib._dp), Xt.shape[0], nt, 0, None,
                                     var.ctypes.data_as(_lib._dp)))
    M.check_vec("pred_var", var, O.predict_variances(ok, Z, model, Xt, predictive=False), TOL_POST)
    u, r = p.co_variance_coeffs()
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(r)) and p.condition()[0] >= 1.0
    # the single-target state is not: means and training statistics refuse, by name
    with pytest.raises(_lib.GprHipError) as e1:
        p.predict(Xt)
    assert e1.value.status == _lib.ESTATE and "gprhip_eval_targets" in str(e1.value)
    with pytest.raises(_lib.GprHipError) as e2:
        p.train_stats()
    assert e2.value.status == _lib.ESTATE
    # ... until the next gprhip_eval
    p.set_targets(Y[:, 0])
    p.eval(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
    m1, _ = p.predict(Xt)
    M.check_vec("pred_mean_single", m1, means[:, 0], TOL_POST)
    with pytest.raises(_lib.GprHipError) as e3:
        p.predict_targets(Xt)
    assert e3.value.status == _lib.ESTATE
    p.close()


def test_refused_calls_leave_the_problem_usable():
    si = 0
    X, Y, Z, args, _, _ = _data(si, "iso")
    n = X.shape[1]
    p = _problem(si, "iso")
    with pytest.raises(_lib.GprHipError) as e:
        p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)              # no target matrix yet
    assert e.value.status == _lib.ESTATE
    with pytest.raises(_lib.GprHipError) as e:
        p.set_targets_many(np.zeros((n, 0)))
    assert e.value.status == _lib.EBADARG
    with pytest.raises(_lib.GprHipError) as e:
        p.set_targets_many(np.zeros((n, 17)))
    assert e.value.status == _lib.EBADARG
    p.set_targets_many(Y[:, :3])
    with pytest.raises(_lib.GprHipError) as e:
        p.eval_targets(sigma2=SIGMA2, inducing=Z, model_only=True, **args)
    assert e.value.status == _lib.EBADARG
    f = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, X.shape[0], X.shape[0], Z.shape[1], precision=gpr_amd.F32_BULK)
    f.set_inputs(X)
    with pytest.raises(_lib.GprHipError) as e:
        f.set_targets_many(Y[:, :3])
    assert e.value.status == _lib.EBADARG
    f.close()
    ev = p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)              # a clean evaluation afterwards
    for c in range(3):
        assert M.rel_ok("l", ev.l[c], _oracle(si, "iso", False, c)["l"], TOL_L)
    p.close()


def test_training_on_three_target_columns():
    """The recipe of test_save_data_recipe_training_improves_evidence_and_fits_noise with an n x 3 target matrix: the stored y
    and two more functions of the same inputs."""
    from gpr_amd import optim
    g = load_golden("iso_gen_data")
    X, y, Z = g["X"], g["y"], g["Z"]
    rng = np.random.default_rng(11)
    x = X[0]
    Y = np.asfortranarray(np.stack([y, np.cos(2.0 * x) + 0.5 * rng.normal(size=x.shape[0]),
                                    0.3 * x + np.sin(x) + 0.9 * rng.normal(size=x.shape[0])], axis=1))
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    kernel = cov_se_iso.Kernel.create(cov_se_iso.create_default_kernel_params())
    s0 = float(np.mean(np.sum(Y * Y, axis=0))) / Y.shape[0]
    tr0 = F.Eval.Trained.calc_many(F.Eval.Model.calc(F.Eval.Inputs.calc(X, F.Deriv.Inducing.calc(kernel, Z)), sigma2=s0), Y)
    le0 = F.Eval.Trained.calc_log_evidence(tr0)
    assert F.Eval.Trained.calc_log_evidences(tr0).shape == (3,) and F.Eval.Trained.calc_mean_coeffs(tr0).shape == (Z.shape[1], 3)
    k1, z1, s2, le1, nev = optim.train(F, cov_se_iso, kernel, Z, X, Y, max_iter=60)
    print("training on 3 columns: summed log evidence %.6f -> %.6f in %d evaluations, sigma2 %.4f" % (le0, le1, nev, s2))
    assert le1 > le0
    ind1 = F.Eval.Inducing.calc(k1, z1)
    total = 0.0
    for c in range(3):
        tr = F.Eval.Trained.calc(F.Eval.Model.calc(F.Eval.Inputs.calc(X, ind1), sigma2=s2), np.ascontiguousarray(Y[:, c]))
        total += F.Eval.Trained.calc_log_evidence(tr)
    assert M.rel_ok("l_sum", le1, total, TOL_L)
    GP.close()
