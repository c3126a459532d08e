"""Several target vectors on one model in one evaluation (gprhip_set_targets_many / gprhip_eval_targets /
gprhip_predict_targets, Problem.eval_targets, Deriv.Trained.calc_many, optim.train with an n x k target matrix) against
the CPU oracle run once per column.

Tolerances are those of tests/test_gpu_parity.py, restated.  The bound on the summed gradient is derived, not tuned: the
error of a sum is at most the sum of the errors, each within TOL_GRAD of its own family's largest entry, so a family of the
summed gradient is measured against the SUM over the targets of that family's largest entry -- dividing by the largest
entry of the sum would let cancellation between targets eat the margin.  No conditioning allowance: the shapes are the
well-conditioned ones of smoke() (Z = perturbed inputs, log_ell = 1/2 log d, sigma2 = 0.1).

Covered, beside the four small shapes at K = 1, 2, 5, 16:
  - every column-count template KT in {1, 2, 4, 8, 16} of targets.hip with k = KT and with k < KT (K = 3, 4, 8, 9);
  - the sizes the path was built for, against oracle.evaluate_fast_many (one model, every column): n = 40037, m = 2048 (several
    64-row slabs per tg_vty workgroup, a ragged last slab, 16 column tiles) and n = 20011, m = 1100 in three row chunks with a
    ragged last one (9 column tiles, m no multiple of 128), Cov_se_iso and Cov_se_fat with a projection / with heteroskedastic
    noise too, standard and variational, gprhip_predict_targets over more test points than a chunk.  The shapes are admitted by
    the condition number of the oracle's own K_m + jitter I, not by the library's estimate;
  - replacing the target matrix by one of another width (bit-identical to a fresh problem), gprhip_predict_targets after a
    replacement of the same / of another width, a host matrix with ld > n (and ld < n refused);
  - gprhip_eval_targets at the degenerate and tile-edge shapes of tests/test_gpu_parity.py;
  - n = 1 000 000, m = 2048, K = 3: consistency with the single-target path (62-slab tg_vty blocks, eight row chunks).
"""
import functools

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib, cov_se_fat, cov_se_iso, fitc_gp
from oracle import fitc_oracle as O
from tests import margins as M
from tests.util import load_golden, synth

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


def _target_columns(X, rng, kmax=KMAX):
    """n x kmax: different functions of the inputs at different noise levels"""
    d, n = X.shape
    s = X.sum(0)
    cols = []
    for k in range(kmax):
        f = np.sin((0.4 + 0.15 * k) * s + 0.7 * k) + (0.3 * k / KMAX) * np.cos(X[k % d] * (1.0 + 0.1 * k)) + 0.05 * k
        cols.append(f + (0.03 + 0.02 * k) * rng.normal(size=n))
    return np.asfortranarray(np.stack(cols, axis=1))


@functools.lru_cache(maxsize=None)
def _data(si, kind):
    """Inputs, inducing points, a 16-column target matrix (different functions of the inputs, different noise levels), the
    keyword arguments of Problem.eval and the oracle's kernel."""
    n, m, d, _ = SHAPES[si]
    rng = np.random.default_rng(100 + si)
    X = np.asfortranarray(rng.normal(size=(d, n)))
    Y = _target_columns(X, rng)
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
    return _check_against(refs, _problem(si, kind), Y, Z, args, fams, K, variational, "%s %s" % (SHAPES[si], kind))


def _check_against(refs, p, Y, Z, args, fams, K, variational, label):
    """p: a problem with its inputs set (closed here).  Returns the achieved errors."""
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
    print("targets %s K=%d %s: l1 %.1e  l %.1e  coeffs %.1e  dl_dsigma2_sum %.1e  grad_sum %s  cond %.1e" % (
        label, K, "variational" if variational else "standard", err_l1, max(err_l), max(err_c), err_ds2,
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
    return dict(l=max(err_l), coeffs=max(err_c), dl_dsigma2_sum=err_ds2, grad_sum=errs)


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


# ---- the sizes the several-target path was built for -------------------------------------------------------------------------
# (kind, n, m, d, chunk_rows, K).  Data: the generator of test_parity_at_headline_inducing_count / test_mid_size_against_oracle
# (synth(2, n, m, d), log_ell = 1/2 log d, sigma2 = 0.1), which hold the single-target bounds with no conditioning allowance.
#
# What each shape makes the kernels of targets.hip do (targets_vty_rows_per_block(rows) = max(64, round_up(ceil(rows / 256), 64));
# pass 1 runs tg_vty_kernel over the whole V store, rows = n):
#   n = 40037, m = 2048, one chunk of 40064 rows (the default chunk is 131072): ceil(40037 / 256) = 157 -> 192 rows per block,
#     209 blocks, three 64-row slabs per block; the last block holds 40037 - 208 * 192 = 101 rows = 64 + 37 (a ragged last
#     slab).  mp = 2048: 16 column tiles -- tg_rows_kernel<KT, true> starts its walk at j0 = 0 .. 1984, tg_vty_kernel<KT, true>
#     clips at 128 .. 2048, tg_w_rankk / tg_xcorr run 8 blocks of 256 columns.  K = 5: a KT = 8 launch with k < 8 (nine columns
#     were run first, to the same bounds; with them the oracle work of this case alone took these tests past a quarter of the
#     rest of the GPU suite's time, and a column adds no path here that five do not take).
#   n = 20011, m = 1100 in chunks of 8192 rows: 8192 + 8192 + 3627 rows (3627 = 28 * 128 + 43); ceil(20011 / 256) = 79 -> 128
#     rows per block, 157 blocks, two slabs per block; the last block holds 20011 - 156 * 128 = 43 rows (one ragged slab).
#     mp = 1152 = 9 tiles (odd; m is no multiple of 128: 52 padded columns), 4.5 blocks of 256 columns.  The es row sums and
#     the X corrections are applied per chunk at base = 0, 8192, 16384.
# Admission: cond(K_m + jitter I) by numpy.linalg.eigvalsh of the ORACLE's matrix (spec_calc_shared_upper + CHOLESKY_JITTER),
# computed on the CPU, must not exceed that of synth(2, 40000, 2048, 8), 7.74e8, where the single-target test holds TOL_GRAD raw:
#   iso 40037 x 2048: 6.65e8     iso 20011 x 1100: 1.30e8     fat_proj 20011 x 1100: 1.18e8     fat_proj_het 20011 x 1100: 6.86e4
# (test_large_shapes_are_no_worse_conditioned_than_the_single_target_parity_shape recomputes them.)
LARGE = [("iso", 40037, 2048, 8, 0, 5), ("iso", 20011, 1100, 8, 8192, 16), ("fat_proj", 20011, 1100, 8, 8192, 3),
         ("fat_proj_het", 20011, 1100, 8, 8192, 3)]
LARGE_IDS = ["%s_n%d_m%d_c%d_K%d" % (c[0], c[1], c[2], c[4], c[5]) for c in LARGE]
COND_ADMIT_SHAPE = (40000, 2048, 8)


def test_vty_figures_of_the_large_shapes():
    """The figures in the comment above, from the formula of targets_vty_rows_per_block."""
    def vty(rows):
        ceil = lambda a, b: -(-a // b)
        rpb = max(64, ceil(ceil(rows, 256), 64) * 64)
        nblk = ceil(rows, rpb)
        last = rows - (nblk - 1) * rpb
        return rpb, nblk, rpb // 64, last
    assert vty(3000) == (64, 47, 1, 56) and vty(16384)[0] == 64          # every earlier shape: one slab per block
    assert vty(40037) == (192, 209, 3, 101) and 101 % 64 == 37
    assert vty(20011) == (128, 157, 2, 43)
    assert vty(1_000_000) == (3968, 253, 62, 64)
    assert [min(8192, 20011 - b) for b in range(0, 20011, 8192)] == [8192, 8192, 3627]
    assert -(-1100 // 128) * 128 == 1152 and 1152 // 128 == 9
    assert -(-1_000_000 // 131072) == 8


@functools.lru_cache(maxsize=None)
def _large_data(li):
    kind, n, m, d, _, _ = LARGE[li]
    X, _, Zs = synth(2, n, m, d)
    Y = _target_columns(X, np.random.default_rng(300 + li))
    if kind == "iso":
        le = 0.5 * np.log(d)
        return X, Y, Zs, dict(log_ell=le, log_sf2=0.0), O.SeIsoKernel(le, 0.0), M.families("iso", d, m)
    # the fat_proj / fat_proj_het constructions of _data: a perturbed identity / sqrt(d), so that the kernel between projected
    # points is the Cov_se_iso one above; the inducing points are the projected ones of the generator
    tp = (np.eye(d) + 0.1 * np.random.default_rng(7).uniform(-1.0, 1.0, size=(d, d))) / np.sqrt(d)
    prm = cov_se_fat.Params.create(d, 0.0, tproj=tp, log_hetero_skedasticity=np.full(m, -5.0) if kind == "fat_proj_het" else None)
    kernel = cov_se_fat.Kernel.create(prm)
    Z = np.asfortranarray(cov_se_fat.project(kernel, Zs))
    args = {k: v for k, v in cov_se_fat.eval_args(kernel).items() if k != "log_ell"}
    ok = O.SeFatKernel(prm.d, prm.log_sf2, prm.tproj, prm.log_hetero_skedasticity, prm.log_multiscales_m05)
    fams = M.families("fat", prm.d, m, D=d, proj=True, het=prm.log_hetero_skedasticity is not None, ms=False)
    return X, Y, Z, args, ok, fams


@functools.lru_cache(maxsize=None)
def _large_oracle(li, variational):
    """One model, every column of the case: shared by the parametrisations below."""
    X, Y, Z, _, ok, _ = _large_data(li)
    return O.evaluate_fast_many(ok, Z, X, Y[:, :LARGE[li][5]], SIGMA2, variational=variational)


def _large_problem(li):
    kind, n, m, d, chunk, _ = LARGE[li]
    X, _, Z, _, _, _ = _large_data(li)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT, n, d, Z.shape[0], m, chunk_rows=chunk)
    p.set_inputs(X)
    return p


def _oracle_cond(ok, Z):
    """cond_2(K_m + jitter I) of the matrix the oracle factorises"""
    km, _ = O.spec_calc_shared_upper(ok, np.asfortranarray(Z))
    km = np.triu(np.nan_to_num(km, nan=0.0))
    w = np.linalg.eigvalsh(km + np.triu(km, 1).T + O.CHOLESKY_JITTER * np.eye(km.shape[0]))
    return float(w[-1] / w[0])


def test_large_shapes_are_no_worse_conditioned_than_the_single_target_parity_shape():
    n, m, d = COND_ADMIT_SHAPE
    _, _, Z0 = synth(2, n, m, d)
    bar = _oracle_cond(O.SeIsoKernel(0.5 * np.log(d), 0.0), Z0)
    conds = [_oracle_cond(_large_data(li)[4], _large_data(li)[2]) for li in range(len(LARGE))]
    print("cond(K_m + jitter): admission bar %.3e; %s" % (bar, dict(zip(LARGE_IDS, ["%.3e" % c for c in conds]))))
    assert all(c <= bar for c in conds), (bar, conds)


@pytest.mark.parametrize("variational", [False, True], ids=["standard", "variational"])
@pytest.mark.parametrize("li", range(len(LARGE)), ids=LARGE_IDS)
def test_large_shapes_against_the_oracle_per_column(li, variational):
    """Multi-slab tg_vty blocks with a ragged last slab, 9 and 16 column tiles, three row chunks with a ragged last one in the
    engine regime: the checks of test_targets_against_the_oracle_per_column, the same bounds, no conditioning allowance."""
    _, Y, Z, args, _, fams = _large_data(li)
    _check_against(_large_oracle(li, variational), _large_problem(li), Y, Z, args, fams, LARGE[li][5], variational, LARGE_IDS[li])


@pytest.mark.parametrize("li", [1, 3], ids=[LARGE_IDS[1], LARGE_IDS[3]])
def test_predict_targets_at_the_chunked_large_shapes(li):
    X, Y, Z, args, ok, _ = _large_data(li)
    K = LARGE[li][5]
    nt = 8192 + 1500   # (more test points than one 8192-row chunk)
    Xt = np.asfortranarray(np.random.default_rng(6).normal(size=(X.shape[0], nt)))
    refs = _large_oracle(li, False)
    p = _large_problem(li)
    p.set_targets_many(Y[:, :K])
    p.eval_targets(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
    means = p.predict_targets(Xt)
    p.close()
    assert means.shape == (nt, K)
    for c in range(K):
        M.check_vec("pred_mean[%d]" % c, means[:, c], O.predict_means(ok, Z, refs[c]["coeffs"], Xt), TOL_POST)


# ---- column counts: every template width KT in {1, 2, 4, 8, 16} with k = KT and with k < KT ------------------------------------
@pytest.mark.parametrize("K", [3, 4, 8, 9])
@pytest.mark.parametrize("si", [2, 3], ids=["engine", "chunks"])
def test_every_column_count_template_against_the_oracle(si, K):
    """tg_kt: 3 -> KT = 4 (k < KT), 4 -> 4, 8 -> 8, 9 -> 16 (k < KT); with K = 1, 2, 5, 16 above: 1, 2, 8 (k < KT), 16."""
    _check_against_the_oracle(si, K, "iso", False)


# ---- replacing the target matrix ---------------------------------------------------------------------------------------------
def _identical(a, b):
    return (a.l1 == b.l1 and np.array_equal(a.l2, b.l2) and a.l_sum == b.l_sum and a.dl_dsigma2_sum == b.dl_dsigma2_sum
            and np.array_equal(a.grad_sum, b.grad_sum) and np.array_equal(a.coeffs, b.coeffs))


def _assert_parity(ev, refs, fams):
    K = len(refs)
    assert ev.l.shape == (K,) and ev.coeffs.shape[1] == K
    for c in range(K):
        assert M.rel_ok("l[%d]" % c, ev.l[c], refs[c]["l"], TOL_L)
        M.check_vec("coeffs[%d]" % c, ev.coeffs[:, c], refs[c]["coeffs"], TOL_COEFF)
    ds2_ref = sum(r["dl_dsigma2"] for r in refs)
    assert abs(ev.dl_dsigma2_sum - ds2_ref) <= TOL_DS2 * abs(ds2_ref)
    errs = _summed_family_errors(ev.grad_sum, refs, fams)
    assert all(v <= TOL_GRAD for v in errs.values()), errs


@pytest.mark.parametrize("si", [2, 3], ids=["engine", "chunks"])
def test_replacing_the_target_matrix_by_one_of_another_width(si):
    """gprhip_set_targets_many with another k frees and re-makes the five target buffers: 5 -> 2 -> 16 columns (and other
    columns each time).  Every evaluation is the oracle's, and bit for bit that of a problem that never held another matrix."""
    X, Y, Z, args, _, fams = _data(si, "iso")
    p = _problem(si, "iso")
    for cols in (slice(0, 5), slice(7, 9), slice(0, 16)):
        p.set_targets_many(Y[:, cols])
        ev = p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
        _assert_parity(ev, [_oracle(si, "iso", False, c) for c in range(KMAX)[cols]], fams)
        if cols.start != 0 or cols.stop != 5:
            q = _problem(si, "iso")
            q.set_targets_many(Y[:, cols])
            assert _identical(ev, q.eval_targets(sigma2=SIGMA2, inducing=Z, **args))
            q.close()
    p.close()


@pytest.mark.parametrize("si", [2, 3], ids=["engine", "chunks"])
def test_predict_targets_after_the_target_matrix_was_replaced(si):
    """include/gprhip.h: a matrix of the SAME width keeps the coefficients of the last evaluation for gprhip_predict_targets
    (they are those of the earlier columns); one of another width discards them -- GPRHIP_ESTATE, not an nt x k' matrix of
    zeros -- and the single-target state stays as invalid as it was."""
    K = 5
    X, Y, Z, args, ok, _ = _data(si, "iso")
    nt = 1500
    Xt = np.asfortranarray(np.random.default_rng(8).normal(size=(X.shape[0], nt)))
    p = _problem(si, "iso")
    p.set_targets_many(Y[:, :K])
    p.eval_targets(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
    # same width: the means of the evaluated coefficients
    p.set_targets_many(Y[:, K:2 * K])
    means = p.predict_targets(Xt)
    assert means.shape == (nt, K)
    for c in range(K):
        M.check_vec("pred_mean[%d]" % c, means[:, c], O.predict_means(ok, Z, _oracle(si, "iso", False, c)["coeffs"], Xt), TOL_POST)
    # another width: refused by name; gprhip_predict means and gprhip_train_stats still refuse, variances still answer
    p.set_targets_many(Y[:, :2])
    with pytest.raises(_lib.GprHipError) as e:
        p.predict_targets(Xt)
    assert e.value.status == _lib.ESTATE and "gprhip_eval_targets" in str(e.value)
    with pytest.raises(_lib.GprHipError) as e:
        p.predict(Xt)
    assert e.value.status == _lib.ESTATE and "gprhip_eval_targets" in str(e.value)
    with pytest.raises(_lib.GprHipError) as e:
        p.train_stats()
    assert e.value.status == _lib.ESTATE
    model = O.evaluate(ok, Z, X, Y[:, 0], SIGMA2, want_grad=False, keep=True)["model"]
    var = np.empty(nt)
    _lib.check(p._lib.gprhip_predict(p._handle(), Xt.ctypes.data_as(_lib._dp), Xt.shape[0], nt, 0, None,
                                     var.ctypes.data_as(_lib._dp)))
    M.check_vec("pred_var", var, O.predict_variances(ok, Z, model, Xt, predictive=False), TOL_POST)
    # the next evaluation and prediction are those of the two columns
    ev = p.eval_targets(sigma2=SIGMA2, inducing=Z, want_grad=False, **args)
    means = p.predict_targets(Xt)
    assert means.shape == (nt, 2)
    for c in range(2):
        ref = _oracle(si, "iso", False, c)
        assert M.rel_ok("l[%d]" % c, ev.l[c], ref["l"], TOL_L)
        M.check_vec("pred_mean[%d]" % c, means[:, c], O.predict_means(ok, Z, ref["coeffs"], Xt), TOL_POST)
    p.close()


@pytest.mark.parametrize("si", [2, 3], ids=["engine", "chunks"])
def test_host_matrix_with_a_leading_dimension_above_n(si):
    """gprhip_set_targets_many with ld = n + 7 (Problem.set_targets_many always passes ld = n): the rows beyond n are NaN and
    must not be read; ld < n is refused."""
    K = 5
    X, Y, Z, args, _, _ = _data(si, "iso")
    n = X.shape[1]
    wide = np.full((n + 7, K), np.nan, order="F")
    wide[:n] = Y[:, :K]
    p = _problem(si, "iso")
    _lib.check(p._lib.gprhip_set_targets_many(p._handle(), wide.ctypes.data_as(_lib._dp), n + 7, K))
    a = p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
    assert np.all(np.isfinite(a.l)) and np.all(np.isfinite(a.grad_sum)) and np.all(np.isfinite(a.coeffs))
    q = _problem(si, "iso")
    q.set_targets_many(Y[:, :K])
    assert _identical(a, q.eval_targets(sigma2=SIGMA2, inducing=Z, **args))
    q.close()
    assert p._lib.gprhip_set_targets_many(p._handle(), wide.ctypes.data_as(_lib._dp), n - 1, K) == _lib.EBADARG
    assert _identical(a, p.eval_targets(sigma2=SIGMA2, inducing=Z, **args))     # the refused call changed nothing
    p.close()


# ---- degenerate and tile-edge shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (3, 3, 2), (2, 5, 3), (129, 128, 4), (128, 129, 1)])
def test_degenerate_and_tile_edge_sizes_with_several_targets(n, m, d, K):
    """The shapes, data and bounds of tests/test_gpu_parity.py::test_degenerate_and_tile_edge_sizes (its y is column 0).  That
    test gives the gradient the conditioning allowance of tests/margins.py (m > n, points on a line: K_m is jitter-dominated);
    here the condition number is that of the oracle's K_m + jitter I by numpy.linalg.eigvalsh, not the library's estimate.
    For the summed gradient the allowance and the family scale are summed over the columns, as the errors are."""
    rng = np.random.default_rng(n * 1000 + m)
    X = np.asfortranarray(rng.normal(size=(d, n)))
    y = rng.normal(size=n)
    Z = np.asfortranarray(rng.normal(size=(d, m)))
    Y = np.asfortranarray(np.concatenate([y[:, None], rng.normal(size=(n, K - 1))], axis=1))
    ok = O.SeIsoKernel(0.2, -0.3)
    refs = [O.evaluate(ok, Z, X, Y[:, c], 0.5) for c in range(K)]
    allow = M.ALLOW_FACTOR * _oracle_cond(ok, Z) * M.EPS64
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets_many(Y)
    ev = p.eval_targets(log_ell=0.2, log_sf2=-0.3, sigma2=0.5, inducing=Z)
    p.close()
    for c in range(K):
        assert M.rel_ok("l[%d]" % c, ev.l[c], refs[c]["l"], TOL_L)
    assert M.rel_ok("l_sum", ev.l_sum, sum(r["l"] for r in refs), TOL_L)
    total = np.sum([r["grad"] for r in refs], axis=0)
    wholes = [max(float(np.max(np.abs(r["grad"]))), 1e-300) for r in refs]
    errs = {}
    for name, sl in M.families("iso", d, m):
        scales = [float(np.max(np.abs(r["grad"][sl]))) for r in refs]
        scale = sum(s if s >= 1e-12 * w else w for s, w in zip(scales, wholes))      # (as margins.family_errors)
        errs[name] = max(0.0, float(np.max(np.abs(ev.grad_sum[sl] - total[sl]))) - allow * sum(wholes)) / scale
    assert all(v <= TOL_GRAD for v in errs.values()), errs
    ds2 = sum(r["dl_dsigma2"] for r in refs)
    assert abs(ev.dl_dsigma2_sum - ds2) <= TOL_DS2 * sum(max(abs(r["dl_dsigma2"]), 1e-3) for r in refs)
    assert np.all(np.isfinite(ev.coeffs))


# ---- the headline shape: consistency with the single-target path, not parity ---------------------------------------------------
def test_headline_size_consistency_with_the_single_target_path():
    """n = 1 000 000, m = 2048, d = 8, three target columns, default chunking: 253 tg_vty blocks of 3968 rows = 62 slabs each
    (the last one 64 rows), eight row chunks of 131072 rows (the last one 82496).  No oracle at this size: the single-target
    evaluation is the yardstick -- itself pinned here by test_headline_size_properties and against the oracle at n = 40 000."""
    n, m, d, K = 1_000_000, 2048, 8, 3
    X, _, Z = synth(2, n, m, d)
    Y = _target_columns(X, np.random.default_rng(400), kmax=K)
    le = 0.5 * np.log(d)
    hyp = dict(log_ell=le, log_sf2=0.0, sigma2=SIGMA2, inducing=Z)
    fams = M.families("iso", d, m)
    Xt = np.asfortranarray(np.random.default_rng(9).normal(size=(d, 3000)))
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets_many(Y)
    a = p.eval_targets(**hyp)
    b = p.eval_targets(**hyp)
    assert _identical(a, b)
    assert np.all(np.isfinite(a.l)) and np.isfinite(a.dl_dsigma2_sum) and np.all(np.isfinite(a.grad_sum))
    assert np.all(np.isfinite(a.coeffs))
    means = p.predict_targets(Xt)
    assert means.shape == (3000, K) and np.all(np.isfinite(means))
    l0 = p.eval_targets(want_grad=False, **hyp).l
    for c in range(K):
        assert M.rel_ok("l[%d] evidence only" % c, l0[c], a.l[c], 1e-12)
    singles = []
    for c in range(K):
        p.set_targets(Y[:, c])
        e = p.eval(**hyp)
        m1, _ = p.predict(Xt, want_variances=False)
        assert M.rel_ok("l[%d]" % c, a.l[c], e.l, TOL_L)
        M.check_vec("coeffs[%d]" % c, a.coeffs[:, c], e.coeffs, TOL_COEFF)
        M.check_vec("pred_mean[%d]" % c, means[:, c], m1, TOL_POST)
        singles.append(dict(grad=e.grad, dl_dsigma2=e.dl_dsigma2))
    p.close()
    errs = _summed_family_errors(a.grad_sum, singles, fams)
    ds2 = sum(s["dl_dsigma2"] for s in singles)
    err_ds2 = abs(a.dl_dsigma2_sum - ds2) / sum(abs(s["dl_dsigma2"]) for s in singles)
    print("headline consistency K=%d: dl_dsigma2_sum %.1e  grad_sum %s" % (K, err_ds2, {k: "%.1e" % v for k, v in errs.items()}))
    assert all(v <= TOL_GRAD for v in errs.values()), errs
    assert err_ds2 <= TOL_DS2
