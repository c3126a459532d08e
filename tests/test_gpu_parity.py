"""Parity of the HIP path (through the C ABI) with the CPU oracle and the golden fixtures.

Stated fp64 tolerances.  The device path is the whitened SYRK + potrf
formulation (B~ = I + V^T S^-1 V), whose rounding behaviour is of the same class as the reference's
Householder QR of the stacked matrix; the remaining differences are summation order and exp() ulps.
"""
import os

import numpy as np
import pytest

import gpr_amd
from gpr_amd import cov_se_fat, cov_se_iso, fitc_gp
from oracle import fitc_oracle as O
from tests import margins as M
from tests.util import (STAT_KEYS, golden_names, illcond_golden_names, load_golden, oracle_kernel, posterior_golden_names, relinf,
                        synth)

pytestmark = pytest.mark.gpu

# Stated fp64 bounds, each <= 10 x the worst error observed over the suite and the long random-shape sweeps of round 6 (5000
# gradient checks, 1500 evidence checks; table with every test's achieved errors: profiles/r06_parity_margins.txt):
TOL_L = 7e-10       # |l - l_ref| <= TOL_L * |l_ref|   (also l1)                                        worst seen 7.6e-11
TOL_DS2 = 4e-10     # dl/dsigma2, relative                                                             worst seen 4.0e-11
TOL_GRAD = 1e-8     # gradient, PER FAMILY of the reference's Hyper.get_all order (log_ell | log_sf2 | inducing | Proj |
                    # hetero | multiscale), each against its own largest entry (tests/margins.py); where the case's
                    # cond(K_m + jitter) is known, plus the conditioning allowance 8 cond 2^-53 of the largest entry
                    #                                                                                  worst seen 9.6e-10
TOL_COEFF = 1e-7    # mean coefficients t, max-abs error relative to max-abs entry                     worst seen 3.0e-8
TOL_COEFF_LINE = 3e-7   # ... for training points on a line (d = 1): K_m is jitter-dominated, see
                        # test_mean_coefficients_against_an_80_bit_evaluation                          worst seen 5.1e-8
TOL_ROW = 1e-10     # per-row intermediates r, 1/s                                                     worst seen 1.2e-11
TOL_ROWVW = 2e-10   # per-row v, w                                                                     worst seen 1.9e-11
TOL_SHARD = 2e-14   # l, dl/dsigma2 of two row partitions of one problem (summation order only)        worst seen 1.4e-15
TOL_SHARD_GRAD = 1e-9  # ... their gradient families and coefficients                                  worst seen 9.4e-11
TOL_POST = 3e-10    # posterior means / variances / training means / statistics / samples against the oracle   worst seen 3.2e-11
TOL_FACTOR = 1e-11  # exported factors chol_km, r_mat                                                   worst seen 1.2e-12
TOL_BENCH = 1e-9    # bench.py's last evaluation across launch modes (l, dl/dsigma2, |grad|; relative to max(1, |.|))


def _problem_for(g, chunk_rows=0):
    X, Z = g["X"], g["Z"]
    D, n = X.shape
    d, m = Z.shape
    kind = gpr_amd.COV_SE_ISO if g["kind"] == "iso" else gpr_amd.COV_SE_FAT
    p = gpr_amd.Problem(kind, n, D, d, m, chunk_rows=chunk_rows)
    p.set_inputs(X)
    p.set_targets(g["y"])
    return p


def _eval_golden(p, g, **kw):
    args = dict(log_sf2=float(g["log_sf2"]), sigma2=float(g["sigma2"]), inducing=g["Z"],
                variational=bool(g.get("variational", False)))
    if g["kind"] == "iso":
        args["log_ell"] = float(g["log_ell"])
    else:
        if "tproj" in g:
            args["tproj"] = g["tproj"]
        if "log_hetero" in g:
            args["log_hetero_skedasticity"] = g["log_hetero"]
        if "log_multiscales" in g:
            args["log_multiscales_m05"] = g["log_multiscales"]
    args.update(kw)
    return p.eval(**args)


def _small_path_applies(g):
    """gpr_amd/csrc/small.hip: one-kernel row passes for m <= 64, d <= 16 (8 with multiscales), D <= 64."""
    d, m = g["Z"].shape
    D = g["X"].shape[0]
    return m <= 64 and d <= (8 if "log_multiscales" in g else 16) and D <= 64


def _mid_path_applies(g):
    """gpr_amd/csrc/mid.hip: one-kernel row passes for one or two 128-column tiles of inducing points (m <= 256) that the
    small path does not take: d <= 16, 1 + d + D <= 32 with a projection, no multiscales."""
    d, m = g["Z"].shape
    D = g["X"].shape[0] if "tproj" in g else 0
    return m <= 256 and d <= 16 and 1 + d + D <= 32 and "log_multiscales" not in g


def _golden_cases(names):
    """(fixture, row-pass path).  "default" is what the library picks: small.hip for m <= 64, mid.hip for 65 .. 256, else the
    engine; fixtures the small path takes also run through mid.hip ("mid": GPRHIP_SMALL_PATH=0) where that applies, and
    every fixture a one-kernel path takes also runs through the engine ("engine": both switched off)."""
    out = []
    for n in names:
        g = load_golden(n)
        out.append(pytest.param(n, "default", id=n))
        if _small_path_applies(g) and _mid_path_applies(g):
            out.append(pytest.param(n, "mid", id=n + "-mid"))
        if _small_path_applies(g) or _mid_path_applies(g):
            out.append(pytest.param(n, "engine", id=n + "-engine"))
    return out


def _select_row_path(g, path, monkeypatch):
    if path in ("mid", "engine"):
        monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")  # read when the problem is created
    if path == "engine":
        monkeypatch.setenv("GPRHIP_MID_PATH", "0")


def _check_row_path(p, g, path):
    p.set_timing(2)
    _eval_golden(p, g)
    stages = set(p.last_timings())
    p.set_timing(0)
    if path == "default" and _small_path_applies(g):
        assert {"p1_small", "p2_small"} <= stages and "p1_trmm_V" not in stages and "p1_mid" not in stages, stages
    elif path in ("default", "mid") and _mid_path_applies(g):
        assert {"p1_mid", "p2_mid"} <= stages and "p1_trmm_V" not in stages and "p1_small" not in stages, stages
    else:
        assert "p1_trmm_V" in stages and "p1_small" not in stages and "p1_mid" not in stages, stages


ISO_GOLDEN = [n for n in golden_names() if n.startswith("iso")]


@pytest.mark.parametrize("name,path", _golden_cases(ISO_GOLDEN))
def test_golden_iso(name, path, monkeypatch):
    g = load_golden(name)
    _select_row_path(g, path, monkeypatch)
    p = _problem_for(g)
    _check_row_path(p, g, path)
    ev = _eval_golden(p, g)
    assert M.rel_ok("l1", ev.l1, g["l1"], TOL_L)
    assert M.rel_ok("l", ev.l, g["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, g["dl_dsigma2"], TOL_DS2)
    assert ev.grad.shape == g["grad"].shape
    assert M.grad_ok(ev.grad, g["grad"], M.families_golden(g), TOL_GRAD)
    assert M.vec_ok("coeffs", ev.coeffs, g["coeffs"], TOL_COEFF)
    assert M.vec_ok("row_r", p.debug_fetch("r"), g["r_vec"], TOL_ROW)
    assert M.vec_ok("row_is", p.debug_fetch("is"), g["is_vec"], TOL_ROW)
    assert M.vec_ok("row_v", p.debug_fetch("v"), g["v_vec"], TOL_ROWVW)
    assert M.vec_ok("row_w", p.debug_fetch("w"), g["w_vec"], TOL_ROWVW)
    # evidence-only entry point (multim_f) agrees with the gradient one
    ev0 = _eval_golden(p, g, want_grad=False)
    assert M.rel_ok("l", ev0.l, ev.l, 1e-12)
    # model-only gradient (Deriv.Model.prepare_hyper / calc_log_evidence)
    evm = _eval_golden(p, g, model_only=True)
    assert M.rel_ok("l", evm.l, g["l1"], TOL_L)
    assert M.rel_ok("model_dl_dsigma2", evm.dl_dsigma2, g["model_dl_dsigma2"], TOL_DS2)
    assert M.grad_ok(evm.grad, g["model_grad"], M.families_golden(g), TOL_GRAD, "model_grad")
    p.close()


FAT_GOLDEN = [n for n in golden_names() if n.startswith("fat")]


@pytest.mark.parametrize("name,path", _golden_cases(FAT_GOLDEN))
def test_golden_fat(name, path, monkeypatch):
    """Cov_se_fat (projection-only): Log_sf2, inducing and Proj hypers in lib/cov_se_fat.ml:290-342 order."""
    g = load_golden(name)
    _select_row_path(g, path, monkeypatch)
    p = _problem_for(g)
    _check_row_path(p, g, path)
    ev = _eval_golden(p, g)
    assert M.rel_ok("l", ev.l, g["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, g["dl_dsigma2"], TOL_DS2)
    assert ev.grad.shape == g["grad"].shape
    assert M.grad_ok(ev.grad, g["grad"], M.families_golden(g), TOL_GRAD)
    assert M.vec_ok("coeffs", ev.coeffs, g["coeffs"], TOL_COEFF)
    evm = _eval_golden(p, g, model_only=True)
    assert M.grad_ok(evm.grad, g["model_grad"], M.families_golden(g), TOL_GRAD, "model_grad")
    p.close()


def test_fat_functor_mirror_self_test():
    """test/test_derivatives.ml uses Cov_se_fat: finite differences for Log_sf2, an inducing coordinate
    and Proj entries through the mirrored functor (eps=1e-8, tol=1e-2 as in the reference)."""
    rng = np.random.default_rng(9)
    X = np.asfortranarray(rng.uniform(size=(3, 10)))
    y = rng.uniform(size=10)
    P = np.asfortranarray(rng.uniform(-1, 1, size=(3, 2)))
    # projection, heteroskedastic noise and multiscales all on, as create_default_kernel_params does
    # (lib/cov_se_fat.ml:191-213: log_hetero = -5, log_multiscales_m05 = 0)
    kernel = cov_se_fat.Kernel.create(cov_se_fat.Params.create(2, 0.3, P, np.full(5, -5.0), np.zeros((2, 5))))
    Z = np.asfortranarray((P.T @ X)[:, :5].copy())
    GP = fitc_gp.Make_deriv(cov_se_fat)
    FITC = GP.FITC
    hypers = FITC.Deriv.Spec.HyperModule.get_all(kernel, Z, X)
    assert len(hypers) == 1 + 2 * 5 + 3 * 2 + 5 + 2 * 5
    FITC.Deriv.Test.self_test(kernel, Z, X, sigma2=1.0, targets=y, hyper="Sigma2")
    for h in hypers:
        FITC.Deriv.Test.self_test(kernel, Z, X, sigma2=1.0, targets=y, hyper=h)
    GP.close()


def test_chunking_does_not_change_results():
    g = load_golden("iso_ragged")
    p1, p2 = _problem_for(g), _problem_for(g, chunk_rows=256)
    a, b = _eval_golden(p1, g), _eval_golden(p2, g)
    assert abs(a.l - b.l) <= TOL_SHARD * abs(a.l)
    assert M.grad_ok(a.grad, b.grad, M.families_golden(g), TOL_SHARD_GRAD)
    p1.close()
    p2.close()


def test_mid_size_against_oracle():
    n, m, d = 20000, 256, 8
    X, y, Z = synth(2, n, m, d)
    le = 0.5 * np.log(d)
    ref = O.evaluate_fast(O.SeIsoKernel(le, 0.0), Z, X, y, 0.1)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=4096)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=le, log_sf2=0.0, sigma2=0.1, inducing=Z)
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD)
    p.close()


@pytest.mark.parametrize("m", [640, 800, 1100, 2048, 3100])
def test_odd_block_counts_of_the_triangular_inverse(m):
    """m/128 = 5, 7, 9 (padded), 16, 25 (an odd k-range under split-K): exercises the ragged joins of the recursive triangular inverse, its
    split-K late levels (m >= 1024) and the tile enumeration away from powers of two."""
    n, d = max(3000, m + 500), 4
    X, y, Z = synth(17, n, m, d)
    ref = O.evaluate_fast(O.SeIsoKernel(0.7, 0.0), Z, X, y, 0.1)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=0.7, log_sf2=0.0, sigma2=0.1, inducing=Z)
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD, cond=p.condition()[0])
    assert M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)
    p.close()


# fp32-bulk mode (BASELINE.json config 3): the reference is fp64 only, so parity is "fp32 build vs
# fp64 oracle" within these stated tolerances (n x m data and contractions in fp32; everything
# m x m, the covariance evaluation and every accumulation across training points in fp64)
TOL32_L = 1e-4
TOL32_DS2 = 8e-4
TOL32_GRAD = 5e-3
TOL32_COEFF = 5e-3


@pytest.mark.parametrize("case", [(1, 2000, 50, 3, 0.1), (4, 5000, 300, 8, 0.1), (6, 20000, 512, 16, 0.1),
                                  (7, 8000, 256, 8, 1e-3)])
def test_fp32_bulk_iso_against_fp64_oracle(case):
    seed, n, m, d, s2 = case
    X, y, Z = synth(seed, n, m, d)
    le = 0.5 * np.log(d)
    ref = O.evaluate_fast(O.SeIsoKernel(le, 0.0), Z, X, y, s2)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, precision=gpr_amd.F32_BULK)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=le, log_sf2=0.0, sigma2=s2, inducing=Z)
    assert M.rel_ok("l", ev.l, ref["l"], TOL32_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL32_DS2)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL32_GRAD)
    assert M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL32_COEFF)
    ev0 = p.eval(log_ell=le, log_sf2=0.0, sigma2=s2, inducing=Z, want_grad=False)
    assert ev0.l == ev.l
    p.close()


def test_fp32_bulk_fat_ard_config3_shape():
    """BASELINE.json config 3 in miniature: Cov_se_fat with tproj = diag(1/ell_i) (ARD), d = D = 32,
    fp32 bulk, against the fp64 oracle; gradient includes all D*d Proj entries."""
    rng = np.random.default_rng(3)
    n, m, d = 6000, 256, 32
    X = np.asfortranarray(rng.normal(size=(d, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    ell = rng.uniform(-0.5, 0.5, size=d)
    P = np.asfortranarray(np.diag(np.exp(-ell)) / np.sqrt(d))
    k = O.SeFatKernel(d, 0.0, P)
    Z = np.asfortranarray(O.se_fat_project(k, X[:, rng.permutation(n)[:m]]) + 0.01 * rng.normal(size=(d, m)))
    ref = O.evaluate_fast(k, Z, X, y, 0.1)
    for prec, tl, tg in ((gpr_amd.F64, TOL_L, TOL_GRAD), (gpr_amd.F32_BULK, TOL32_L, TOL32_GRAD)):
        p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, d, d, m, precision=prec)
        p.set_inputs(X)
        p.set_targets(y)
        ev = p.eval(log_sf2=0.0, sigma2=0.1, inducing=Z, tproj=P)
        assert ev.grad.shape == ref["grad"].shape == (1 + d * m + d * d,)
        assert M.rel_ok("l", ev.l, ref["l"], tl)
        assert M.grad_ok(ev.grad, ref["grad"], M.families("fat", d, m, D=d, proj=True), tg)
        p.close()


def test_update_sigma2_reuses_resident_v():
    """Model.update_sigma2 (lib/fitc_gp.ml:234-236): re-evaluating with only sigma2 changed reuses K_nm, V, r
    and gives the same numbers as a fresh evaluation."""
    g = load_golden("iso_ragged")
    p = _problem_for(g, chunk_rows=256)
    _eval_golden(p, g)
    fresh = _eval_golden(p, g, sigma2=0.37)
    _eval_golden(p, g)
    fast = _eval_golden(p, g, sigma2=0.37, reuse_v=True)
    assert fast.l == fresh.l and fast.dl_dsigma2 == fresh.dl_dsigma2
    assert np.array_equal(fast.grad, fresh.grad)
    ref = O.evaluate_fast(oracle_kernel(g), g["Z"], g["X"], g["y"], 0.37)
    assert M.rel_ok("l", fast.l, ref["l"], TOL_L)
    p.close()
    q = _problem_for(g)
    with pytest.raises(gpr_amd.GprHipError, match="holds no V"):
        _eval_golden(q, g, reuse_v=True)
    # a loaded predictor installs factors but no V: reuse_v must still be refused
    ev = _eval_golden(q, g)
    u, r = q.co_variance_coeffs()
    q.load_predictor(log_ell=float(g["log_ell"]), log_sf2=float(g["log_sf2"]), sigma2=float(g["sigma2"]),
                     inducing=g["Z"], coeffs=ev.coeffs, co_variance_coeffs=(u, r))
    with pytest.raises(gpr_amd.GprHipError, match="holds no V"):
        _eval_golden(q, g, reuse_v=True)
    q.close()
    # through the mirror: update_sigma2 on a model whose kernel/inducing were just evaluated
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(float(g["log_ell"]), float(g["log_sf2"])))
    inducing = F.Deriv.Inducing.calc(kernel, g["Z"])
    model = F.Deriv.Model.calc(F.Deriv.Inputs.calc(inducing, g["X"]), sigma2=float(g["sigma2"]))
    tr = F.Deriv.Trained.calc(model, targets=g["y"])
    assert M.rel_ok("l", F.Eval.Trained.calc_log_evidence(tr), float(g["l"]), TOL_L)
    tr2 = F.Deriv.Trained.calc(F.Deriv.Model.update_sigma2(model, 0.37), targets=g["y"])
    assert M.rel_ok("l", F.Eval.Trained.calc_log_evidence(tr2), ref["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", F.Deriv.Trained.calc_log_evidence_sigma2(tr2), ref["dl_dsigma2"], TOL_DS2)
    GP.close()


def test_prediction_means_and_variances():
    """Means.calc / Variances.calc (lib/fitc_gp.ml:418-425, :498-518) on the device
    against the oracle, directly and through the mirrored module surface; test set larger than a chunk."""
    n, m, d, nt = 4000, 150, 3, 1300
    X, y, Z = synth(21, n, m, d)
    rng = np.random.default_rng(5)
    Xt = np.asfortranarray(rng.normal(size=(d, nt)))
    k = O.SeIsoKernel(0.4, 0.2)
    ref = O.evaluate(k, Z, X, y, 0.15, want_grad=False, keep=True)
    mean_ref = O.predict_means(k, Z, ref["coeffs"], Xt)
    var_ref = O.predict_variances(k, Z, ref["model"], Xt, predictive=False)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=512)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(log_ell=0.4, log_sf2=0.2, sigma2=0.15, inducing=Z, want_grad=False)
    mean, var = p.predict(Xt, predictive=False)
    assert M.vec_ok("pred_mean", mean, mean_ref, TOL_POST)
    assert np.max(np.abs(var - var_ref)) <= 1e-8 * np.max(np.abs(var_ref))
    _, varp = p.predict(Xt, predictive=True)
    assert np.allclose(varp, var + 0.15, rtol=0, atol=1e-12)
    p.close()
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(0.4, 0.2))
    inducing = F.Eval.Inducing.calc(kernel, Z)
    model = F.Eval.Model.calc(F.Eval.Inputs.calc(X, inducing), sigma2=0.15)
    trained = F.Eval.Trained.calc(model, targets=y)
    test_inputs = F.Eval.Inputs.calc(Xt, inducing)
    means = F.Eval.Means.get(F.Eval.Means.calc(F.Eval.Mean_predictor.calc_trained(trained), test_inputs))
    variances = F.Eval.Variances.calc(F.Eval.Co_variance_predictor.calc_model(model), 0.15, test_inputs)
    assert M.vec_ok("pred_mean", means, mean_ref, TOL_POST)
    assert M.vec_ok("pred_var", F.Eval.Variances.get(variances, predictive=False), var_ref, TOL_POST)
    assert M.vec_ok("pred_var", F.Eval.Variances.get(variances), var_ref + 0.15, TOL_POST)
    other = F.Eval.Inputs.calc(Xt, F.Eval.Inducing.calc(kernel, Z.copy()))
    with pytest.raises(ValueError, match="disagree about inducing points"):   # lib/fitc_gp.ml:419-424
        F.Eval.Means.calc(trained, other)
    GP.close()


@pytest.mark.parametrize("kind,n,m,d,nt", [("iso", 700, 30, 2, 20000), ("fat", 1500, 140, 3, 150000), ("iso", 300, 10, 1, 300000)])
def test_prediction_of_far_more_test_points_than_training_points(kind, n, m, d, nt):
    """A model trained on few points predicts many: the test points pass through chunks of their own (up to 131 072 rows,
    in buffers kept by the problem), not through the training chunk.  Means and variances against the oracle on a sample,
    against the chunk-by-chunk path (which a small second call still takes) on all of them."""
    rng = np.random.default_rng(n + nt)
    D = d + (2 if kind == "fat" else 0)
    X = np.asfortranarray(rng.normal(size=(D, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    Xt = np.asfortranarray(rng.normal(size=(D, nt)))
    if kind == "iso":
        Z = np.asfortranarray(X[:, rng.permutation(n)[:m]] + 0.01 * rng.normal(size=(d, m)))
        k = O.SeIsoKernel(0.3, 0.1)
        args = dict(log_ell=0.3, log_sf2=0.1)
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    else:
        P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d))
        Z = np.asfortranarray((P.T @ X)[:, rng.permutation(n)[:m]] + 0.01 * rng.normal(size=(d, m)))
        k = O.SeFatKernel(d, 0.1, P, None, None)
        args = dict(log_sf2=0.1, tproj=P)
        p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, d, m)
    ref = O.evaluate(k, Z, X, y, 0.2, want_grad=False, keep=True)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(sigma2=0.2, inducing=Z, want_grad=False, **args)
    mean, var = p.predict(Xt, predictive=False)
    sample = rng.permutation(nt)[:3000]
    Xs = np.asfortranarray(Xt[:, sample])
    assert M.vec_ok("pred_mean", mean[sample], O.predict_means(k, Z, ref["coeffs"], Xs), TOL_POST)
    vref = O.predict_variances(k, Z, ref["model"], Xs, predictive=False)
    assert np.max(np.abs(var[sample] - vref)) <= 1e-8 * np.max(np.abs(vref))
    # the same points in pieces no larger than the training chunk
    step = 256
    for lo in range(0, min(nt, 4096), step):
        mp_, vp_ = p.predict(np.asfortranarray(Xt[:, lo:lo + step]), predictive=False)
        assert np.array_equal(mp_, mean[lo:lo + step]) and np.array_equal(vp_, var[lo:lo + step])
    p.close()


def test_save_data_recipe_training_improves_evidence_and_fits_noise():
    """test/save_data.ml + test/gen_data.ml:23-44 recipe: 1-D f(x) = sin(3x)/x + |x-3|/(x^2+1), noise
    sigma 0.7, n=1000, m=10, Cov_se_iso FITC; evidence maximisation must raise the log evidence and the
    fit's RMSE against the noisy targets must sit near the noise level."""
    from gpr_amd import optim
    g = load_golden("iso_gen_data")
    X, y, Z = g["X"], g["y"], g["Z"]
    GP = fitc_gp.Make_deriv(cov_se_iso)
    kernel = cov_se_iso.Kernel.create(cov_se_iso.create_default_kernel_params())
    F = GP.FITC
    ind0 = F.Deriv.Inducing.calc(kernel, Z)
    tr0 = F.Eval.Trained.calc(F.Eval.Model.calc(F.Eval.Inputs.calc(X, ind0), sigma2=float(y @ y) / 1000), y)
    le0 = F.Eval.Trained.calc_log_evidence(tr0)
    k1, z1, s2, le1, nev = optim.train(F, cov_se_iso, kernel, Z, X, y, max_iter=60)
    assert le1 > le0 + 50.0
    assert 0.3 < s2 < 0.8                      # true noise variance 0.49
    ind1 = F.Eval.Inducing.calc(k1, z1)
    trained = F.Eval.Trained.calc(F.Eval.Model.calc(F.Eval.Inputs.calc(X, ind1), sigma2=s2), y)
    means = F.Eval.Means.calc(trained, F.Eval.Inputs.calc(X, ind1))
    rmse = float(np.sqrt(np.mean((means - y) ** 2)))
    assert 0.55 < rmse < 0.85                  # noise sigma 0.7
    GP.close()


@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (3, 3, 2), (2, 5, 3), (129, 128, 4), (128, 129, 1)])
def test_degenerate_and_tile_edge_sizes(n, m, d):
    """Single point, m == n, m > n, and sizes straddling the 128-tile boundary."""
    rng = np.random.default_rng(n * 1000 + m)
    X = np.asfortranarray(rng.normal(size=(d, n)))
    y = rng.normal(size=n)
    Z = np.asfortranarray(rng.normal(size=(d, m)))
    ref = O.evaluate_fast(O.SeIsoKernel(0.2, -0.3), Z, X, y, 0.5)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=0.2, log_sf2=-0.3, sigma2=0.5, inducing=Z)
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    # (m > n, points on a line: K_m is jitter-dominated -- the conditioning allowance of tests/margins.py applies)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD, cond=p.condition()[0])
    assert abs(ev.dl_dsigma2 - ref["dl_dsigma2"]) <= TOL_DS2 * max(abs(ref["dl_dsigma2"]), 1e-3)
    p.close()


def test_functor_mirror_and_reference_self_test_recipe():
    """test/test_derivatives.ml's recipe through the mirrored module surface: finite differences at
    the reference's eps=1e-8 / tol=1e-2 for sigma2 and every hyper (n=10, m=5, D=3)."""
    rng = np.random.default_rng(4)
    X = np.asfortranarray(rng.uniform(size=(3, 10)))
    y = rng.uniform(size=10)
    Z = np.asfortranarray(X[:, :5].copy())
    GP = fitc_gp.Make_deriv(cov_se_iso)
    FITC = GP.FITC
    kernel = cov_se_iso.Kernel.create(cov_se_iso.create_default_kernel_params())
    hypers = FITC.Deriv.Spec.HyperModule.get_all(kernel, Z, X)
    FITC.Deriv.Test.self_test(kernel, Z, X, sigma2=1.0, targets=y, hyper="Sigma2")
    for h in hypers:
        FITC.Deriv.Test.self_test(kernel, Z, X, sigma2=1.0, targets=y, hyper=h)
    # staged calls of the signature, against the oracle
    inducing = FITC.Deriv.Inducing.calc(kernel, Z)
    inputs = FITC.Deriv.Inputs.calc(inducing, X)
    model = FITC.Deriv.Model.calc(inputs, sigma2=1.0)
    trained = FITC.Deriv.Trained.calc(model, targets=y)
    ref = O.evaluate(O.SeIsoKernel(0.0, 0.0), Z, X, y, 1.0)
    assert abs(FITC.Eval.Trained.calc_log_evidence(FITC.Deriv.Trained.calc_eval(trained)) - ref["l"]) < 1e-9
    assert abs(FITC.Eval.Model.calc_log_evidence(FITC.Deriv.Model.calc_eval(model)) - ref["l1"]) < 1e-9
    assert abs(FITC.Deriv.Trained.calc_log_evidence_sigma2(trained) - ref["dl_dsigma2"]) < 1e-8
    ht = FITC.Deriv.Trained.prepare_hyper(trained)
    got = np.array([FITC.Deriv.Trained.calc_log_evidence(ht, h) for h in hypers])
    assert M.grad_ok(got, ref["grad"], M.families("iso", 3, 5), TOL_GRAD)
    hm = FITC.Deriv.Model.prepare_hyper(model)
    gotm = np.array([FITC.Deriv.Model.calc_log_evidence(hm, h) for h in hypers])
    assert M.grad_ok(gotm, ref["model_grad"], M.families("iso", 3, 5), TOL_GRAD, "model_grad")
    assert M.vec_ok("pred_mean", FITC.Eval.Trained.calc_mean_coeffs(trained), ref["coeffs"], 1e-7)
    g = FITC.Deriv.Optim.calc_gradient(True, 1.0, hypers, trained)
    assert abs(g[0] - ref["dl_dsigma2"] * 1.0) < 1e-8 and M.grad_ok(g[1:], ref["grad"], M.families("iso", 3, 5), TOL_GRAD)
    # variational functor
    V = GP.Variational_FITC
    vt = V.Deriv.Trained.calc(V.Deriv.Model.calc(V.Deriv.Inputs.calc(V.Deriv.Inducing.calc(kernel, Z), X), 1.0), y)
    refv = O.evaluate(O.SeIsoKernel(0.0, 0.0), Z, X, y, 1.0, variational=True)
    assert abs(V.Eval.Trained.calc_log_evidence(vt) - refv["l"]) < 1e-9
    GP.close()


def test_two_shards_on_one_device_equal_the_whole():
    """The staged entry points: two row shards whose exchange buffers are summed == one problem."""
    import torch
    n, m, d = 3001, 140, 4
    X, y, Z = synth(12, n, m, d)
    hyp = dict(log_ell=0.6, log_sf2=0.1, sigma2=0.2, inducing=Z)
    whole = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    whole.set_inputs(X)
    whole.set_targets(y)
    ref = whole.eval(**hyp)
    cut = 1234
    shards = []
    for lo, hi in ((0, cut), (cut, n)):
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, hi - lo, d, d, m, chunk_rows=512)
        p.set_inputs(X[:, lo:hi])
        p.set_targets(y[lo:hi])
        shards.append(p)
    dev = torch.device("cuda", 0)
    ar1 = [torch.zeros(p.ar1_len(), dtype=torch.float64, device=dev) for p in shards]
    ar2 = [torch.zeros(p.ar2_len(), dtype=torch.float64, device=dev) for p in shards]
    for p, a in zip(shards, ar1):
        p.eval_pass1(a.data_ptr(), n, **hyp)
        p.sync()
    tot1 = ar1[0] + ar1[1]
    torch.cuda.synchronize()
    for p, a in zip(shards, ar2):
        p.eval_pass2(tot1.data_ptr(), a.data_ptr())
        p.sync()
    tot2 = ar2[0] + ar2[1]
    torch.cuda.synchronize()
    evs = [p.eval_finish(tot2.data_ptr()) for p in shards]
    for ev in evs:
        assert M.rel_ok("l", ev.l, ref.l, TOL_SHARD)
        assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref.dl_dsigma2, TOL_SHARD)
        assert M.grad_ok(ev.grad, ref.grad, M.families("iso", d, m), TOL_SHARD_GRAD)
    for p in shards + [whole]:
        p.close()


def test_error_behaviour():
    X, y, Z = synth(0, 50, 4, 2)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, 50, 2, 2, 4)
    p.set_inputs(X)
    p.set_targets(y)
    with pytest.raises(gpr_amd.GprHipError, match="sigma2 < 0"):          # lib/fitc_gp.ml:148-149
        p.eval(log_ell=0.0, log_sf2=0.0, sigma2=-1.0, inducing=Z)
    Zdup = np.asfortranarray(np.repeat(Z[:, :1], 4, axis=1))
    with pytest.raises(gpr_amd.NotPositiveDefinite):                        # Lacaml potrf Failure
        p.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Zdup, jitter=0.0)
    # A refused factorisation leaves NaN behind it on the device (the pivot chain does not patch a non-positive pivot: the
    # select would sit on its dependent path; chol.hip, CH_PIVOT) -- in the factor, in V, and in the exchange buffers that a
    # sharded evaluation all-reduces.  What the host may rely on: the status with the failing minor, no state kept from
    # the failed call (reuse_v is refused), and a clean result from the next call.
    with pytest.raises(gpr_amd.GprHipError, match="holds no V"):
        p.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Zdup, reuse_v=True)
    # with the reference's jitter the same inducing set factorises (lib/utils.ml:35)
    ev = p.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Zdup)
    assert np.isfinite(ev.l) and np.all(np.isfinite(ev.grad))
    good = p.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Z)
    # ... and the same through the multi-device entry (two shards on the one device: both exchange buffers carry the NaN
    # of the failed call through the fixed-order sum) and through several 128-blocks of inducing points
    ctx = gpr_amd.Context([0, 0])
    sp = gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, 50, 2, 2, 4)
    sp.set_inputs(X)
    sp.set_targets(y)
    with pytest.raises(gpr_amd.NotPositiveDefinite, match="leading minor of order 2 of K_m"):
        sp.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Zdup, jitter=0.0)
    with pytest.raises(gpr_amd.GprHipError, match="holds no V"):
        sp.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Zdup, reuse_v=True)
    after = sp.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Z)
    assert M.rel_ok("l", after.l, good.l, TOL_SHARD) and M.grad_ok(after.grad, good.grad, M.families("iso", 2, 4), TOL_SHARD_GRAD)
    sp.close()
    ctx.close()
    Xb, yb, Zb = synth(3, 900, 300, 3)
    Zb[:, 200] = Zb[:, 17]
    q = gpr_amd.Problem(gpr_amd.COV_SE_ISO, 900, 3, 3, 300)
    q.set_inputs(Xb)
    q.set_targets(yb)
    with pytest.raises(gpr_amd.NotPositiveDefinite, match="leading minor of order 201 of K_m"):
        q.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Zb, jitter=0.0)
    evb = q.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Zb)
    assert np.isfinite(evb.l) and np.all(np.isfinite(evb.grad)) and np.all(np.isfinite(evb.coeffs))
    q.close()
    with pytest.raises(ValueError, match="targets"):                         # lib/fitc_gp.ml:283-284
        p.set_targets(y[:-1])
    p.close()
    with pytest.raises(gpr_amd.GprHipError):
        gpr_amd.Problem(gpr_amd.COV_SE_ISO, 0, 2, 2, 4)


def test_library_loaded_before_torch_is_refused_by_name():
    """On the GPU box: libgprhip.so first, torch second maps two HIP runtimes -- gprhip_problem_create / gprhip_ctx_create
    refuse, naming both files; torch first, one runtime serves both and both entry points succeed (tests/test_abi.py holds
    the probe; INTEGRATION.md, "hosts that also load torch")."""
    from tests.test_abi import _load_order_probe
    bad = _load_order_probe("library")
    if bad["N"] == "2":
        assert bad["P"].startswith("3 gprhip_problem_create: two HIP runtimes are mapped"), bad
        assert bad["C"].startswith("3 gprhip_ctx_create: two HIP runtimes are mapped"), bad
    good = _load_order_probe("torch")
    assert good["N"] == "1" and good["P"].split(" ", 1)[0] == "0" and good["C"].split(" ", 1)[0] == "0", good


def test_headline_size_properties():
    """BASELINE.json C2 shape (n=1M, m=2048, d=8): size-independent properties -- run-to-run bitwise
    determinism, evidence-only == gradient-mode evidence, directional derivative vs a central
    difference of device evaluations."""
    n, m, d = 1_000_000, 2048, 8
    X, y, Z = synth(2, n, m, d)
    le = 0.5 * np.log(d)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    hyp = dict(log_ell=le, log_sf2=0.0, sigma2=0.1, inducing=Z)
    a = p.eval(**hyp)
    b = p.eval(**hyp)
    assert a.l == b.l and np.array_equal(a.grad, b.grad)
    assert np.isfinite(a.l) and np.all(np.isfinite(a.grad))
    l0 = p.eval(want_grad=False, **hyp).l
    assert M.rel_ok("l", l0, a.l, 1e-12)
    rng = np.random.default_rng(0)
    dz = rng.normal(size=Z.shape)
    dz /= np.linalg.norm(dz)
    dle, dls, ds2 = 0.3, -0.2, 0.05
    eps = 1e-4
    plus = p.eval(want_grad=False, log_ell=le + eps * dle, log_sf2=eps * dls, sigma2=0.1 + eps * ds2,
                  inducing=Z + eps * dz).l
    minus = p.eval(want_grad=False, log_ell=le - eps * dle, log_sf2=-eps * dls, sigma2=0.1 - eps * ds2,
                   inducing=Z - eps * dz).l
    fd = (plus - minus) / (2 * eps)
    analytic = a.grad[0] * dle + a.grad[1] * dls + a.dl_dsigma2 * ds2 + float(a.grad[2:] @ dz.T.reshape(-1))
    assert abs(fd - analytic) <= 1e-5 * max(abs(analytic), abs(a.l) * 1e-6)
    p.close()


def _run_bench(extra, nproc):
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--steps", "2", "--warmup", "1", "--points", "20011", "--inducing", "200", "--dims", "4", "--full", "--no-cpu-baseline",
              "--no-configs"]
    if nproc == 1 and not extra:
        cmd = [sys.executable, "bench.py", "--gpus", "1"] + common
    elif "--same-device" in extra or "--expect-failure" in extra:  # ONE process, gprhip_ctx_create(devices[])
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
        cmd = [sys.executable, "bench.py", "--gpus", str(nproc)] + common + [e for e in extra if e != "--expect-failure"]
        out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600, env=env)
        if "--expect-failure" in extra:
            return out
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout
        return json.loads(lines[0])
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", str(nproc)] \
            + common + extra
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 prints exactly one JSON line
    return json.loads(lines[0])


def test_bench_two_ranks_on_one_device_match_single_rank():
    """bench.py's N>1 code path (row shards + two all-reduces between the staged calls) on the one GPU a
    test box has: two ranks share cuda:0 and reduce over gloo.  Same seeded hyper-parameter stream, so
    the last evaluation must agree with the single-rank run."""
    one = _run_bench([], 1)
    two = _run_bench(["--backend", "gloo", "--share-device"], 2)
    assert two["n_gpus"] == 2 and two["scaling"] == "strong"
    for k in ("l", "dl_dsigma2", "grad_norm"):
        a, b = one["last_eval"][k], two["last_eval"][k]
        assert abs(a - b) <= TOL_BENCH * max(1.0, abs(a)), (k, a, b)


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    """A plain `bench.py` run (no --full) times the steps and prints the headline fields only; --dump-outputs writes the
    last timed step's results, which the line's last_eval summarises.  --steps sets the number of timed steps, and the
    hyper-parameter set of an evaluation depends only on its position: 3 timed steps after 1 warm-up and 2 after 2 end
    on the same (fourth) set, so the two runs dump the same results bit for bit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for k, (steps, warmup) in enumerate(((3, 1), (2, 2))):
        out_dir = tmp_path / ("out%d" % k)
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--points", "20011",
               "--inducing", "200", "--dims", "4", "--dump-outputs", str(out_dir)]
        out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout
        runs.append((json.loads(lines[0]), {f.stem: np.load(f) for f in out_dir.glob("*.npy")}))
    line, dump = runs[0]
    assert line["step_ms"]["timed_steps"] == 3 and runs[1][0]["step_ms"]["timed_steps"] == 2
    assert line["steps"] == 3 and line["ms_per_step"] > 0.0 and line["unit"] == "training-points/s"
    assert line["dtype"] == "f64" and line["higher_is_better"] is True
    for k in ("stage_ms", "evidence_only", "configs", "cpu_baseline", "single_process_context", "roofline_k_builder"):
        assert k not in line, k
    assert set(dump) == {"l1", "l2", "l", "dl_dsigma2", "grad", "coeffs"}
    assert all(a.dtype == np.float64 for a in dump.values())
    assert dump["grad"].shape == (2 + 4 * 200,) and dump["coeffs"].shape == (200,)
    assert float(dump["l"]) == line["last_eval"]["l"] and float(dump["dl_dsigma2"]) == line["last_eval"]["dl_dsigma2"]
    assert float(np.linalg.norm(dump["grad"])) == line["last_eval"]["grad_norm"]
    for k, a in dump.items():
        assert np.array_equal(a, runs[1][1][k]), k


def test_bench_single_process_eight_way_matches_one_gpu_and_torchrun():
    """`python bench.py --gpus 8` with NO launcher: the reference's host is one process (bin/ocaml_gpr.ml:176-177,
    :340-342), so the N-GPU bench goes through the C ABI's own multi-device entry (gprhip_ctx_create ->
    gprhip_sharded_eval).  On the one GPU a test box has, --same-device puts the eight shards on device 0 (validation
    mode: fixed-order device-local sum as the exchange).  Same seeded hyper-parameter stream in every launch, so the last
    evaluation must agree with the one-GPU run and with the torchrun launch of the same partition."""
    one = _run_bench([], 1)
    ctx8 = _run_bench(["--same-device"], 8)
    assert ctx8["n_gpus"] == 8 and ctx8["scaling"] == "strong" and ctx8["launch"] == "single-process ctx"
    mg = ctx8["multi_gpu"]
    assert mg["launch"] == "single-process ctx" and mg["mode"] == "same-device sum" and mg["devices"] == [0] * 8
    assert mg["collectives_per_gradient_eval"] == 2 and mg["collectives_per_evidence_eval"] == 1
    assert all(b > 0 for b in mg["allreduce_bytes"]) and mg["replicated_mxm_ms"] > 0.0
    assert "n=20011 m=200 d=4" in ctx8["metric"]  # the metric string follows the arguments
    assert 0.0 < ctx8["evidence_only"]["frac"] < 1.0
    two = _run_bench(["--backend", "gloo", "--share-device"], 2)
    assert two["launch"] == "torchrun" and two["multi_gpu"]["launch"] == "torchrun"
    for other in (ctx8, two):
        for k in ("l", "dl_dsigma2", "grad_norm"):
            a, b = one["last_eval"][k], other["last_eval"][k]
            assert abs(a - b) <= TOL_BENCH * max(1.0, abs(a)), (k, a, b)
    # more devices asked for than the box has, without --same-device: a message naming both counts, non-zero exit
    visible = gpr_amd.device_count()
    out = _run_bench(["--expect-failure"], visible + 1)
    assert out.returncode != 0 and "--gpus %d" % (visible + 1) in out.stderr and "%d HIP device" % visible in out.stderr


def test_bench_config_c4_launch_on_one_device():
    """`python bench.py --gpus 8 --config c4` is BASELINE.json configs[3]'s command (n = 8M, m = 4096, d = 16, seed 4, one
    process, RCCL inside the library).  An 8-GPU node is not available to the build, so the same launch runs here with the
    eight shards on the one device (--same-device) at n = 160 003: argument handling, the named workload, the packed
    exchange buffers of m = 4096 and a finite result."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, "bench.py", "--gpus", "8", "--config", "c4", "--same-device", "--points", "160003", "--steps", "1",
           "--warmup", "1", "--full", "--no-cpu-baseline", "--no-configs"]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    cfg = line["config"]
    assert cfg["name"] == "c4" and cfg["seed"] == 4 and (cfg["n"], cfg["m"], cfg["d"]) == (160003, 4096, 16)
    assert "BASELINE.json configs[3]" in cfg["workload"] and "other than the named" in cfg["workload"]
    assert line["n_gpus"] == 8 and line["launch"] == "single-process ctx" and "m=4096 d=16" in line["metric"]
    mg = line["multi_gpu"]
    assert mg["collectives_per_gradient_eval"] == 2 and mg["allreduce_bytes"][0] == 8 * gpr_amd.load().gprhip_exchange_len(0, 16, 16, 4096, 1)
    assert np.isfinite(line["last_eval"]["l"]) and line["last_eval"]["grad_norm"] > 0.0


def test_a_shard_that_cannot_fit_is_refused_before_any_allocation():
    """gprhip_memory_plan + the check in gprhip_problem_create / gprhip_sharded_create: BASELINE.json configs[3] (n = 8M,
    m = 4096, d = 16, fp64) needs 321 GB on one device -- refused with GPRHIP_EOOM and the figures, and the device's free
    memory is what it was (nothing was allocated, nothing to unwind); its 8-way shard (64.6 GB) is created."""
    import torch
    free0 = torch.cuda.mem_get_info(0)[0]
    with pytest.raises(gpr_amd.GprHipError, match=r"needs 32\d\.\d GB on device 0 .* free") as e:
        gpr_amd.Problem(gpr_amd.COV_SE_ISO, 8_000_000, 16, 16, 4096)
    assert e.value.status == 4  # GPRHIP_EOOM
    assert abs(torch.cuda.mem_get_info(0)[0] - free0) < (64 << 20)
    # two shards of it on ONE device (validation mode): 2 x 187.5 GB -- the context refuses before the first shard allocates
    ctx = gpr_amd.Context([0, 0])
    with pytest.raises(gpr_amd.GprHipError, match=r"gprhip_sharded_create: the shards on device 0 need 37\d\.\d GB") as e2:
        gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, 8_000_000, 16, 16, 4096)
    assert e2.value.status == 4
    assert abs(torch.cuda.mem_get_info(0)[0] - free0) < (64 << 20)
    ctx.close()
    lo, hi = gpr_amd.dist.shard_rows(8_000_000, 7, 8)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, hi - lo, 16, 16, 4096)
    plan = gpr_amd.memory_plan(gpr_amd.COV_SE_ISO, hi - lo, 16, 16, 4096)
    used = free0 - torch.cuda.mem_get_info(0)[0]
    # created state = the plan without the V store (that comes with the first evaluation), to allocator granularity
    assert abs(used - (plan["total"] - plan["v_store"])) < 0.02 * plan["total"], (used, plan)
    p.close()


def test_bench_under_torchrun_with_rccl_one_rank():
    """The launch the driver uses for N > 1 (torch.distributed.run, backend nccl = RCCL), with the one rank a test box
    can host: RCCL initialises, the exchange buffers the library filled are all-reduced on the device with event
    ordering between the library's stream and torch's, and the result equals the plain single-process run.  Two
    collectives per gradient evaluation, one per evidence-only evaluation."""
    one = _run_bench([], 1)
    rccl = _run_bench(["--backend", "nccl"], 1)
    mg = rccl["multi_gpu"]
    assert mg["backend"] == "nccl" and mg["rccl_ranks"] == 1
    assert mg["collectives_per_gradient_eval"] == 2 and mg["collectives_per_evidence_eval"] == 1
    assert len(mg["allreduce_ms"]) == 2 and all(t > 0.0 for t in mg["allreduce_ms"])
    assert mg["replicated_mxm_ms"] > 0.0
    for k in ("l", "dl_dsigma2", "grad_norm"):
        a, b = one["last_eval"][k], rccl["last_eval"][k]
        assert abs(a - b) <= 1e-12 * max(1.0, abs(a)), (k, a, b)


def test_stats_covariances_and_samplers():
    """Stats (lib/fitc_gp.ml:304-374), FITC_/FIC_covariances (:565-627), Cov_sampler and Sampler
    (:629-697) on the device against the oracle -- directly on the C ABI and through the mirrored modules.
    nt is not a multiple of the tile and the training set spans several chunks."""
    n, m, d, nt = 3000, 130, 3, 301
    X, y, Z = synth(33, n, m, d)
    rng = np.random.default_rng(8)
    Xt = np.asfortranarray(rng.normal(size=(d, nt)))
    k = O.SeIsoKernel(0.35, 0.15)
    s2 = 0.2
    ref = O.evaluate(k, Z, X, y, s2, want_grad=False, keep=True)
    knm, _ = O.spec_calc_shared_cross(k, X, Z)
    tm_ref = knm @ ref["coeffs"]
    st_ref = O.stats_calc(y, tm_ref, ref["l"])
    fitc_ref = O.fitc_covariances(k, Z, ref["model"], Xt)
    fic_ref = O.fic_covariances(k, Z, ref["model"], Xt)
    mean_ref = O.predict_means(k, Z, ref["coeffs"], Xt)

    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=1024)
    p.set_inputs(X)
    p.set_targets(y)
    p.eval(log_ell=0.35, log_sf2=0.15, sigma2=s2, inducing=Z, want_grad=False)
    sums, tm = p.train_stats(want_means=True)
    assert M.vec_ok("train_means", tm, tm_ref, TOL_POST)
    assert abs(sums[0] - st_ref["sse"]) <= 1e-8 * st_ref["sse"]
    assert abs(sums[1] / n - st_ref["mad"]) <= 1e-8 * st_ref["mad"]
    assert abs(sums[2] - st_ref["maxad"]) <= 1e-8 * st_ref["maxad"]
    assert abs(sums[3] / n - st_ref["target_variance"]) <= 1e-12 * st_ref["target_variance"]
    scale = np.max(np.abs(np.diag(fitc_ref)))
    for kind, cref in (("FITC", fitc_ref), ("FIC", fic_ref)):
        cov = p.covariances(Xt, kind=kind, predictive=False)
        assert np.array_equal(cov, cov.T)
        assert np.max(np.abs(np.triu(cov) - cref)) <= 1e-8 * max(scale, np.max(np.abs(cref)))
        covp = p.covariances(Xt, kind=kind, predictive=True)
        assert np.allclose(np.diag(covp), np.diag(cov) + s2, rtol=0, atol=1e-12)
    cov = p.covariances(Xt, kind="FITC", predictive=False)
    _, var = p.predict(Xt, predictive=False)
    assert np.max(np.abs(np.diag(cov) - var)) <= 1e-9 * scale
    # sampler: same z through the oracle's potrf/trmm
    z = rng.normal(size=(nt, 5))
    smp_ref = O.cov_sampler_calc(mean_ref, fitc_ref, s2, predictive=True)
    S_ref = O.cov_sampler_samples(smp_ref, z)
    S = p.cov_samples(cov, mean_ref, z, add_diag=s2)
    assert S.shape == (nt, 5) and np.max(np.abs(S - S_ref)) <= 1e-9 * np.max(np.abs(S_ref))
    # z = I returns means + chol^T column by column: chol^T chol must rebuild the matrix
    L = p.cov_samples(cov, np.zeros(nt), np.eye(nt), add_diag=s2)          # = chol^T
    assert np.max(np.abs(np.triu(L, 1))) == 0.0
    full = cov + (s2 + 1e-6) * np.eye(nt)
    assert np.max(np.abs(L @ L.T - full)) <= 1e-12 * np.max(np.abs(full))
    with pytest.raises(gpr_amd.NotPositiveDefinite):
        p.cov_samples(-np.eye(nt), np.zeros(nt), z)
    p.close()

    GP = fitc_gp.Make_deriv(cov_se_iso)
    kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(0.35, 0.15))
    for F, cref in ((GP.FITC, fitc_ref), (GP.FIC, fic_ref)):
        E = F.Eval
        inducing = E.Inducing.calc(kernel, Z)
        model = E.Model.calc(E.Inputs.calc(X, inducing), sigma2=s2)
        trained = E.Trained.calc(model, targets=y)
        st = E.Stats.calc(trained)
        for key in ("target_variance", "sse", "mse", "rmse", "smse", "msll", "mad", "maxad"):
            assert abs(getattr(st, key) - st_ref[key]) <= 1e-8 * abs(st_ref[key]), key
        assert st.n_samples == n and abs(E.Stats.calc_rmse(trained) - st_ref["rmse"]) <= 1e-8
        assert M.vec_ok("pred_mean", E.Trained.calc_means(trained), tm_ref, TOL_POST)
        tin = E.Inputs.calc(Xt, inducing)
        covs = E.Covariances.calc(E.Co_variance_predictor.calc_model(model), s2, tin)
        assert np.max(np.abs(np.triu(E.Covariances.get(covs, predictive=False)) - cref)) <= 1e-8 * scale
        assert np.allclose(np.diag(E.Covariances.get(covs)), np.diag(cref) + s2, rtol=0, atol=1e-8)
        v = E.Covariances.get_variances(covs)
        assert np.allclose(E.Variances.get(v, predictive=False), np.diag(cref), rtol=0, atol=1e-8)
    E = GP.FITC.Eval
    means = E.Means.get(E.Means.calc(E.Mean_predictor.calc_trained(trained), tin))
    smp = E.Cov_sampler.calc(means, E.Covariances.calc(model, s2, tin), predictive=True, points=tin.points)
    S2 = E.Cov_sampler.samples_from(smp, z)
    assert np.max(np.abs(S2 - S_ref)) <= 1e-8 * np.max(np.abs(S_ref))
    draws = E.Cov_sampler.samples(smp, 64, rng=np.random.default_rng(0))
    assert draws.shape == (nt, 64) and np.all(np.isfinite(draws))
    assert E.Cov_sampler.sample(smp, rng=np.random.default_rng(1)).shape == (nt,)
    # single-point modules
    inp = E.Input.calc(inducing, Xt[:, 7])
    mean1 = E.Mean.calc(trained, inp)
    var1 = E.Variance.calc(model, s2, inp)
    assert abs(E.Mean.get(mean1) - mean_ref[7]) <= 1e-8 * np.max(np.abs(mean_ref))
    assert abs(E.Variance.get(var1, predictive=False) - fitc_ref[7, 7]) <= 1e-8 * scale
    one = E.Sampler.calc(mean1, var1)
    assert abs(one.stddev - np.sqrt(fitc_ref[7, 7] + s2)) <= 1e-8
    assert E.Sampler.samples(one, 10, rng=np.random.default_rng(2)).shape == (10,)
    GP.close()


def test_calc_model_inputs_family_and_inducing_choice():
    """Sigs.Eval members either side of the path: Variances.calc_model_inputs (lib/fitc_gp.ml:487-496),
    FITC_/FIC_covariances.calc_model_inputs (:569-579, :609-614; as written, with the model's sqrt(1/s)-scaled Q factor)
    against the oracle, for a standard and a variational model, and a model built on Inducing.choose_n_first_inputs /
    choose_n_random_inputs evaluated against the oracle on the same chosen points."""
    n, m, d = 700, 70, 3
    X, y, _ = synth(41, n, m, d)
    s2 = 0.15
    kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(0.3, -0.1))
    k = O.SeIsoKernel(0.3, -0.1)
    GP = fitc_gp.Make_deriv(cov_se_iso)
    for F, fic, variational in ((GP.FITC, False, False), (GP.FIC, True, False), (GP.Variational_FITC, False, True)):
        E = F.Eval
        Z = E.Inducing.choose_n_random_inputs(kernel, X, n_inducing=m, rnd_state=5)  # Spec.Inducing.t: the points
        inducing = E.Inducing.calc(kernel, Z)
        assert E.Inducing.get_points(inducing) is Z
        assert Z.shape == (d, m) and len({tuple(c) for c in Z.T}) == m
        assert all(any(np.array_equal(c, x) for x in X.T) for c in Z.T[:5])
        model = E.Model.calc(E.Inputs.calc(X, inducing), sigma2=s2)
        ref = O.evaluate(k, Z, X, y, s2, want_grad=False, keep=True, variational=variational)
        trained = E.Trained.calc(model, targets=y)
        assert M.rel_ok("l", E.Trained.calc_log_evidence(trained), ref["l"], 1e-9)
        var_ref = O.variances_model_inputs(ref["model"])
        v = E.Variances.calc_model_inputs(model)
        assert M.vec_ok("pred_var", E.Variances.get(v, predictive=False), var_ref, TOL_POST)
        assert M.vec_ok("pred_var", E.Variances.get(v), var_ref + s2, TOL_POST)
        cref = O.fic_covariances_model_inputs(ref["model"]) if fic else O.fitc_covariances_model_inputs(k, ref["model"], X)
        c = E.Covariances.calc_model_inputs(model)
        got = E.Covariances.get(c, predictive=False)
        assert np.max(np.abs(np.triu(got) - cref)) <= 1e-8 * np.max(np.abs(cref))
        assert np.allclose(np.diag(E.Covariances.get(c)), np.diag(cref) + s2, rtol=0, atol=1e-8)
    first = GP.FITC.Eval.Inducing.choose_n_first_inputs(kernel, X, n_inducing=m)
    assert np.array_equal(first, X[:, :m])
    GP.close()
    # Cov_se_fat: the chosen inputs are projected into the kernel's space (create_inducing = project, lib/cov_se_fat.ml:220)
    D, dd = 5, 2
    rng = np.random.default_rng(3)
    Xb = np.asfortranarray(rng.normal(size=(D, 300)) + 2.0)
    fk = cov_se_fat.Kernel.create(cov_se_fat.Params.create(dd, 0.1, tproj=rng.normal(size=(D, dd)) / np.sqrt(D)))
    GPf = fitc_gp.Make_deriv(cov_se_fat)
    Zf = GPf.FITC.Eval.Inducing.choose_n_first_inputs(fk, Xb, n_inducing=20)
    ind = GPf.FITC.Eval.Inducing.calc(fk, Zf)
    assert Zf.shape == (dd, 20) and np.allclose(Zf, fk.params.tproj.T @ Xb[:, :20], rtol=0, atol=1e-15)
    yb = np.sin(Xb.sum(0))
    tr = GPf.FITC.Eval.Trained.calc(GPf.FITC.Eval.Model.calc(GPf.FITC.Eval.Inputs.calc(Xb, ind), sigma2=0.1), targets=yb)
    reff = O.evaluate(O.SeFatKernel(dd, 0.1, fk.params.tproj, None, None), Zf, Xb, yb, 0.1, want_grad=False)
    assert M.rel_ok("l", GPf.FITC.Eval.Trained.calc_log_evidence(tr), reff["l"], 1e-9)
    GPf.close()


@pytest.mark.parametrize("name", posterior_golden_names())
def test_golden_posterior(name):
    """Committed posterior fixtures (tests/golden/make_golden.py save_posterior): prediction, both covariance
    families, the covariance sampler with fixed draws, training-set statistics; iso and Cov_se_fat with
    projection + heteroskedastic + multiscale terms."""
    g = load_golden(name)
    p = _problem_for(g, chunk_rows=256)
    ev = _eval_golden(p, g, want_grad=False)
    assert M.rel_ok("l", ev.l, g["l"], TOL_L)
    s2 = float(g["sigma2"])
    means, var = p.predict(g["Xt"], predictive=False)
    assert M.vec_ok("pred_mean", means, g["means"], TOL_POST)
    assert M.vec_ok("pred_var", var, g["variances"], TOL_POST)
    scale = max(np.max(np.abs(g["fitc_cov"])), np.max(np.abs(g["fic_cov"])))
    cov = p.covariances(g["Xt"], kind="FITC", predictive=False)
    assert np.max(np.abs(np.triu(cov) - g["fitc_cov"])) <= 1e-8 * scale
    assert np.max(np.abs(np.triu(p.covariances(g["Xt"], kind="FIC", predictive=False)) - g["fic_cov"])) <= 1e-8 * scale
    S = p.cov_samples(cov, means, g["z"], add_diag=s2)
    assert np.max(np.abs(S - g["samples"])) <= 1e-8 * np.max(np.abs(g["samples"]))
    sums, tm = p.train_stats(want_means=True)
    assert M.vec_ok("pred_mean", tm, g["train_means"], TOL_POST)
    st = dict(zip(STAT_KEYS, g["stats"]))
    n = int(st["n_samples"])
    assert abs(sums[0] - st["sse"]) <= 1e-8 * st["sse"] and abs(sums[1] / n - st["mad"]) <= 1e-8 * st["mad"]
    assert abs(sums[2] - st["maxad"]) <= 1e-8 * st["maxad"]
    assert abs(sums[3] / n - st["target_variance"]) <= 1e-12 * st["target_variance"]
    p.close()


def _random_posterior_case(seed):
    """Posterior paths at a random shape: prediction (means, variances), both covariance families, the covariance
    sampler, training statistics, against the oracle; iso and Cov_se_fat with random option sets; ragged chunks."""
    rng = np.random.default_rng(7000 + seed)
    iso = seed % 2 == 0
    n = int(rng.integers(50, 3000))
    m = int(rng.integers(3, 300))
    d = int(rng.choice([1, 2, 3, 5, 8, 13]))
    nt = int(rng.integers(1, 400))
    s2 = float(10.0 ** rng.uniform(-2, 0))
    chunk_rows = int(rng.choice([0, 128, 256, 1024]))
    if iso:
        X, y, Z = synth(7100 + seed, n, min(m, n), d)
        if m > n:
            Z = np.asfortranarray(np.hstack([Z, rng.normal(size=(d, m - n))]))
        Xt = np.asfortranarray(rng.normal(size=(d, nt)))
        k = O.SeIsoKernel(0.5 * np.log(d) + rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5))
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=chunk_rows)
        args = dict(log_ell=k.log_ell, log_sf2=k.log_sf2)
    else:
        D = d + int(rng.integers(0, 4))
        X = np.asfortranarray(rng.normal(size=(D, n)))
        Xt = np.asfortranarray(rng.normal(size=(D, nt)))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d)) if (D != d or rng.integers(0, 2)) else None
        Z = np.asfortranarray(rng.normal(size=(d, m)) * 0.5)
        het = rng.uniform(-6, -3, size=m) if rng.integers(0, 2) else None
        ms = rng.uniform(-0.5, 0.5, size=(d, m)) if rng.integers(0, 3) == 0 else None
        k = O.SeFatKernel(d, rng.uniform(-0.5, 0.5), P, het, ms)
        p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, d, m, chunk_rows=chunk_rows)
        args = dict(log_sf2=k.log_sf2)
        if P is not None:
            args["tproj"] = P
        if het is not None:
            args["log_hetero_skedasticity"] = het
        if ms is not None:
            args["log_multiscales_m05"] = np.asfortranarray(ms)
    ref = O.evaluate(k, Z, X, y, s2, want_grad=False, keep=True)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(sigma2=s2, inducing=Z, want_grad=False, **args)
    assert abs(ev.l - ref["l"]) <= TOL_L * max(1.0, abs(ref["l"]))
    means, var = p.predict(Xt, predictive=False)
    mref = O.predict_means(k, Z, ref["coeffs"], Xt)
    vref = O.predict_variances(k, Z, ref["model"], Xt, predictive=False)
    scale_m = max(np.max(np.abs(mref)), 1e-3)
    assert np.max(np.abs(means - mref)) <= 1e-7 * scale_m
    assert np.max(np.abs(var - vref)) <= 1e-8 * max(np.max(np.abs(vref)), k.sf2)
    ntc = min(nt, 150)
    fitc = O.fitc_covariances(k, Z, ref["model"], Xt[:, :ntc])
    fic = O.fic_covariances(k, Z, ref["model"], Xt[:, :ntc])
    scale = max(np.max(np.abs(fitc)), np.max(np.abs(fic)), k.sf2)
    cov = p.covariances(Xt[:, :ntc], kind="FITC", predictive=False)
    assert np.max(np.abs(np.triu(cov) - fitc)) <= 1e-8 * scale
    assert np.max(np.abs(np.triu(p.covariances(Xt[:, :ntc], kind="FIC", predictive=False)) - fic)) <= 1e-8 * scale
    z = rng.normal(size=(ntc, 3))
    smp = O.cov_sampler_calc(mref[:ntc], fitc, s2, predictive=True)
    S = p.cov_samples(cov, mref[:ntc], z, add_diag=s2)
    assert np.max(np.abs(S - O.cov_sampler_samples(smp, z))) <= 1e-7 * max(np.max(np.abs(S)), 1.0)
    sums, tm = p.train_stats(want_means=True)
    knm, _ = O.spec_calc_shared_cross(k, X, Z)
    tref = knm @ ref["coeffs"]
    assert np.max(np.abs(tm - tref)) <= 1e-7 * max(np.max(np.abs(tref)), 1e-3)
    assert abs(sums[0] - float(np.sum((y - tref) ** 2))) <= 1e-7 * max(float(np.sum((y - tref) ** 2)), 1e-6)
    p.close()


@pytest.mark.parametrize("seed", range(8))
def test_random_posterior_paths_against_oracle(seed):
    _random_posterior_case(seed)


def test_random_posterior_long_sweep():
    """GPR_FUZZ_POSTERIOR="lo:hi": the same over a seed range (log: profiles/r03_fuzz_posterior.txt)."""
    spec = os.environ.get("GPR_FUZZ_POSTERIOR")
    if not spec:
        pytest.skip("GPR_FUZZ_POSTERIOR not set")
    lo, hi = (int(v) for v in spec.split(":"))
    bad = []
    for seed in range(lo, hi):
        try:
            _random_posterior_case(seed)
        except AssertionError as e:
            bad.append((seed, str(e)[:200]))
    print("random posterior sweep: seeds %d..%d, %d cases, %d failures %s" % (lo, hi - 1, hi - lo, len(bad), bad))
    assert not bad, bad


def test_device_resident_inputs_equal_host_inputs():
    """gprhip_set_inputs_device / gprhip_set_targets_device (inputs already in HBM, point-major [n][D]) give
    bitwise the same evaluation as the host-pointer entry points (Fortran D x n)."""
    import torch
    n, m, d = 5000, 96, 5
    X, y, Z = synth(3, n, m, d)
    hyp = dict(log_ell=0.3, log_sf2=-0.1, sigma2=0.3, inducing=Z)
    a = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=2048)
    a.set_inputs(X)
    a.set_targets(y)
    ea = a.eval(**hyp)
    xd = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda:0")   # [n][D]
    yd = torch.from_numpy(y).to("cuda:0")
    torch.cuda.synchronize()
    b = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=2048)
    b.set_inputs_device(xd.data_ptr())
    b.set_targets_device(yd.data_ptr())
    eb = b.eval(**hyp)
    assert ea.l == eb.l and ea.dl_dsigma2 == eb.dl_dsigma2
    assert np.array_equal(ea.grad, eb.grad) and np.array_equal(ea.coeffs, eb.coeffs)
    a.close()
    b.close()


def test_model_export_import_and_file_flow(tmp_path):
    """Model.calc_co_variance_coeffs (lib/fitc_gp.ml:240) against the oracle's QR factors, a
    predictor rebuilt from stored numbers alone (Mean_predictor.calc / Co_variance_predictor.calc, the `test`
    flow of bin/ocaml_gpr.ml:373-413) against the live model, and the train -> save -> load -> predict flow."""
    from gpr_amd import model_file
    g = load_golden("posterior_fat_all")
    k = oracle_kernel(g)
    s2 = float(g["sigma2"])
    ref = O.evaluate(k, g["Z"], g["X"], g["y"], s2, want_grad=False, keep=True)
    p = _problem_for(g)
    _eval_golden(p, g, want_grad=True)        # a gradient evaluation must leave R~ intact as well
    chol_km, r_mat = p.co_variance_coeffs()
    assert M.vec_ok("chol_km", np.triu(chol_km), np.triu(ref["model"]["inducing"]["chol_km"]), TOL_FACTOR)
    assert M.vec_ok("r_mat", np.triu(r_mat), np.triu(ref["model"]["r_mat"]), TOL_FACTOR)
    assert np.all(np.tril(chol_km, -1) == 0.0) and np.all(np.tril(r_mat, -1) == 0.0)
    means, var = p.predict(g["Xt"], predictive=False)
    cov = p.covariances(g["Xt"], kind="FIC", predictive=False)
    coeffs = ref["coeffs"]
    p.close()
    # a fresh problem that never sees the training data
    D, nt = g["Xt"].shape
    d, m = g["Z"].shape
    q = gpr_amd.Problem(gpr_amd.COV_SE_FAT, nt, D, d, m)
    args = dict(log_sf2=float(g["log_sf2"]), sigma2=s2, inducing=g["Z"], tproj=g["tproj"],
                log_hetero_skedasticity=g["log_hetero"], log_multiscales_m05=g["log_multiscales"])
    q.load_predictor(coeffs=coeffs, co_variance_coeffs=(chol_km, r_mat), **args)
    means2, var2 = q.predict(g["Xt"], predictive=False)
    assert M.vec_ok("pred_mean", means2, g["means"], TOL_POST) and M.vec_ok("pred_mean", means2, means, 1e-10)
    assert M.vec_ok("pred_var", var2, g["variances"], TOL_POST) and M.vec_ok("pred_var", var2, var, 1e-9)
    assert M.vec_ok("pred_var", q.covariances(g["Xt"], kind="FIC", predictive=False), cov, 1e-9)
    u2, r2 = q.co_variance_coeffs()            # what was loaded comes back out
    assert M.vec_ok("chol_km", u2, chol_km, 1e-12) and M.vec_ok("r_mat", r2, r_mat, 1e-10)
    q.load_predictor(coeffs=coeffs, **args)    # means only
    assert M.vec_ok("pred_mean", q.predict(g["Xt"], want_variances=False)[0], means, 1e-10)
    with pytest.raises(gpr_amd.GprHipError):
        q.predict(g["Xt"])
    q.close()

    # file flow on the 1-D recipe of test/gen_data.ml: samples as text, train, save, load, predict
    gd = load_golden("iso_gen_data")
    text = "".join("%.17g,%.17g\n" % (x, t) for x, t in zip(gd["X"][0], gd["y"]))
    inputs, targets = model_file.read_training_samples(text)
    assert np.array_equal(inputs, gd["X"]) and np.array_equal(targets, gd["y"])
    # the tool standardises every input dimension to unit *norm* (bin/ocaml_gpr.ml:254-265), so the unit-length
    # Cov_se_fat kernel needs its learnt projection (-dim-red) to see any structure
    model = model_file.train(inputs, targets, n_inducing=10, sigma2=1.0, dim_red=1, max_iter=60,
                             rng=np.random.default_rng(4))
    assert model.stats.rmse < 0.8 and 0.3 < model.sigma2 < 0.8     # noise sigma 0.7
    path = tmp_path / "model.npz"
    model_file.save_model(path, model)
    loaded = model_file.load_model(path)
    xt = np.linspace(-4.5, 4.5, 56)[None, :]     # even count: no sample at x = 0
    mu, sd = model_file.predict(loaded, xt, with_stddev=True)
    # the same numbers straight from the oracle with the stored hyper-parameters
    kp = loaded.kernel.params
    ok = O.SeFatKernel(kp.d, kp.log_sf2, kp.tproj, kp.log_hetero_skedasticity, kp.log_multiscales_m05)
    xs = model_file.apply_standardization(inputs, loaded.input_means, loaded.input_stddevs)
    oref = O.evaluate(ok, loaded.inducing_points, xs, targets - loaded.target_mean, loaded.sigma2,
                      variational=True, want_grad=False, keep=True)
    xts = model_file.apply_standardization(xt, loaded.input_means, loaded.input_stddevs)
    mu_ref = O.predict_means(ok, loaded.inducing_points, oref["coeffs"], xts) + loaded.target_mean
    var_ref = O.predict_variances(ok, loaded.inducing_points, oref["model"], xts, predictive=True)
    assert M.vec_ok("mu_ref", mu, mu_ref, 1e-7) and M.vec_ok("pred_var", sd, np.sqrt(var_ref), 1e-7)
    lines = model_file.format_predictions(mu, sd).splitlines()
    assert len(lines) == 56 and all(len(ln.split(",")) == 2 for ln in lines)
    truth = np.sin(3 * xt[0]) / xt[0] + np.abs(xt[0] - 3) / (xt[0] ** 2 + 1)
    assert np.sqrt(np.mean((mu - truth) ** 2)) < 0.35


def _oracle_gradient(k, Z, X, y, s2):
    out = O.evaluate_fast(k, Z, X, y, s2)
    return out["l"], np.concatenate([[out["dl_dsigma2"] * s2], out["grad"]])


def test_sgd_and_smd_drivers_follow_the_oracle_trajectory():
    """Optim.SGD / Optim.SMD (lib/fitc_gp.ml:1724-2017) mirrored over the device gradient, against the same update
    rules driven by the oracle's gradient: three SGD steps, two SMD steps (central-difference Hessian-vector
    product), plus make_test's best-state bookkeeping."""
    from gpr_amd import optim
    n, m, d = 600, 12, 2
    X, y, Z = synth(29, n, m, d)
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(0.2, 0.1))

    def unpack(vals):
        return O.SeIsoKernel(vals[0], vals[1]), np.asfortranarray(vals[2:].reshape(m, d).T)

    # ---- SGD
    t = optim.SGD.create(F, cov_se_iso, kernel, Z, X, y, tau=10.0, eta0=1e-4, sigma2=0.3)
    vals = np.concatenate([[0.2, 0.1], Z.T.ravel()])
    s2, eta = 0.3, 1e-4
    _, g = _oracle_gradient(*unpack(vals), X, y, s2)
    assert relinf(t.gradient, g) <= 1e-7 and abs(t.gradient_norm - np.linalg.norm(g)) <= 1e-7 * np.linalg.norm(g)
    for step in range(3):
        t = optim.SGD.step(t)
        s2 = float(np.exp(np.log(s2) + eta * g[0]))
        vals = vals + eta * g[1:]
        eta = 10.0 / (10.0 + step) * eta
        le, g = _oracle_gradient(*unpack(vals), X, y, s2)
        assert abs(t.sigma2 - s2) <= 1e-9 * s2 and relinf(t.hyper_vals, vals) <= 1e-9
        assert abs(t.eta - eta) <= 1e-15 and t.step_no == step + 1
        assert M.rel_ok("l", t.log_evidence(), le, 1e-8) and relinf(t.gradient, g) <= 1e-6
    best = optim.SGD.test(optim.SGD.create(F, cov_se_iso, kernel, Z, X, y, tau=10.0, eta0=1e-4, sigma2=0.3),
                          epsabs=1e-3, max_iter=3)
    assert best.log_evidence() >= t.log_evidence() - 1e-9 * abs(t.log_evidence())   # ascent: later is better
    with pytest.raises(ValueError, match="tau"):
        optim.SGD.create(F, cov_se_iso, kernel, Z, X, y, tau=0.0)

    # ---- SMD
    eps, lam, mu = 1e-4, 0.1, 1e-3
    t = optim.SMD.create(F, cov_se_iso, kernel, Z, X, y, eps=eps, sigma2=0.3, eta0=np.full(3 + m * d, 2e-4))
    vals = np.concatenate([[0.2, 0.1], Z.T.ravel()])
    s2 = 0.3
    eta = np.full(3 + m * d, 2e-4)
    nu = np.full(3 + m * d, 1e-3)
    nh = 2 + m * d
    _, g = _oracle_gradient(*unpack(vals), X, y, s2)
    for _ in range(2):
        t = optim.SMD.step(t)
        gp = _oracle_gradient(*unpack(vals + eps * nu[1:]), X, y, float(np.exp(np.log(s2) + eps * nu[0])))[1]
        gm = _oracle_gradient(*unpack(vals - eps * nu[1:]), X, y, float(np.exp(np.log(s2) - eps * nu[0])))[1]
        lhn = lam / (2 * eps) * (gp - gm)
        new_eta = eta * np.maximum(0.5, 1.0 + mu * g * nu)
        new_s2 = float(np.exp(np.log(s2) + new_eta[0] * g[0]))
        new_vals = vals + new_eta[:nh] * g[1:1 + nh]
        nu = eta * (g + lhn) + lam * nu
        eta, s2, vals = new_eta, new_s2, new_vals
        _, g = _oracle_gradient(*unpack(vals), X, y, s2)
        assert relinf(t.eta, eta) <= 1e-9 and abs(t.sigma2 - s2) <= 1e-9 * s2
        assert relinf(t.hyper_vals, vals) <= 1e-9 and relinf(t.gradient, g) <= 1e-6
        assert relinf(t.nu, nu) <= 1e-3      # carries the finite-difference noise of both sides
    with pytest.raises(ValueError, match="lambda"):
        optim.SMD.create(F, cov_se_iso, kernel, Z, X, y, lam=1.5)
    GP.close()


def _run_mirror_check(tmp_path, g, Xt, variational):
    """Dump a fixture for tests/cpp/mirror_check.cpp (built by gpr_amd/csrc/Makefile), run it, parse its lines."""
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "gpr_amd", "_build", "mirror_check")
    assert os.path.exists(exe), "mirror_check not built (make -C gpr_amd/csrc)"
    X, Z = np.asfortranarray(g["X"]), np.asfortranarray(g["Z"])
    D, n = X.shape
    d, m = Z.shape
    iso = g["kind"] == "iso"
    path = tmp_path / "dump.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<10q", 0 if iso else 1, n, D, d, m, Xt.shape[1], int("tproj" in g), int("log_hetero" in g),
                            int("log_multiscales" in g), int(variational)))
        f.write(struct.pack("<3d", float(g["log_ell"]) if iso else 0.0, float(g["log_sf2"]), float(g["sigma2"])))
        arrays = [X, g["y"], Z]
        arrays += [g[key] for key in ("tproj", "log_hetero", "log_multiscales") if key in g]
        arrays.append(Xt)
        for a in arrays:
            f.write(np.asfortranarray(a, dtype=np.float64).tobytes(order="F"))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    if out.stderr:
        print(out.stderr[-2000:])  # shown by pytest when an assertion on the parsed results fails
    res = {}
    for line in out.stdout.splitlines():
        key, *vals = line.split()
        res[key] = np.array([float(v) for v in vals])
    return res


def test_c_abi_from_a_plain_c_program():
    """tests/cpp/eval_latency.c (C99, the header included as C) creates a problem, evaluates with and without the
    gradient and destroys it: both entry forms return the same evidence, and no Python is involved."""
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpr_amd", "_build", "eval_latency")
    if not os.path.exists(exe):
        pytest.fail("gpr_amd/_build/eval_latency missing: run __graft_entry__.build()")
    out = subprocess.run([exe, "1500", "40", "2", "6"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    ls = [float(v) for v in re.findall(r"l = (-?[0-9.]+)", out.stdout)]
    assert len(ls) == 2 and abs(ls[0] - ls[1]) <= 1e-6 * abs(ls[0]), out.stdout


@pytest.mark.parametrize("name", ["iso_c1_var", "posterior_fat_all"])
def test_cpp_host_mirror(tmp_path, name):
    """include/gprhip.hpp -- the C++ mirror of Fitc_gp.Make_deriv(Spec).{FITC, Variational_FITC, FIC,
    Variational_FIC} over the C ABI -- driven by a compiled program and compared with the oracle: evidence,
    per-hyper derivative lookups in Hyper.get_all order, model-only derivatives, Optim.calc_gradient, Stats,
    prediction, covariances, co-variance coefficients, update_sigma2, the self-test recipe and error messages."""
    g = load_golden(name)
    variational = bool(g.get("variational", False))
    k = oracle_kernel(g)
    s2 = float(g["sigma2"])
    Xt = g["Xt"] if "Xt" in g else np.asfortranarray(np.random.default_rng(1).normal(size=(g["X"].shape[0], 40)))
    res = _run_mirror_check(tmp_path, g, Xt, variational)
    ref = O.evaluate(k, g["Z"], g["X"], g["y"], s2, variational=variational, keep=True)
    assert M.rel_ok("l1", res["l1"][0], ref["l1"], TOL_L)
    assert M.rel_ok("l", res["l"][0], ref["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", res["dl_dsigma2"][0], ref["dl_dsigma2"], TOL_DS2)
    assert M.rel_ok("model_dl_dsigma2", res["model_dl_dsigma2"][0], ref["model_dl_dsigma2"], TOL_DS2)
    assert res["grad"].shape == ref["grad"].shape and M.grad_ok(res["grad"], ref["grad"], M.families_golden(g), TOL_GRAD)
    assert M.grad_ok(res["model_grad"], ref["model_grad"], M.families_golden(g), TOL_GRAD, "model_grad")
    assert M.vec_ok("coeffs", res["coeffs"], ref["coeffs"], TOL_COEFF)
    # Optim.calc_gradient: [dl/dlog sigma2; hypers in Hyper.get_all order] (lib/fitc_gp.ml:1674-1694)
    assert M.rel_ok("dl_dlogsigma2", res["optim_gradient"][0], ref["dl_dsigma2"] * s2, TOL_DS2)
    assert M.grad_ok(res["optim_gradient"][1:], ref["grad"], M.families_golden(g), TOL_GRAD)
    knm, _ = O.spec_calc_shared_cross(k, g["X"], g["Z"])
    tm = knm @ ref["coeffs"]
    st = O.stats_calc(g["y"], tm, ref["l"])
    assert M.vec_ok("pred_mean", res["train_means"], tm, TOL_POST)
    assert M.vec_ok("stats", res["stats"], [st[key] for key in STAT_KEYS], TOL_POST)
    assert M.vec_ok("pred_mean", res["means"], O.predict_means(k, g["Z"], ref["coeffs"], Xt), TOL_POST)
    var = O.predict_variances(k, g["Z"], ref["model"], Xt, predictive=False)
    assert M.vec_ok("pred_var", res["variances"], var, TOL_POST) and M.vec_ok("pred_var", res["variances_predictive"], var + s2, TOL_POST)
    nt = Xt.shape[1]
    cref = (O.fitc_covariances if g["kind"] == "iso" else O.fic_covariances)(k, g["Z"], ref["model"], Xt)
    cov = res["cov"].reshape(nt, nt)
    assert np.max(np.abs(np.triu(cov) - cref)) <= 1e-8 * np.max(np.abs(cref))
    m = g["Z"].shape[1]
    assert M.vec_ok("chol_km", np.triu(res["chol_km"].reshape(m, m).T), np.triu(ref["model"]["inducing"]["chol_km"]), TOL_FACTOR)
    assert M.vec_ok("r_mat", np.triu(res["r_mat"].reshape(m, m).T), np.triu(ref["model"]["r_mat"]), TOL_FACTOR)
    ref2 = O.evaluate(k, g["Z"], g["X"], g["y"], 2 * s2, variational=variational, want_grad=False)
    assert M.rel_ok("l", res["l_sigma2x2"][0], ref2["l"], TOL_L)
    mean_ref = O.predict_means(k, g["Z"], ref["coeffs"], Xt)
    assert M.vec_ok("pred_mean", res["standalone_means"], mean_ref, TOL_POST)
    assert M.vec_ok("pred_var", res["standalone_variances"], var, TOL_POST)
    zz = np.stack([np.sin(1.0 + np.arange(nt)), np.cos(2.0 * np.arange(nt))], axis=1)
    smp = O.cov_sampler_calc(mean_ref, O.fitc_covariances(k, g["Z"], ref["model"], Xt), s2, predictive=True)
    assert M.vec_ok("samples", res["samples"].reshape(2, nt).T, O.cov_sampler_samples(smp, zz), TOL_POST)
    assert res["phys_equal_check"][0] == 1.0 and res["self_test"][0] == 1.0
    assert np.array_equal(res["error_checks"], [1.0, 1.0])


def test_hip_path_against_snelson_spgp_lik():
    """The HIP path against Edward Snelson's SPGP routine (test/spgp_lik.m, restated in oracle/snelson_spgp.py) at the
    BASELINE C1 shape -- the external cross-check the reference's own test/oct.m:183-191 performs."""
    from oracle.snelson_spgp import spgp_lik
    g = load_golden("iso_c1")
    X, y, Z = g["X"], g["y"], g["Z"]
    d, m = Z.shape
    log_ell, log_sf2, s2 = float(g["log_ell"]), float(g["log_sf2"]), float(g["sigma2"])
    p = _problem_for(g)
    ev = _eval_golden(p, g)
    p.close()
    ew = np.concatenate([Z.T.ravel(order="F"), np.full(d, -2.0 * log_ell), [log_sf2, np.log(s2)]])
    fw, dfw = spgp_lik(ew, y, np.ascontiguousarray(X.T), m)
    assert abs(ev.l - (-fw)) <= 1e-9 * abs(fw)
    scale = np.max(np.abs(ev.grad))
    assert abs(ev.grad[0] - 2.0 * np.sum(dfw[m * d:m * d + d])) <= 1e-7 * scale
    assert abs(ev.grad[1] + dfw[-2]) <= 1e-7 * scale
    assert abs(ev.dl_dsigma2 + dfw[-1] / s2) <= 1e-7 * abs(ev.dl_dsigma2)
    assert np.max(np.abs(ev.grad[2:].reshape(m, d) + dfw[:m * d].reshape(m, d, order="F"))) <= 1e-7 * scale


@pytest.mark.parametrize("name", illcond_golden_names())
def test_ill_conditioned_regime(name):
    """ell = e: K_m is jitter-dominated (cond(K_m + 1e-6 I) ~ 1e7 .. 4e7), sigma2 = 1e-4 and 1.  Forming
    B = K_m + K_mn S^-1 K_nm and factoring it loses 1e-5 here -- the reason the reference runs a
    Householder QR of the stacked matrix (lib/fitc_gp.ml:170-182).  The device path's whitened B~ = I + V^T S^-1 V must
    hold the oracle's accuracy: against the oracle at the C1 shape, and against a 40-digit evaluation on the small case.
    Stated tolerances for this regime: l 1e-10, dl/dsigma2 1e-9, gradient and coefficients 1e-8
    (relative, max-norm); l1 / l2 against the 40-digit values 1e-10.  Measured on MI355X: l <= 3e-12, dl/dsigma2 <= 7e-12,
    gradient <= 2e-10, coefficients <= 3e-10."""
    g = load_golden(name)
    p = _problem_for(g)
    ev = _eval_golden(p, g)
    p.close()
    assert M.rel_ok("l", ev.l, float(g["l"]), 1e-10)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, float(g["dl_dsigma2"]), 1e-9)
    assert M.grad_ok(ev.grad, g["grad"], M.families_golden(g), 1e-8)
    assert M.vec_ok("coeffs", ev.coeffs, g["coeffs"], 5e-9)
    if "mp_l1" in g:
        assert M.rel_ok("l1", ev.l1, float(g["mp_l1"]), 1e-10)
        assert M.rel_ok("l2", ev.l2, float(g["mp_l2"]), 1e-10)
        assert M.vec_ok("coeffs", ev.coeffs, g["mp_coeffs"], 5e-9)
    print("illcond %s: l %.2e  ds2 %.2e  grad %.2e  coeffs %.2e" % (
        name, abs(ev.l - float(g["l"])) / abs(float(g["l"])),
        abs(ev.dl_dsigma2 - float(g["dl_dsigma2"])) / abs(float(g["dl_dsigma2"])), relinf(ev.grad, g["grad"]),
        relinf(ev.coeffs, g["coeffs"])))


def _fd_directional(p, hyp, a, le_key, extra_dirs, rng, eps=1e-4):
    """Directional derivative of the device log evidence by central differences against the analytic gradient."""
    Z = hyp["inducing"]
    dz = rng.normal(size=Z.shape)
    dz /= np.linalg.norm(dz)
    dls, ds2 = -0.2, 0.05
    plus, minus = dict(hyp), dict(hyp)
    plus.update(log_sf2=hyp["log_sf2"] + eps * dls, sigma2=hyp["sigma2"] + eps * ds2, inducing=Z + eps * dz)
    minus.update(log_sf2=hyp["log_sf2"] - eps * dls, sigma2=hyp["sigma2"] - eps * ds2, inducing=Z - eps * dz)
    analytic = a.dl_dsigma2 * ds2
    for key, direction, grad_slice in extra_dirs:
        plus[key] = hyp[key] + eps * direction
        minus[key] = hyp[key] - eps * direction
        analytic += float(np.sum(grad_slice * direction))
    fd = (p.eval(want_grad=False, **plus).l - p.eval(want_grad=False, **minus).l) / (2 * eps)
    return fd, analytic, dls, dz


def test_c4_shard_size_properties():
    """BASELINE.json configs[3] (cov_se_iso, n=8M, m=4096, d=16 over 8 GPUs): one GPU's shard at full size
    (n=1M rows, m=4096, d=16, fp64).  Size-independent properties: run-to-run bitwise determinism, evidence-only ==
    gradient-mode evidence, directional derivative against a central difference of device evaluations."""
    n, m, d = 1_000_000, 4096, 16
    X, y, Z = synth(4, n, m, d)
    le = 0.5 * np.log(d)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    hyp = dict(log_ell=le, log_sf2=0.0, sigma2=0.1, inducing=Z)
    a = p.eval(**hyp)
    b = p.eval(**hyp)
    assert a.l == b.l and np.array_equal(a.grad, b.grad)
    assert np.isfinite(a.l) and np.all(np.isfinite(a.grad)) and a.grad.shape == (2 + d * m,)
    assert abs(p.eval(want_grad=False, **hyp).l - a.l) <= 1e-12 * abs(a.l)
    rng = np.random.default_rng(0)
    fd, analytic, dls, dz = _fd_directional(p, hyp, a, "log_ell", [("log_ell", 0.3, a.grad[0:1])], rng)
    analytic += a.grad[1] * dls + float(a.grad[2:] @ dz.T.reshape(-1))
    assert abs(fd - analytic) <= 1e-5 * max(abs(analytic), abs(a.l) * 1e-6)
    p.close()


def test_c3_full_size_properties():
    """BASELINE.json configs[2] at full size: cov_se_fat as ARD (tproj = diag(1/ell_i)), n=1M, m=4096, d=D=32.
    fp64: determinism, evidence-only == gradient-mode evidence, directional derivative (inducing points, log sf2,
    sigma2 and the whole projection matrix) against central differences.  fp32 bulk (the configuration BASELINE names):
    determinism, and agreement with the fp64 run inside the stated fp32-bulk tolerances (l 1e-4, gradient and
    coefficients 5e-3, max-norm relative)."""
    n, m, d = 1_000_000, 4096, 32
    rng = np.random.default_rng(3)
    X = np.asfortranarray(rng.normal(size=(d, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    ell = rng.uniform(-0.5, 0.5, size=d)
    P = np.asfortranarray(np.diag(np.exp(-ell)) / np.sqrt(d))
    Z = np.asfortranarray((P.T @ X[:, rng.permutation(n)[:m]]) + 0.01 * rng.normal(size=(d, m)))
    hyp = dict(log_sf2=0.0, sigma2=0.1, inducing=Z, tproj=P)
    p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    a = p.eval(**hyp)
    b = p.eval(**hyp)
    assert a.l == b.l and np.array_equal(a.grad, b.grad)
    assert a.grad.shape == (1 + d * m + d * d,) and np.all(np.isfinite(a.grad))
    assert abs(p.eval(want_grad=False, **hyp).l - a.l) <= 1e-12 * abs(a.l)
    dP = rng.normal(size=P.shape)
    dP /= np.linalg.norm(dP) * 10.0
    proj_grad = a.grad[1 + d * m:].reshape(d, d)   # Proj {big; small}, big-major
    fd, analytic, dls, dz = _fd_directional(p, hyp, a, None, [("tproj", dP, proj_grad)], np.random.default_rng(0))
    analytic += a.grad[0] * dls + float(a.grad[1:1 + d * m] @ dz.T.reshape(-1))
    assert abs(fd - analytic) <= 1e-5 * max(abs(analytic), abs(a.l) * 1e-6)
    p.close()
    q = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, d, d, m, precision=gpr_amd.F32_BULK)
    q.set_inputs(X)
    q.set_targets(y)
    c = q.eval(**hyp)
    c2 = q.eval(**hyp)
    q.close()
    assert c.l == c2.l and np.array_equal(c.grad, c2.grad)
    assert M.rel_ok("l", c.l, a.l, TOL32_L)
    assert M.grad_ok(c.grad, a.grad, M.families("fat", d, m, D=d, proj=True), TOL32_GRAD) and M.vec_ok("coeffs", c.coeffs, a.coeffs, TOL32_COEFF)
    print("C3 fp32-bulk vs fp64 at full size: l %.2e  grad %.2e  coeffs %.2e" % (
        abs(c.l - a.l) / abs(a.l), relinf(c.grad, a.grad), relinf(c.coeffs, a.coeffs)))


def test_parity_at_4096_inducing_points():
    """Oracle parity at m = 4096 (configs[2] / [3]): cov_se_iso d=16 against the C restatement of the reference's
    LAPACK sequence (oracle/fitc_ref.c) on 24 000 rows, cov_se_fat ARD d=32 (fp64 and fp32 bulk) against the numpy
    oracle on 6 000 rows."""
    from oracle import fitc_ref as R
    n, m, d = 24000, 4096, 16
    X, y, Z = synth(4, n, m, d)
    le = 0.5 * np.log(d)
    ref = R.iso_eval(X, y, Z, le, 0.0, 0.1)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=le, log_sf2=0.0, sigma2=0.1, inducing=Z)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
    assert ev.grad.shape == (2 + m * d,) and M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD)
    assert M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)
    rng = np.random.default_rng(3)
    n, d = 6000, 32
    X = np.asfortranarray(rng.normal(size=(d, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    ell = rng.uniform(-0.5, 0.5, size=d)
    P = np.asfortranarray(np.diag(np.exp(-ell)) / np.sqrt(d))
    k = O.SeFatKernel(d, 0.0, P)
    Z = np.asfortranarray(O.se_fat_project(k, X[:, rng.permutation(n)[:m]]) + 0.01 * rng.normal(size=(d, m)))
    ref = O.evaluate_fast(k, Z, X, y, 0.1)
    for prec, tl, tg in ((gpr_amd.F64, TOL_L, TOL_GRAD), (gpr_amd.F32_BULK, TOL32_L, TOL32_GRAD)):
        p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, d, d, m, precision=prec)
        p.set_inputs(X)
        p.set_targets(y)
        ev = p.eval(log_sf2=0.0, sigma2=0.1, inducing=Z, tproj=P)
        p.close()
        assert M.rel_ok("l", ev.l, ref["l"], tl)
        assert M.grad_ok(ev.grad, ref["grad"], M.families("fat", d, m, D=d, proj=True), tg)


def test_parity_at_headline_inducing_count():
    """Oracle parity at the headline m and d (2048, 8) on as many rows as the oracle evaluates in well under a
    minute on the GPU box's host cores: two row chunks, the split-K factor search, the full 16 387-entry gradient."""
    n, m, d = 40000, 2048, 8
    X, y, Z = synth(2, n, m, d)
    le = 0.5 * np.log(d)
    ref = O.evaluate_fast(O.SeIsoKernel(le, 0.0), Z, X, y, 0.1)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=le, log_sf2=0.0, sigma2=0.1, inducing=Z)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
    assert ev.grad.shape == (2 + m * d,) and M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD)
    assert M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)


@pytest.mark.parametrize("name", ["iso_ragged", "fat_proj", "fat_hetero"])
def test_scalar_and_mfma_gradient_kernels_agree(name, monkeypatch):
    """The fused gradient pass exists twice: on the matrix cores (grad_mfma.hip: distance and inducing-gradient
    products as MFMA tiles, |p - z|^2 by expansion) and as the scalar kernel that multiscales still need
    (rowops.hip, direct differences).  Both must meet the oracle tolerance and agree with each other."""
    g = load_golden(name)
    monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")  # these switches belong to the engine's row passes
    monkeypatch.setenv("GPRHIP_MID_PATH", "0")
    p = _problem_for(g)
    a = _eval_golden(p, g)
    p.close()
    monkeypatch.setenv("GPRHIP_GRAD_SCALAR", "1")
    q = _problem_for(g)
    b = _eval_golden(q, g)
    q.close()
    assert M.grad_ok(a.grad, g["grad"], M.families_golden(g), TOL_GRAD) and M.grad_ok(b.grad, g["grad"], M.families_golden(g), TOL_GRAD)
    assert M.grad_ok(a.grad, b.grad, M.families_golden(g), 1e-9)
    assert a.l == b.l


@pytest.mark.parametrize("name", ["fat_proj", "fat_hetero", "fat_proj_var"])
def test_resident_and_recomputed_covariance_gradient_passes_agree(name, monkeypatch):
    """Cov_se_fat with projection hypers keeps K_nm of pass 1 on the device when there is room and the gradient kernel
    reads E = X .* K (grad_mfma.hip, KR) instead of recomputing distances and exp; GPRHIP_K_RESIDENT=0 forces the
    recomputing kernel.  Both meet the oracle tolerance, agree with each other, and sigma2-only re-evaluations
    (update_sigma2: V, r and K reused) go through the kept K as well."""
    g = load_golden(name)
    if "tproj" not in g:
        pytest.skip("no projection hypers in this fixture")
    monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")  # these switches belong to the engine's row passes
    monkeypatch.setenv("GPRHIP_MID_PATH", "0")
    p = _problem_for(g)
    a = _eval_golden(p, g)
    a2 = _eval_golden(p, g, sigma2=2.0 * float(g["sigma2"]), reuse_v=True)
    p.close()
    monkeypatch.setenv("GPRHIP_K_RESIDENT", "0")
    q = _problem_for(g)
    b = _eval_golden(q, g)
    b2 = _eval_golden(q, g, sigma2=2.0 * float(g["sigma2"]), reuse_v=True)
    q.close()
    assert M.grad_ok(a.grad, g["grad"], M.families_golden(g), TOL_GRAD) and M.grad_ok(b.grad, g["grad"], M.families_golden(g), TOL_GRAD)
    assert M.grad_ok(a.grad, b.grad, M.families_golden(g), 1e-9) and M.grad_ok(a2.grad, b2.grad, M.families_golden(g), 1e-9)
    assert a.l == b.l and a2.l == b2.l


@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (2, 1, 3), (3, 7, 2), (129, 128, 4), (128, 129, 4), (127, 257, 1)])
def test_degenerate_and_tile_boundary_shapes(n, m, d):
    """One training point, one inducing point, more inducing than training points, sizes one off the 128-tile: every
    padded row and column must stay out of the sums (Cov_se_iso evidence + full gradient, standard and variational)."""
    rng = np.random.default_rng(100 * n + m)
    X = np.asfortranarray(rng.normal(size=(d, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    Z = np.asfortranarray(rng.normal(size=(d, m)))
    k = O.SeIsoKernel(0.1, -0.2)
    for variational in (False, True):
        ref = O.evaluate(k, Z, X, y, 0.3, variational=variational)
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
        p.set_inputs(X)
        p.set_targets(y)
        ev = p.eval(log_ell=0.1, log_sf2=-0.2, sigma2=0.3, inducing=Z, variational=variational)
        cond = p.condition()[0]
        p.close()
        assert M.rel_ok("l", ev.l, ref["l"], TOL_L, floor=1.0)
        assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2, floor=1.0)
        assert ev.grad.shape == ref["grad"].shape
        assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD, cond=cond)
        assert np.max(np.abs(ev.coeffs - ref["coeffs"])) <= TOL_COEFF * max(1.0, np.max(np.abs(ref["coeffs"])))


@pytest.mark.parametrize("name", ["iso_c1", "iso_ragged", "iso_c1_var", "fat_proj", "fat_all", "illcond_c1_hi", "illcond_small_lo"])
def test_two_phase_and_two_launch_x_products_agree(name, monkeypatch):
    """X = diag(is) Q' R^-T - diag(v) V U^-T - w t^T comes from one launch of two-phase engine items on large shards
    (from 48 m training points on) and from X~, X = X~ U^-T otherwise; GPRHIP_MERGED_X=2 / 0 force either.  Both meet the
    fixture's tolerance (the ill-conditioned ones included) and agree with each other."""
    g = load_golden(name)
    tol = 1e-8 if name.startswith("illcond") else TOL_GRAD
    res = {}
    monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")  # these switches belong to the engine's row passes
    monkeypatch.setenv("GPRHIP_MID_PATH", "0")
    for mode in ("2", "0"):
        monkeypatch.setenv("GPRHIP_MERGED_X", mode)
        p = _problem_for(g, chunk_rows=512)  # the switch is read when the problem is created
        p.set_timing(2)
        res[mode] = _eval_golden(p, g)
        stages = set(p.last_timings())
        p.close()
        # the switch must have selected the code path (it used to be a load-time static no test could toggle)
        if mode == "2":
            assert "p2_trmm_SX" in stages and "p2_trmm_S" not in stages, stages
        else:
            assert {"p2_trmm_S", "p2_trmm_X"} <= stages and "p2_trmm_SX" not in stages, stages
        assert M.grad_ok(res[mode].grad, g["grad"], M.families_golden(g), tol), mode
        assert M.rel_ok("dl_dsigma2", res[mode].dl_dsigma2, g["dl_dsigma2"], TOL_DS2)
    assert res["2"].l == res["0"].l
    assert M.grad_ok(res["2"].grad, res["0"].grad, M.families_golden(g), 1e-8 if name.startswith("illcond") else 1e-10)


@pytest.mark.parametrize("m", [300, 700])
def test_opt_in_factorisation_variants_are_bit_identical(m, tmp_path):
    """Round 5 built two alternatives to the three-launches-per-step factorisation of K_m + jitter and B~ (chol.hip):
    ONE persistent launch with device-side dependencies (GPRHIP_POTRF_CHAIN=1) and a look-ahead split of every step's
    trailing update over two streams (GPRHIP_POTRF_LOOKAHEAD=n).  Both measured slower ("Round 5") and
    since round 6 live in the LAB build only (libgprhip_lab.so, `make -C gpr_amd/csrc lab`, GPRHIP_LIBRARY=lab; the production
    library carries one factorisation and ignores the switches), but they apply the same tile updates in the same order:
    whole evaluations through them return the very same numbers as the production library's (each variant in a fresh
    interpreter, since the library is chosen when gpr_amd first loads it)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lab = os.path.join(root, "gpr_amd", "libgprhip_lab.so")
    if not os.path.exists(lab):
        subprocess.run(["make", "-C", os.path.join(root, "gpr_amd", "csrc"), "-j8", "lab"], capture_output=True, timeout=1800)
    assert os.path.exists(lab), "gpr_amd/libgprhip_lab.so not built (make -C gpr_amd/csrc lab)"
    n, d = 4000, 5
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import torch, gpr_amd\n"
        "from tests.util import synth\n"
        "n, m, d = %d, %d, %d\n"
        "X, y, Z = synth(900 + m, n, m, d)\n"
        "p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)\n"
        "p.set_inputs(X); p.set_targets(y)\n"
        "ev = p.eval(log_ell=0.5 * np.log(d), log_sf2=0.1, sigma2=0.05, inducing=Z)\n"
        "assert gpr_amd._lib.LIB_PATH.endswith(sys.argv[2]), gpr_amd._lib.LIB_PATH\n"
        "np.savez(sys.argv[1], l=ev.l, ds2=ev.dl_dsigma2, grad=ev.grad, coeffs=ev.coeffs)\n") % (root, n, m, d)
    res = {}
    for tag, env in (("production", {}), ("lab", {"GPRHIP_LIBRARY": "lab"}),
                     ("chain", {"GPRHIP_LIBRARY": "lab", "GPRHIP_POTRF_CHAIN": "1"}),
                     ("lookahead", {"GPRHIP_LIBRARY": "lab", "GPRHIP_POTRF_LOOKAHEAD": "1"}),
                     ("ignored", {"GPRHIP_POTRF_CHAIN": "1", "GPRHIP_POTRF_LOOKAHEAD": "1", "GPRHIP_COV_OVERLAP": "1"})):
        out_file = str(tmp_path / (tag + ".npz"))
        want = "libgprhip_lab.so" if env.get("GPRHIP_LIBRARY") == "lab" else "libgprhip.so"
        run = subprocess.run([sys.executable, "-c", code, out_file, want], capture_output=True, text=True, timeout=600,
                             env=dict({k: v for k, v in os.environ.items() if not k.startswith("GPRHIP_")}, **env))
        assert run.returncode == 0, (tag, run.stderr[-1500:])
        res[tag] = np.load(out_file)
    X, y, Z = synth(900 + m, n, m, d)
    ref = O.evaluate_fast(O.SeIsoKernel(0.5 * np.log(d), 0.1), Z, X, y, 0.05)
    assert M.rel_ok("l", float(res["production"]["l"]), ref["l"], TOL_L)
    for tag in ("lab", "chain", "lookahead", "ignored"):
        assert res[tag]["l"] == res["production"]["l"] and res[tag]["ds2"] == res["production"]["ds2"], tag
        assert np.array_equal(res[tag]["grad"], res["production"]["grad"]), tag
        assert np.array_equal(res[tag]["coeffs"], res["production"]["coeffs"]), tag


@pytest.mark.parametrize("n,m,d,log_ell,tol", [(2630, 176, 1, -0.0496, 3e-7), (2034, 432, 1, -0.1, 3e-7),
                                                (3000, 540, 4, 0.55, 2e-8), (3488, 171, 32, 1.8, 1e-12)])
def test_mean_coefficients_against_an_80_bit_evaluation(n, m, d, log_ell, tol):
    """Evidence and mean coefficients of the device path against the x87 long-double evaluation of tests/util.py, over
    several 128-blocks of inducing points.  The n x m products run against explicit triangular inverses (DESIGN.md
    section 3): where K_m is jitter-dominated (points on a line, length scale ~ 1) that costs digits on the
    coefficients -- 1.1e-7 measured at (2630, 176, 1), where the reference's trsm sequence (the oracle) keeps 2e-9; from a
    few dimensions on the device path is at or below the oracle's own distance from the 80-bit values (1e-9 .. 1e-14)."""
    from tests.util import longdouble_fitc
    X, y, Z = synth(5000 + n, n, m, d)
    Xt = np.asfortranarray(np.random.default_rng(6).normal(size=(d, 200)))
    l, t, mean, var = longdouble_fitc(X, y, Z, log_ell, 0.1, 0.05, Xt=Xt)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=1024)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=log_ell, log_sf2=0.1, sigma2=0.05, inducing=Z, want_grad=False)
    dmean, dvar = p.predict(Xt, predictive=False)
    p.close()
    assert M.rel_ok("l", ev.l, l, 1e-10)
    assert np.max(np.abs(ev.coeffs - t)) <= tol * np.max(np.abs(t))
    # posterior means and variances at new inputs against the same 80-bit evaluation
    assert np.max(np.abs(dmean - mean)) <= max(tol, 1e-9) * max(np.max(np.abs(mean)), 1e-3)
    assert np.max(np.abs(dvar - var)) <= 1e-7 * np.exp(0.1)


def test_inputs_with_a_large_common_offset():
    """The matrix-core gradient kernel expands |p - z|^2 around the centroid of the inducing points: data far from
    the origin (offset 1e4 at unit spread) must not cost digits against the oracle's direct differences."""
    n, m, d = 3000, 100, 3
    X, y, Z = synth(31, n, m, d)
    X = np.asfortranarray(X + 1.0e4)
    Z = np.asfortranarray(Z + 1.0e4)
    # The expected values come from the oracle on the SAME points moved back to the origin (the subtraction is exact): the
    # kernel only sees differences, and evaluated on the offset data the oracle itself -- the reference's operation sequence --
    # differs from this by 2.6e-7 of the largest inducing-point entry (the sums sum_r x_kr E_rc carry the offset), which a
    # per-family bound of 1e-8 would then charge to the device.
    ref = O.evaluate_fast(O.SeIsoKernel(0.3, 0.0), np.asfortranarray(Z - 1.0e4), np.asfortranarray(X - 1.0e4), y, 0.1)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=0.3, log_sf2=0.0, sigma2=0.1, inducing=Z)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD)


def test_zero_noise_is_accepted_like_the_reference():
    """Model.check_sigma2 only rejects sigma2 < 0 (lib/fitc_gp.ml:148-149): sigma2 = 0 leaves s = r, which the
    Cholesky jitter keeps positive.  Parity with the oracle at that corner (looser: s spans many decades)."""
    n, m, d = 800, 25, 2
    X, y, Z = synth(37, n, m, d)
    ref = O.evaluate_fast(O.SeIsoKernel(0.1, 0.0), Z, X, y, 0.0)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=0.1, log_sf2=0.0, sigma2=0.0, inducing=Z)
    p.close()
    assert np.isfinite(ev.l) and M.rel_ok("l", ev.l, ref["l"], 1e-7)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), 1e-5)


@pytest.mark.parametrize("d", [12, 20, 40])
def test_wide_point_dimensions(d):
    """Point dimensions 12 / 20 / 40 select the 16-, 32- and 64-wide instantiations of the covariance kernels and the
    (k-steps, dimension-tile) variants of the matrix-core gradient kernel; Cov_se_fat with a full D x d projection
    (D = d + 3) adds the projection-gradient tiles."""
    n, m = 1500, 70
    X, y, Z = synth(41, n, m, d)
    le = 0.5 * np.log(d)
    ref = O.evaluate_fast(O.SeIsoKernel(le, 0.1), Z, X, y, 0.2)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=le, log_sf2=0.1, sigma2=0.2, inducing=Z)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD)
    rng = np.random.default_rng(d)
    D = d + 3
    Xb = np.asfortranarray(rng.normal(size=(D, n)))
    P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d))
    kf = O.SeFatKernel(d, 0.1, P)
    Zf = np.asfortranarray(O.se_fat_project(kf, Xb[:, :m]) + 0.01 * rng.normal(size=(d, m)))
    yb = np.sin(Xb.sum(0)) + 0.1 * rng.normal(size=n)
    reff = O.evaluate_fast(kf, Zf, Xb, yb, 0.2)
    q = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, d, m)
    q.set_inputs(Xb)
    q.set_targets(yb)
    evf = q.eval(log_sf2=0.1, sigma2=0.2, inducing=Zf, tproj=P)
    q.close()
    assert M.rel_ok("l", evf.l, reff["l"], TOL_L)
    assert evf.grad.shape == reff["grad"].shape and M.grad_ok(evf.grad, reff["grad"], M.families("fat", d, m, D=D, proj=True), TOL_GRAD)


def test_point_dimensions_above_64():
    """No dimension limit in the reference (lib/cov_se_fat.ml:215-252 projects arbitrary-width inputs,
    bin/ocaml_gpr.ml:196-202 reads arbitrary-width samples): a general projection D = 200 -> d = 80 (MFMA projection
    kernel, chunked dimension loops in the covariance / gradient / trace kernels, 16 000 Proj gradient entries) and
    cov_se_iso at d = 100, against the oracle; predictions through the same kernels."""
    rng = np.random.default_rng(17)
    n, m, D, d = 3000, 150, 200, 80
    X = np.asfortranarray(rng.normal(size=(D, n)))
    y = np.sin(X[:5].sum(0)) + 0.1 * rng.normal(size=n)
    P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d))
    k = O.SeFatKernel(d, 0.1, P)
    Z = np.asfortranarray(O.se_fat_project(k, X[:, rng.permutation(n)[:m]]) + 0.01 * rng.normal(size=(d, m)))
    ref = O.evaluate_fast(k, Z, X, y, 0.1)
    p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, d, m, chunk_rows=1024)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_sf2=0.1, sigma2=0.1, inducing=Z, tproj=P)
    assert ev.grad.shape == ref["grad"].shape == (1 + d * m + D * d,)
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("fat", d, m, D=D, proj=True), TOL_GRAD) and M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)
    Xt = np.asfortranarray(rng.normal(size=(D, 77)))
    mean, var = p.predict(Xt, predictive=False)
    assert M.vec_ok("pred_mean", mean, O.predict_means(k, Z, ref["coeffs"], Xt), TOL_POST)
    model = O.evaluate(k, Z, X, y, 0.1, want_grad=False, keep=True)["model"]
    assert M.vec_ok("pred_var", var, O.predict_variances(k, Z, model, Xt, predictive=False), TOL_POST)
    p.close()
    n, m, d = 2500, 130, 100
    X, y, Z = synth(23, n, m, d)
    le = 0.5 * np.log(d)
    ref = O.evaluate_fast(O.SeIsoKernel(le, -0.2), Z, X, y, 0.05)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=le, log_sf2=-0.2, sigma2=0.05, inducing=Z)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.grad_ok(ev.grad, ref["grad"], M.families("iso", d, m), TOL_GRAD) and M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)
    with pytest.raises(gpr_amd.GprHipError, match="multiscales support"):
        q = gpr_amd.Problem(gpr_amd.COV_SE_FAT, 300, 70, 70, 20)
        q.set_inputs(X[:70, :300])
        q.set_targets(y[:300])
        try:
            q.eval(log_sf2=0.0, sigma2=0.1, inducing=np.asfortranarray(X[:70, :20]),
                   log_multiscales_m05=np.zeros((70, 20), order="F"))
        finally:
            q.close()


def test_fp32_bulk_posterior_paths():
    """Prediction, training-set statistics and covariances on a problem created in the fp32-bulk mode (the n x m
    work of prediction and statistics runs in fp32 there; covariances are always fp64), against the fp64 oracle
    within the fp32 tolerances."""
    n, m, d, nt = 4000, 120, 8, 500  # (8 dimensions: the fp32-bulk coefficients are refused when K_m is ill-conditioned)
    X, y, Z = synth(43, n, m, d)
    Xt = np.asfortranarray(np.random.default_rng(2).normal(size=(d, nt)))
    k = O.SeIsoKernel(0.4, 0.1)
    ref = O.evaluate(k, Z, X, y, 0.2, want_grad=False, keep=True)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, precision=gpr_amd.F32_BULK, chunk_rows=1024)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(log_ell=0.4, log_sf2=0.1, sigma2=0.2, inducing=Z, want_grad=False)
    assert M.rel_ok("l", ev.l, ref["l"], TOL32_L)
    mean, var = p.predict(Xt, predictive=False)
    assert M.vec_ok("pred_mean", mean, O.predict_means(k, Z, ref["coeffs"], Xt), TOL32_COEFF)
    vref = O.predict_variances(k, Z, ref["model"], Xt, predictive=False)
    assert np.max(np.abs(var - vref)) <= 1e-3 * np.max(np.abs(vref))
    sums, tm = p.train_stats(want_means=True)
    knm, _ = O.spec_calc_shared_cross(k, X, Z)
    assert M.vec_ok("coeffs", tm, knm @ ref["coeffs"], TOL32_COEFF)
    cov = p.covariances(Xt[:, :64], kind="FITC", predictive=False)
    cref = O.fitc_covariances(k, Z, ref["model"], Xt[:, :64])
    assert np.max(np.abs(np.triu(cov) - cref)) <= 1e-3 * np.max(np.abs(cref))
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_random_shapes_against_oracle(seed):
    """Seeded sweep over shapes the fixed cases do not hit: odd point counts (several k-slices and row chunks with
    ragged tails), 1..6 tile rows of inducing points (SYRK diagonal / off-diagonal tile maps and their slice ratios),
    every point-dimension instantiation, both kernels with random option sets, standard and variational."""
    _random_shape_case(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3000, 3024))
def test_random_small_shapes_against_oracle(seed):
    """The same sweep over the shapes the one-kernel passes take (gpr_amd/csrc/small.hip: m <= 64, d <= 16, D <= 64;
    multiscale cases with more than 8 point dimensions fall back to the engine and say so): 1..64 inducing points and
    1..4000 training points, every kernel option, followed by a sigma2-only re-evaluation (reuse_v) on the state the
    small path left."""
    _random_shape_case(seed, small=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,m,d,D", [("iso", 20000, 40, 3, 3), ("iso", 65536, 64, 16, 16), ("fat", 9000, 33, 5, 8),
                                          ("iso", 65537, 20, 2, 2), ("fat", 700, 25, 4, 17), ("fat", 2500, 64, 16, 64),
                                          ("fat", 1500, 12, 9, 41), ("iso", 300001, 40, 3, 3), ("fat", 140000, 30, 4, 20)])
def test_small_path_with_several_blocks_per_workgroup(kind, n, m, d, D, monkeypatch):
    """Above 16 384 training points a workgroup of the small row passes walks several 64-row blocks (256 workgroups at
    most) and accumulates its partial sums across them; the rows of several chunks (131 072 each) are one range to it.
    Projections from more than 16 input dimensions (up to 64) form their input moments
    as one more matrix-core product per block.  Against the oracle, and against the engine path on the same problem."""
    rng = np.random.default_rng(n + m)
    if kind == "iso":
        X, y, Z = synth(77, n, m, d)
        k = O.SeIsoKernel(0.5 * np.log(d) + 0.1, 0.2)
        args = dict(log_ell=k.log_ell, log_sf2=k.log_sf2)
        code = gpr_amd.COV_SE_ISO
    else:
        X = np.asfortranarray(rng.normal(size=(D, n)))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d))
        Z = np.asfortranarray((P.T @ X)[:, rng.permutation(n)[:m]] + 0.01 * rng.normal(size=(d, m)))
        het = rng.uniform(-6, -3, size=m)
        k = O.SeFatKernel(d, 0.1, P, het, None)
        args = dict(log_sf2=k.log_sf2, tproj=P, log_hetero_skedasticity=het)
        code = gpr_amd.COV_SE_FAT
    ref = O.evaluate(k, Z, X, y, 0.15, variational=True)
    fams = M.families("iso", d, m) if kind == "iso" else M.families("fat", d, m, D=D, proj=True, het=True)
    out = {}
    for path in ("default", "engine"):
        if path == "engine":
            monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")
            monkeypatch.setenv("GPRHIP_MID_PATH", "0")
        p = gpr_amd.Problem(code, n, D, d, m)
        p.set_inputs(X)
        p.set_targets(y)
        p.set_timing(2)
        ev = p.eval(sigma2=0.15, inducing=Z, variational=True, **args)
        assert ("p1_small" in p.last_timings()) == (path == "default")
        p.close()
        assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
        assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
        assert M.grad_ok(ev.grad, ref["grad"], fams, TOL_GRAD)
        assert M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)
        out[path] = ev
    # (with few inducing points the default path also builds K_m inside its factorisation kernel: entries may differ from
    #  cov_upper_kernel's in the last bit, which a jitter-dominated K_m amplifies to ~1e-12 of the evidence)
    assert M.rel_ok("l", out["default"].l, out["engine"].l, 1e-10)
    assert M.grad_ok(out["default"].grad, out["engine"].grad, fams, 1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(5000, 5032))
def test_random_mid_shapes_against_oracle(seed):
    """The shapes of gpr_amd/csrc/mid.hip -- 65 .. 256 inducing points, the regime of the reference's default
    m = min (n / 10) 1000 (lib/fitc_gp.ml:1474-1479) for data sets of 650 .. 2560 points -- and its thresholds (m = 64 | 65:
    small.hip | mid.hip; 128 | 129: one tile | two tiles; 256 | 257: mid.hip | engine): every fourth seed sits exactly on one,
    the rest are drawn from 60 .. 261; projections either side of the moment-matrix limit, multiscales and d > 16 falling back to the
    engine; each followed by a reuse_v re-evaluation on the state the path left."""
    _random_shape_case(seed, mid=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(5100, 5108))
def test_random_mid_shapes_through_the_context(seed):
    """... and as 2 .. 4 shards of the single-process multi-device entry."""
    _random_shape_case(seed, shards=2 + seed % 3, mid=True)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [64, 65, 128, 129, 256, 257])
def test_row_path_thresholds_agree_with_their_neighbours(m, monkeypatch):
    """The same problem through every row-pass family that can take it (m = 64: small.hip, mid.hip, engine; 65 .. 256:
    mid.hip -- one 128-column tile up to 128, two from 129 --, engine; 257: engine only): each against the oracle, and
    against each other far inside that bound."""
    n, d = 1500, 3
    X, y, Z = synth(70 + m, n, m, d)
    hyp = dict(log_ell=0.5 * np.log(d) + 0.05, log_sf2=0.1, sigma2=0.12, inducing=Z, variational=True)
    ref = O.evaluate(O.SeIsoKernel(hyp["log_ell"], 0.1), Z, X, y, 0.12, variational=True)
    fams = M.families("iso", d, m)
    paths = [("default", {})]
    if m <= 64:
        paths.append(("mid", {"GPRHIP_SMALL_PATH": "0"}))
    if m <= 256:
        paths.append(("engine", {"GPRHIP_SMALL_PATH": "0", "GPRHIP_MID_PATH": "0"}))
    out = {}
    for name, env in paths:
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
        p.set_inputs(X)
        p.set_targets(y)
        p.set_timing(2)
        ev = p.eval(**hyp)
        stages = set(p.last_timings())
        cond = p.condition()[0]
        p.close()
        taken = "small" if "p1_small" in stages else ("mid" if "p1_mid" in stages else "engine")
        expect = {"default": "small" if m <= 64 else ("mid" if m <= 256 else "engine"), "mid": "mid", "engine": "engine"}[name]
        assert taken == expect, (name, stages)
        assert M.rel_ok("l", ev.l, ref["l"], TOL_L) and M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
        assert M.grad_ok(ev.grad, ref["grad"], fams, TOL_GRAD, cond=cond) and M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)
        out[name] = ev
    for name in out:
        assert M.rel_ok("l", out[name].l, out["default"].l, 1e-10)
        assert M.grad_ok(out[name].grad, out["default"].grad, fams, 1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,d", [(1291, 129, 3), (3000, 200, 4), (4096, 256, 8), (4097, 131, 2)])
def test_two_tile_gram_launches_agree_with_the_engines(n, m, d, monkeypatch):
    """129 .. 256 inducing points: B~, c~ and G~ are accumulated over the resident V by mid.hip's own launch pair
    (mid_gram_kernel + its slice reduction; shards of at most 4096 rows, gpr_amd/csrc/kernels.h: MID_GRAM_ROWS) or --
    GPRHIP_MID_GRAM=0, and above that size -- by the engine's SYRK-shaped launch, both into the same exchange buffers.  Each
    against the oracle, and against each other."""
    X, y, Z = synth(300 + m, n, m, d)
    hyp = dict(log_ell=0.5 * np.log(d) + 0.1, log_sf2=-0.1, sigma2=0.2, inducing=Z)
    ref = O.evaluate(O.SeIsoKernel(hyp["log_ell"], hyp["log_sf2"]), Z, X, y, hyp["sigma2"])
    fams = M.families("iso", d, m)
    out = {}
    for gram in ("1", "0"):
        monkeypatch.setenv("GPRHIP_MID_GRAM", gram)
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
        p.set_inputs(X)
        p.set_targets(y)
        p.set_timing(2)
        ev = p.eval(**hyp)
        stages = set(p.last_timings())
        cond = p.condition()[0]
        ev2 = p.eval(**dict(hyp, sigma2=0.3), reuse_v=True)  # (update_sigma2: pass 1 re-weights the kept V, same Gram launches)
        p.close()
        assert {"p1_mid", "p1_syrk_B", "p2_mid", "p2_syrk_W"} <= stages, stages
        assert M.rel_ok("l", ev.l, ref["l"], TOL_L) and M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
        assert M.grad_ok(ev.grad, ref["grad"], fams, TOL_GRAD, cond=cond) and M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)
        out[gram] = (ev, ev2)
    for k in (0, 1):
        assert M.rel_ok("l", out["1"][k].l, out["0"][k].l, 1e-10)
        assert M.grad_ok(out["1"][k].grad, out["0"][k].grad, fams, 1e-8)
    ref2 = O.evaluate(O.SeIsoKernel(hyp["log_ell"], hyp["log_sf2"]), Z, X, y, 0.3)
    assert M.rel_ok("l", out["1"][1].l, ref2["l"], TOL_L) and M.grad_ok(out["1"][1].grad, ref2["grad"], fams, TOL_GRAD, cond=cond)


@pytest.mark.gpu
def test_shards_on_both_sides_of_the_two_tile_row_limit():
    """mid.hip's two-tile kernels take shards of at most 32768 rows (gpr_amd/csrc/kernels.h: MID_ROWS_TWO_TILES; the engine
    is faster above).  65537 rows over two shards: 32769 go through the engine, 32768 through mid.hip, both into the same
    exchange buffers -- the sums and the finish do not know which family filled them."""
    n, m, d = 2 * 32768 + 1, 200, 4
    X, y, Z = synth(77, n, m, d)
    hyp = dict(log_ell=0.5 * np.log(d), log_sf2=0.05, sigma2=0.15, inducing=Z)
    ref = O.evaluate(O.SeIsoKernel(hyp["log_ell"], hyp["log_sf2"]), Z, X, y, hyp["sigma2"])
    fams = M.families("iso", d, m)
    ctx = gpr_amd.Context([0, 0])
    sp = gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, n, d, d, m)
    sp.set_inputs(X)
    sp.set_targets(y)
    for i in range(2):
        sp.problem(i).set_timing(2)
    ev = sp.eval(**hyp)
    taken = []
    for i in range(2):
        stages = set(sp.problem(i).last_timings())
        taken.append((sp.shard(i)[2] - sp.shard(i)[1], "mid" if "p1_mid" in stages else "engine"))
    cond = sp.problem(0).condition()[0]
    sp.close()
    ctx.close()
    assert taken == [(32769, "engine"), (32768, "mid")], taken
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L) and M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
    assert M.grad_ok(ev.grad, ref["grad"], fams, TOL_GRAD, cond=cond) and M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL_COEFF)


# ("kernel_p1_syrk_B" is the level-1 event pair around the pass-1 Gram launch, which level 2 includes; tcollect lists it first)
_ENGINE_P1 = ["kernel_p1_syrk_B", "km_chol", "p1_cov", "p1_trmm_V", "p1_rows", "p1_syrk_B", "b_chol", "inverses", "p2_trmm_Q", "p2_rows"]
# (n, m, d, chunk_rows, switches, stages of a gradient evaluation, stages of the reuse_v re-evaluation or None)
_STAGE_ORDER = {
    "small": (300, 20, 3, 0, {}, ["km_chol", "p1_small", "b_chol", "p2_small", "finish"], None),
    "one_tile": (300, 100, 3, 0, {}, ["km_chol", "p1_mid", "b_chol", "p2_mid", "finish"], None),
    "two_tiles": (600, 200, 3, 0, {}, ["kernel_p1_syrk_B", "km_chol", "p1_mid", "p1_syrk_B", "b_chol", "p2_mid", "p2_syrk_W", "finish"],
                  ["km_chol", "p1_rows", "p1_syrk_B", "b_chol", "p2_mid", "p2_syrk_W", "finish"]),
    "two_tiles_engine_gram": (600, 200, 3, 0, {"GPRHIP_MID_GRAM": "0"},
                              ["kernel_p1_syrk_B", "km_chol", "p1_mid", "p1_syrk_B", "b_chol", "p2_mid", "p2_syrk_W", "finish"], None),
    "engine_two_launch_x": (1500, 300, 3, 512, {"GPRHIP_MERGED_X": "0"},
                            _ENGINE_P1 + ["p2_trmm_S", "p2_trmm_X", "p2_grad", "p2_syrk_W", "finish"], None),
    "engine_two_phase_x": (1500, 300, 3, 512, {"GPRHIP_MERGED_X": "2"},
                           _ENGINE_P1 + ["p2_trmm_SX", "p2_grad", "p2_syrk_W", "finish"], None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_STAGE_ORDER))
def test_stage_order_of_every_evaluation_path(case, monkeypatch):
    """The order in which a gradient evaluation enters its stages (last_timings() under set_timing(2) lists every stage once,
    by first entry), per path: small.hip, mid.hip with one tile, with two tiles and its own Gram launch pair, with two tiles and
    the engine's Gram launch, the engine over three ragged chunks with either X product -- and the re-weighted (reuse_v)
    evaluation of a two-tile problem, whose rows go through the engine's row kernel and whose Gram accumulation through the
    pair again.  The lists were recorded from the driver before each path got a function of its own."""
    n, m, d, chunk_rows, env, expect, expect_reuse = _STAGE_ORDER[case]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)  # read when the problem is created
    X, y, Z = synth(11, n, m, d)
    hyp = dict(log_ell=0.5 * np.log(d) + 0.1, log_sf2=-0.1, sigma2=0.2, inducing=Z)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=chunk_rows)
    p.set_inputs(X)
    p.set_targets(y)
    p.set_timing(2)
    p.eval(**hyp)
    stages = list(p.last_timings())
    reuse = None
    if expect_reuse is not None:
        p.eval(**dict(hyp, sigma2=0.4), reuse_v=True)
        reuse = list(p.last_timings())
    p.close()
    assert stages == expect, stages
    assert reuse == expect_reuse, reuse


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3100, 3106))
def test_random_small_shapes_through_the_context(seed):
    """... and through the single-process multi-device entry: the small passes write the same exchange buffers the
    engine path does, so shards of a small problem reduce and finish like any other."""
    _random_shape_case(seed, shards=2 + seed % 3, small=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_shapes_through_the_context(seed):
    """The same random-shape cases evaluated by the single-process multi-device entry (gprhip_sharded_eval) over 2..5
    shards of the one device a test box has: ragged shards, every kernel option, standard and variational, with and
    without row chunks inside a shard -- against the oracle at the unsharded tolerances."""
    _random_shape_case(seed, shards=2 + seed % 4)


@pytest.mark.gpu
def test_random_shapes_long_sweep():
    """The same sweep over a seed range given in GPR_FUZZ_SEEDS="lo:hi" (skipped without it): the long runs whose logs
    are kept under profiles/ (r03_fuzz.txt: seeds 24..423)."""
    spec = os.environ.get("GPR_FUZZ_SEEDS")
    if not spec:
        pytest.skip("GPR_FUZZ_SEEDS not set")
    lo, hi = (int(v) for v in spec.split(":"))
    bad = []
    shards = int(os.environ.get("GPR_FUZZ_SHARDS", "0"))  # > 0: through the context, seed-dependent shard counts up to it
    small = os.environ.get("GPR_FUZZ_SMALL", "0") == "1"   # the shapes of the small row passes
    mid = os.environ.get("GPR_FUZZ_MID", "0") == "1"       # the shapes of the one-tile row passes and their thresholds
    for seed in range(lo, hi):
        try:
            _random_shape_case(seed, shards=(2 + seed % (shards - 1)) if shards > 1 else 0, small=small, mid=mid)
        except AssertionError as e:  # keep going: the log should name every failing seed
            bad.append((seed, str(e)[:200]))
    print("random-shape sweep: seeds %d..%d, %d cases, %d failures %s" % (lo, hi - 1, hi - lo, len(bad), bad))
    assert not bad, bad


class _ShardedAsProblem:
    """A gpr_amd.ShardedDeviceProblem over `shards` shards of cuda:0 (the context's validation mode) with the small part
    of gpr_amd.Problem's surface the random-shape cases use."""

    def __init__(self, kind, n, D, d, m, shards, chunk_rows=0):
        self.ctx = gpr_amd.Context([0] * shards)
        self.sp = gpr_amd.ShardedDeviceProblem(self.ctx, kind, n, D, d, m, chunk_rows=chunk_rows)
        self.set_inputs, self.set_targets, self.eval = self.sp.set_inputs, self.sp.set_targets, self.sp.eval

    def problem(self, i):
        return self.sp.problem(i)

    def close(self):
        self.sp.close()
        self.ctx.close()


def _random_shape_case(seed, shards=0, small=False, mid=False):
    rng = np.random.default_rng(1000 + seed)
    iso = seed % 2 == 0   # (the oracle forms one dense n x m derivative matrix per Proj hyper: smaller fat cases)
    n = int(rng.integers(300, 6000 if iso else 3000))
    m = int(rng.integers(5, 520 if iso else 270))
    d = int(rng.choice([1, 2, 3, 5, 8, 11, 16, 23, 32, 40] if iso else [1, 2, 3, 5, 8, 11, 16, 20]))
    if seed % 8 == 4:  # five to seven tile rows of inducing points
        m, d = int(rng.integers(520, 800)), int(rng.choice([2, 4, 8]))
    variational = bool(rng.integers(0, 2))
    sigma2 = float(10.0 ** rng.uniform(-2, 0))
    chunk_rows = int(rng.choice([0, 256, 1024, 4096]))
    if small:  # the shapes of gpr_amd/csrc/small.hip: at most 64 inducing points, 16 point dimensions
        n = int(rng.integers(1, 4000 if iso else 2500))
        m = int(rng.integers(1, 65))
        d = int(rng.choice([1, 2, 3, 4, 5, 8, 9, 13, 16] if iso else [1, 2, 3, 5, 8, 11, 13]))
        chunk_rows = 0
        if not iso:
            n = max(n, m)  # (the fat cases draw their inducing points from the projected inputs)
        if shards:
            n = max(n, 200)
    if mid:  # the shapes of gpr_amd/csrc/mid.hip (65 .. 128 inducing points) and both of its thresholds: 64 | 65, 128 | 129
        n = int(rng.integers(1, 5000 if iso else 2500))
        m = int(rng.choice([64, 65, 128, 129, 256, 257])) if seed % 4 == 0 else int(rng.integers(60, 262))
        d = int(rng.choice([1, 2, 3, 4, 5, 8, 9, 13, 16, 20] if iso else [1, 2, 3, 5, 8, 11, 13]))
        chunk_rows = int(rng.choice([0, 0, 1024]))
        if not iso:
            n = max(n, m)
        if shards:
            n = max(n, 200)
    if iso:
        X, y, Z = synth(2000 + seed, n, min(m, n), d)
        if m > n:  # more inducing points than training points: legal, and a shape of its own (k-range shorter than m)
            Z = np.asfortranarray(np.hstack([Z, rng.normal(size=(d, m - n))]))
        log_ell = 0.5 * np.log(d) + rng.uniform(-0.3, 0.3)
        k = O.SeIsoKernel(log_ell, rng.uniform(-0.5, 0.5))
        p = (gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=chunk_rows) if not shards
             else _ShardedAsProblem(gpr_amd.COV_SE_ISO, n, d, d, m, shards, chunk_rows))
        args = dict(log_ell=k.log_ell, log_sf2=k.log_sf2)
        fams = M.families("iso", d, m)
    else:
        D = d + int(rng.integers(0, 4))
        if small and seed % 3 == 0:
            D = int(rng.integers(17, 65))  # (the small path's wide-input variant; the oracle's n x m matrices stay small)
        if mid and seed % 3 == 0:
            D = int(rng.integers(d + 4, 36))  # (either side of mid.hip's 1 + d + D <= 32)
        X = np.asfortranarray(rng.normal(size=(D, n)))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d)) if (D != d or rng.integers(0, 2)) else None
        proj = (P.T @ X) if P is not None else X
        Z = np.asfortranarray(proj[:, rng.permutation(n)[:m]] + 0.01 * rng.normal(size=(d, m)))
        het = rng.uniform(-6, -3, size=m) if rng.integers(0, 2) else None
        ms = rng.uniform(-0.5, 0.5, size=(d, m)) if (rng.integers(0, 3) == 0 and D <= 32) else None
        k = O.SeFatKernel(d, rng.uniform(-0.5, 0.5), P, het, ms)
        p = (gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, d, m, chunk_rows=chunk_rows) if not shards
             else _ShardedAsProblem(gpr_amd.COV_SE_FAT, n, D, d, m, shards, chunk_rows))
        args = dict(log_sf2=k.log_sf2)
        fams = M.families("fat", d, m, D=D, proj=P is not None, het=het is not None, ms=ms is not None)
        if P is not None:
            args["tproj"] = P
        if het is not None:
            args["log_hetero_skedasticity"] = het
        if ms is not None:
            args["log_multiscales_m05"] = np.asfortranarray(ms)
    ref = O.evaluate(k, Z, X, y, sigma2, variational=variational)
    M.note(seed=seed, n=n, m=m, d=d)
    p.set_inputs(X)
    p.set_targets(y)
    if (small or mid) and not shards:
        p.set_timing(2)
    ev = p.eval(sigma2=sigma2, inducing=Z, variational=variational, **args)
    # the device's own 2-norm estimate of cond(K_m + jitter): the gradient checks below carry the conditioning allowance
    # cond x 2^-53 relative to the gradient's largest entry (tests/margins.py, family_errors) beside the family-relative bound
    cond = (p.problem(0) if shards else p).condition()[0]
    M.note(_reset=False, cond=cond)
    if mid and not shards:
        stages = set(p.last_timings())
        Dp = D if (not iso and "tproj" in args) else 0
        want_mid = 64 < m <= 256 and d <= 16 and 1 + d + Dp <= 32 and "log_multiscales_m05" not in args
        want_small = m <= 64 and d <= (8 if "log_multiscales_m05" in args else 16) and Dp <= 64
        assert ("p1_mid" in stages) == (want_mid or (m <= 64 and not want_small and d <= 16 and 1 + d + Dp <= 32
                                                   and "log_multiscales_m05" not in args)), (stages, m, d, Dp)
        assert ("p1_small" in stages) == want_small, (stages, m, d, Dp)
        p.set_timing(0)
        # Model.update_sigma2 on the state a mid-path evaluation left: the engine's pass 1 reuses its V and r
        ref2 = O.evaluate(k, Z, X, y, 2.0 * sigma2, variational=variational)
        ev2 = p.eval(sigma2=2.0 * sigma2, inducing=Z, variational=variational, reuse_v=True, **args)
        assert M.rel_ok("l", ev2.l, ref2["l"], TOL_L)
        assert M.grad_ok(ev2.grad, ref2["grad"], fams, TOL_GRAD, cond=cond)
    if small and not shards:
        took_small = "p1_small" in p.last_timings()
        assert took_small == ("log_multiscales_m05" not in args or d <= 8), (took_small, d, sorted(args))
        p.set_timing(0)
        # Model.update_sigma2 after a small-path evaluation: V and r of the small pass are reused by the engine's pass 1
        ref2 = O.evaluate(k, Z, X, y, 2.0 * sigma2, variational=variational)
        ev2 = p.eval(sigma2=2.0 * sigma2, inducing=Z, variational=variational, reuse_v=True, **args)
        assert M.rel_ok("l", ev2.l, ref2["l"], TOL_L)
        assert M.grad_ok(ev2.grad, ref2["grad"], fams, TOL_GRAD, cond=cond)
    ev0 = p.eval(sigma2=sigma2, inducing=Z, variational=variational, want_grad=False, **args)
    p.close()
    assert M.rel_ok("l", ev.l, ref["l"], TOL_L)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref["dl_dsigma2"], TOL_DS2)
    assert ev.grad.shape == ref["grad"].shape and M.grad_ok(ev.grad, ref["grad"], fams, TOL_GRAD, cond=cond)
    # (points on a line: K_m is jitter-dominated and the coefficients carry cond^2 eps through the explicit inverses --
    #  1.1e-7 at seed 600, see test_mean_coefficients_against_an_80_bit_evaluation)
    #  One case in 600 of the final round-6 sweep went past the bound by a tenth (seed 21536: 3.35e-7): the forward error of
    #  the solves is cond eps, so the allowance the gradient families get applies here as well.
    assert M.vec_ok("coeffs" if d > 1 else "coeffs_d1", ev.coeffs, ref["coeffs"], TOL_COEFF if d > 1 else TOL_COEFF_LINE,
                    cond=cond)
    assert M.rel_ok("l", ev0.l, ev.l, 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_shapes_fp32_bulk_against_oracle(seed):
    """The fp32-bulk mode over the same kind of sweep (16- and 32-dimensional points take the matrix-core covariance
    builder, projections the derived inducing gradient), against the fp64 oracle inside the mode's stated bounds."""
    _random_fp32_case(seed)


@pytest.mark.gpu
def test_random_shapes_fp32_bulk_long_sweep():
    """GPR_FUZZ_F32="lo:hi": the fp32-bulk sweep over a seed range (log: profiles/r03_fuzz.txt)."""
    spec = os.environ.get("GPR_FUZZ_F32")
    if not spec:
        pytest.skip("GPR_FUZZ_F32 not set")
    lo, hi = (int(v) for v in spec.split(":"))
    bad = []
    for seed in range(lo, hi):
        try:
            _random_fp32_case(seed)
        except AssertionError as e:
            bad.append((seed, str(e)[:160]))
    print("fp32-bulk random-shape sweep: seeds %d..%d, %d cases, %d failures %s" % (lo, hi - 1, hi - lo, len(bad), bad))
    assert not bad, bad


def _random_fp32_case(seed, collect=None):
    rng = np.random.default_rng(3000 + seed)
    n = int(rng.integers(1500, 7000))
    m = int(rng.integers(40, 420))
    d = int(rng.choice([3, 8, 16, 24, 32]))
    sigma2 = float(10.0 ** rng.uniform(-1.3, 0))
    chunk_rows = int(rng.choice([0, 1024]))
    if seed % 2 == 0:
        X, y, Z = synth(4000 + seed, n, m, d)
        k = O.SeIsoKernel(0.5 * np.log(d) + rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3))
        p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, chunk_rows=chunk_rows, precision=gpr_amd.F32_BULK)
        args = dict(log_ell=k.log_ell, log_sf2=k.log_sf2)
        fams = M.families("iso", d, m)
    else:
        m = min(m, 200)
        d = min(d, 16)
        D = d + int(rng.integers(0, 3))
        X = np.asfortranarray(rng.normal(size=(D, n)))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        P = np.asfortranarray(rng.normal(size=(D, d)) / np.sqrt(D * d))
        Z = np.asfortranarray((P.T @ X)[:, rng.permutation(n)[:m]] + 0.01 * rng.normal(size=(d, m)))
        k = O.SeFatKernel(d, rng.uniform(-0.3, 0.3), P, None, None)
        p = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, d, m, chunk_rows=chunk_rows, precision=gpr_amd.F32_BULK)
        args = dict(log_sf2=k.log_sf2, tproj=P)
        fams = M.families("fat", d, m, D=D, proj=True)
    ref = O.evaluate(k, Z, X, y, sigma2)
    p.set_inputs(X)
    p.set_targets(y)
    ev = p.eval(sigma2=sigma2, inducing=Z, **args)
    cond = p.condition()[0]
    p.close()
    M.note(seed=seed, n=n, m=m, d=d, cond=cond)
    if collect is not None:
        collect.append(dict(seed=seed, n=n, m=m, d=d, iso=seed % 2 == 0, sigma2=sigma2,
                            l=abs(ev.l - ref["l"]) / abs(ref["l"]), grad=relinf(ev.grad, ref["grad"]),
                            coeffs=relinf(ev.coeffs, ref["coeffs"])))
        return
    # Stated bounds of the mode (1e-4 on the evidence, 5e-3 on gradient and mean coefficients) hold from 8 point
    # dimensions on -- over 200 random shapes (profiles/r03_f32_sweep.txt) the 170 cases with d >= 8 stay below 3.9e-6 /
    # 2.3e-4 / 3.6e-3.  With hundreds of inducing points in 3 dimensions K_m is ill-conditioned and the fp32 operands
    # show it: evidence up to 1.3e-4, gradient up to 4.2e-3, and the mean coefficients t = B^-1 K_mn S^-1 y lose
    # their digits altogether (0.06 median, up to 0.55): the mode is not meant for that regime, and only the evidence
    # and the gradient are bounded there.
    if d >= 8:
        assert M.rel_ok("l", ev.l, ref["l"], TOL32_L)
        # (per family, with the conditioning allowance at the fp32 unit roundoff: cond(K_m + jitter) x 2^-24 of the largest entry)
        assert M.grad_ok(ev.grad, ref["grad"], fams, TOL32_GRAD, cond=cond, unit=M.EPS32)
        assert M.vec_ok("coeffs", ev.coeffs, ref["coeffs"], TOL32_COEFF)
    else:
        # (few dimensions, many inducing points: outside the mode's stated regime -- the gradient as ONE family, i.e. against
        #  its largest entry, and the evidence to 2e-3: worst seen over 400 such cases 5.1e-4, profiles/r06_parity_margins.txt)
        assert M.rel_ok("l_lowdim", ev.l, ref["l"], 2e-3)
        assert M.grad_ok(ev.grad, ref["grad"], [("whole", slice(0, ref["grad"].shape[0]))], 1e-2, "grad_lowdim")


def _harness(name):
    """build/<name>, built by __graft_entry__.build(); built on the spot (hipcc is on the GPU box) if the snapshot
    came without it."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "build", name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "gpr_amd", "csrc"), "tools"], capture_output=True, timeout=900)
    assert os.path.exists(exe), "build/%s not built (make -C gpr_amd/csrc tools)" % name
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"F32": "1"}], ids=["fp64", "fp32"])
def test_engine_harness(env):
    """tools/gemm_check.hip (built by `make -C gpr_amd/csrc tools`, i.e. by __graft_entry__.build()): every operand
    layout, triangular k-range, weighted / column-sum / diagonal-tile variant and fused epilogue of the MFMA engine
    against a naive kernel, in the paired XCD-local tile order the library launches with."""
    import subprocess
    exe = _harness("gemm_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ORD="3", **env))
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("check ")]
    assert len(lines) >= 10 and all(ln.rstrip().endswith("OK") for ln in lines), out.stdout[-3000:]
    assert ("f32 checks failed: 0" if env else "checks failed: 0") in out.stdout


@pytest.mark.gpu
def test_diagonal_block_harness():
    """tools/potrf_check.hip: the LDS-resident 128 x 128 Cholesky + inverse kernel against its definition."""
    import re
    import subprocess
    exe = _harness("potrf_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    m = re.search(r"max \|U\^T U - A\| = (\S+)\s+max \|U Dinv - I\| = (\S+)", out.stdout)
    assert m, out.stdout[-2000:]
    assert float(m.group(1)) < 1e-12 and float(m.group(2)) < 1e-13
    # the whole blocked factorisation (factor-only diagonal kernel, substitution panel, small-tile trailing update,
    # block inverses in one launch) at 1 .. 32 block rows; the strict lower triangle is poisoned with 1e300
    rows = re.findall(r"blocked potrf m=(\d+): \S+ us  info=(-?\d+)  max \|U\^T U - A\| / max\|A\| = (\S+)  "
                      r"max \|U_jj Dinv_j - I\| = (\S+)", out.stdout)
    assert [int(r[0]) for r in rows] == [128, 256, 384, 512, 1024, 2048, 4096], out.stdout[-2000:]
    for _, info, ea, ed in rows:
        assert int(info) == 0 and float(ea) < 1e-13 and float(ed) < 1e-10
    # ... and with the identity carried along as right-hand side: the same factor, U X = I, X upper triangular
    inv = re.findall(r"blocked potrf\+inverse m=(\d+): \S+ us  factor differs by (\S+)  max \|U X - I\| = (\S+)  "
                     r"max \|strict lower of X\| = (\S+)", out.stdout)
    assert [int(r[0]) for r in inv] == [128, 256, 384, 512, 1024, 2048, 4096], out.stdout[-2000:]
    for _, eu, ei, el in inv:
        assert float(eu) == 0.0 and float(ei) < 1e-10 and float(el) == 0.0
    # the same factorisation + inverse as ONE persistent launch with device-side dependencies (potrf_upper_chain: measured
    # slower than the step launches and off by default, DESIGN section 14 -- but it must stay correct): no dependency wait
    # ran into its bound, and both results are bit-identical to the step launches'
    chain = re.findall(r"chain potrf\+inverse m=(\d+): \S+ us \(stepwise \S+\)  info=(-?\d+)\S*  factor differs by (\S+)  "
                       r"inverse differs by (\S+)", out.stdout)
    assert [int(r[0]) for r in chain] == [256, 384, 512, 1024, 2048, 4096], out.stdout[-2000:]
    for _, info, du, dx in chain:
        assert int(info) == 0 and float(du) == 0.0 and float(dx) == 0.0


# ---- round 4: single-process multi-device context (gprhip_ctx_* / gprhip_sharded_*), element-wise covariance pins

def _ctx_eval(devices, kind, X, y, Z, hyp, D=None, chunk_rows=0, precision=None, want_stats=False):
    d, m = Z.shape
    Dn, n = X.shape
    ctx = gpr_amd.Context(devices)
    sp = gpr_amd.ShardedDeviceProblem(ctx, kind, n, Dn, d, m, chunk_rows=chunk_rows,
                                      precision=gpr_amd.F64 if precision is None else precision)
    sp.set_inputs(X)
    sp.set_targets(y)
    if want_stats:
        sp.set_timing(1)
    ev = sp.eval(**hyp)
    ev0 = sp.eval(want_grad=False, **hyp)
    stats = (sp.comm_stats(), ctx.comm_mode, [sp.shard(i) for i in range(ctx.ndev)])
    t = sp.problem(0).debug_fetch("t")
    sp.close()
    ctx.close()
    return ev, ev0, stats, t


def test_context_with_one_device_is_bit_identical_to_the_plain_evaluation():
    """gprhip_sharded_eval over a one-device context runs the very same enqueue sequence as gprhip_eval."""
    n, m, d = 3001, 140, 4
    X, y, Z = synth(12, n, m, d)
    hyp = dict(log_ell=0.6, log_sf2=0.1, sigma2=0.2, inducing=Z)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ref = p.eval(**hyp)
    ref0 = p.eval(want_grad=False, **hyp)
    p.close()
    ev, ev0, (stats, mode, shards), t = _ctx_eval([0], gpr_amd.COV_SE_ISO, X, y, Z, hyp)
    assert mode == gpr_amd.context.COMM_NONE and stats["collectives"] == 0
    assert shards == [(0, 0, n)]
    assert ev.l == ref.l and ev.l1 == ref.l1 and ev.dl_dsigma2 == ref.dl_dsigma2
    assert np.array_equal(ev.grad, ref.grad) and np.array_equal(ev.coeffs, ref.coeffs)
    assert ev0.l == ref0.l
    assert np.array_equal(t, ref.coeffs)


def test_context_through_rccl_with_one_rank():
    """GPRHIP_CTX_RCCL=1: the library dlopens RCCL, creates a one-rank communicator (ncclCommInitAll) and runs its two
    all-reduces on its own stream -- the in-library collective path on the one GPU a test box has.  Run in a fresh
    process so that the RCCL the library loads is its own choice, not one torch brought in."""
    import subprocess
    import sys
    code = (
        "import os, sys, json, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "os.environ['GPRHIP_CTX_RCCL'] = '1'\n"
        "import gpr_amd\n"
        "from tests.util import synth\n"
        "n, m, d = 3001, 140, 4\n"
        "X, y, Z = synth(12, n, m, d)\n"
        "hyp = dict(log_ell=0.6, log_sf2=0.1, sigma2=0.2, inducing=Z)\n"
        "p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m); p.set_inputs(X); p.set_targets(y); ref = p.eval(**hyp); p.close()\n"
        "ctx = gpr_amd.Context([0])\n"
        "sp = gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, n, d, d, m)\n"
        "sp.set_inputs(X); sp.set_targets(y); sp.set_timing(1)\n"
        "ev = sp.eval(**hyp); st = sp.comm_stats(); ev0 = sp.eval(want_grad=False, **hyp); st0 = sp.comm_stats()\n"
        "print(json.dumps(dict(mode=ctx.comm_mode, st=st, st0=st0, same=bool(ev.l == ref.l and np.array_equal(ev.grad, ref.grad)),\n"
        "      same0=bool(abs(ev0.l - ref.l) <= 1e-12 * abs(ref.l)), torch='torch' in sys.modules)))\n"
    ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    import json
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])  # (RCCL prints a banner to stdout)
    assert r["mode"] == gpr_amd.context.COMM_RCCL and not r["torch"]
    assert r["st"]["collectives"] == 2 and r["st0"]["collectives"] == 1
    assert r["st"]["bytes"][0] > 0 and r["st"]["bytes"][1] > 0 and all(t > 0.0 for t in r["st"]["ms"])
    assert r["same"] and r["same0"]  # a one-rank sum is the identity: bit-identical results


@pytest.mark.parametrize("ndev", [2, 3, 8])
def test_context_shards_on_one_device_equal_the_whole(ndev):
    """Validation mode of the context (one device named ndev times): ragged row shards, device-local exchange, every
    hyper family of Cov_se_fat -- against the unsharded evaluation (TOL_SHARD: only the summation order differs)."""
    g = load_golden("fat_all")
    p = _problem_for(g)
    ref = _eval_golden(p, g)
    p.close()
    hyp = dict(log_sf2=float(g["log_sf2"]), sigma2=float(g["sigma2"]), inducing=g["Z"], tproj=g["tproj"],
               log_hetero_skedasticity=g["log_hetero"], log_multiscales_m05=g["log_multiscales"])
    ev, ev0, (stats, mode, shards), t = _ctx_eval([0] * ndev, gpr_amd.COV_SE_FAT, g["X"], g["y"], g["Z"], hyp,
                                                  chunk_rows=256)
    n = g["X"].shape[1]
    assert mode == gpr_amd.context.COMM_SAME_DEVICE
    assert shards[0][1] == 0 and shards[-1][2] == n and all(a[2] == b[1] for a, b in zip(shards, shards[1:]))
    assert max(hi - lo for _, lo, hi in shards) - min(hi - lo for _, lo, hi in shards) <= 1
    assert stats["collectives"] == 1  # the evidence-only evaluation ran last
    assert M.rel_ok("l", ev.l, ref.l, TOL_SHARD)
    assert M.rel_ok("l", ev0.l, ref.l, TOL_SHARD)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref.dl_dsigma2, TOL_SHARD)
    assert M.grad_ok(ev.grad, ref.grad, M.families_golden(g), TOL_SHARD_GRAD)
    assert M.vec_ok("coeffs", ev.coeffs, ref.coeffs, TOL_SHARD_GRAD)
    assert M.grad_ok(ev.grad, g["grad"], M.families_golden(g), TOL_GRAD)


def test_context_eight_way_partition_at_4096_inducing_points():
    """BASELINE.json configs[3]'s partition (8 row shards, m = 4096, d = 16) at a size one GPU holds: ragged rows
    (160003 mod 8 != 0), the packed exchange buffers of m = 4096, gradient and evidence against the unsharded
    evaluation, and the bytes per exchange step against the packed lengths."""
    n, m, d = 160003, 4096, 16
    X, y, Z = synth(4, n, m, d)
    hyp = dict(log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p.set_inputs(X)
    p.set_targets(y)
    ref = p.eval(**hyp)
    a1, a2 = p.ar1_len(), p.ar2_len()
    p.close()
    ctx = gpr_amd.Context([0] * 8)
    sp = gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, n, d, d, m)
    sp.set_inputs(X)
    sp.set_targets(y)
    ev = sp.eval(**hyp)
    st = sp.comm_stats()
    sizes = [sp.shard(i)[2] - sp.shard(i)[1] for i in range(8)]
    sp.close()
    ctx.close()
    assert sorted(set(sizes)) == [20000, 20001] and sum(sizes) == n
    nt = m // 128
    packed = nt * (nt + 1) // 2 * 128 * 128
    assert a1 == packed + m + 4 and a2 == packed + (d + 1) * m + 8
    assert st["collectives"] == 2 and st["bytes"] == [a1 * 8, a2 * 8]
    assert M.rel_ok("l", ev.l, ref.l, TOL_SHARD)
    assert M.rel_ok("dl_dsigma2", ev.dl_dsigma2, ref.dl_dsigma2, 1e-11)
    assert M.grad_ok(ev.grad, ref.grad, M.families("iso", d, m), TOL_SHARD_GRAD)
    assert M.vec_ok("coeffs", ev.coeffs, ref.coeffs, 1e-6)  # cond(K_m) at m = 4096, d = 16 amplifies the summation-order difference


def test_context_posterior_paths_from_any_shard():
    """After a sharded evaluation the m x m model state is replicated: prediction, covariances and the export of the
    factors work on every shard's problem and agree with the unsharded problem; training statistics are per shard and
    combine with sum / sum / max / sum."""
    g = load_golden("posterior_iso")
    X, y, Z, Xt = g["X"], g["y"], g["Z"], g["Xt"]
    hyp = dict(log_ell=float(g["log_ell"]), log_sf2=float(g["log_sf2"]), sigma2=float(g["sigma2"]), inducing=Z)
    p = _problem_for(g)
    p.eval(**hyp)
    mean, var = p.predict(Xt)
    sums, _ = p.train_stats()
    u, r = p.co_variance_coeffs()
    p.close()
    ctx = gpr_amd.Context([0, 0, 0])
    sp = gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, X.shape[1], X.shape[0], Z.shape[0], Z.shape[1])
    sp.set_inputs(X)
    sp.set_targets(y)
    sp.eval(**hyp)
    acc = np.zeros(4)
    for i in range(3):
        q = sp.problem(i)
        mi, vi = q.predict(Xt)
        assert M.vec_ok("pred_mean", mi, mean, TOL_SHARD_GRAD) and M.vec_ok("pred_var", vi, var, TOL_SHARD_GRAD)
        si, _ = q.train_stats()
        acc[[0, 1, 3]] += si[[0, 1, 3]]
        acc[2] = max(acc[2], si[2])
    assert M.vec_ok("stats", acc, sums, TOL_SHARD_GRAD)
    ui, ri = sp.problem(2).co_variance_coeffs()
    assert M.vec_ok("u", ui, u, TOL_SHARD_GRAD) and M.vec_ok("r", ri, r, TOL_SHARD_GRAD)
    # the sharded entry points: test points split over the devices, statistics combined by the library
    ms, vs = sp.predict(Xt)
    assert M.vec_ok("pred_mean", ms, mean, TOL_SHARD_GRAD) and M.vec_ok("pred_var", vs, var, TOL_SHARD_GRAD)
    m1, v1 = sp.predict(Xt[:, :2], want_variances=False)  # fewer points than shards
    assert v1 is None and M.vec_ok("pred_mean", m1, mean[:2], TOL_SHARD_GRAD)
    ss, tm = sp.train_stats(want_means=True)
    assert M.vec_ok("stats", ss, sums, TOL_SHARD_GRAD) and M.vec_ok("pred_mean", tm, g["train_means"], 1e-7)
    sp.close()
    ctx.close()


def test_context_argument_checks():
    with pytest.raises(gpr_amd.GprHipError):
        gpr_amd.Context([])
    with pytest.raises(gpr_amd.GprHipError):
        gpr_amd.Context([99])
    with pytest.raises(gpr_amd.GprHipError):
        gpr_amd.Context([0, 0, 99])
    ctx = gpr_amd.Context([0, 0, 0])
    with pytest.raises(gpr_amd.GprHipError):  # fewer training points than shards
        gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, 2, 2, 2, 1)
    sp = gpr_amd.ShardedDeviceProblem(ctx, gpr_amd.COV_SE_ISO, 50, 2, 2, 4)
    X, y, Z = synth(0, 50, 4, 2)
    with pytest.raises(gpr_amd.GprHipError):  # inputs not set
        sp.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Z)
    sp.set_inputs(X)
    sp.set_targets(y)
    with pytest.raises(gpr_amd.GprHipError):  # Model.check_sigma2 on every shard
        sp.eval(log_ell=0.0, log_sf2=0.0, sigma2=-1.0, inducing=Z)
    ev = sp.eval(log_ell=0.0, log_sf2=0.0, sigma2=0.1, inducing=Z)  # usable after the failures
    assert np.isfinite(ev.l)
    sp.close()
    ctx.close()


def _oracle_km_knm(g):
    k = oracle_kernel(g)
    Km, _ = O.spec_calc_shared_upper(k, g["Z"])
    if g["kind"] != "iso" and k.hetero_skedasticity is not None:
        Km = Km.copy()
        Km[np.diag_indices(Km.shape[0])] -= k.hetero_skedasticity  # the device keeps K_m and the noise apart
    Knm, _ = O.spec_calc_shared_cross(k, g["X"], g["Z"])
    return Km, Knm


@pytest.mark.parametrize("name", ["iso_c1", "iso_ragged", "fat_proj", "fat_hetero", "fat_multiscale", "fat_all"])
def test_covariance_kernels_element_by_element(name):
    """The element-wise half of Test.check_deriv_hyper's recipe (lib/fitc_gp.ml:1223-1396): K_m and rows of K_nm as the
    device kernels produce them, against the oracle's direct-difference loops (lib/cov_se_iso.ml:56-87, :128-159,
    lib/cov_se_fat.ml:85-142, :224-256) -- the covariance kernels pinned by themselves, not through downstream sums."""
    g = load_golden(name)
    p = _problem_for(g)
    _eval_golden(p, g)
    m = g["Z"].shape[1]
    n = g["X"].shape[1]
    Km, Knm = _oracle_km_knm(g)
    km = p.debug_fetch_matrix("km")
    assert np.all(km[np.tril_indices(m, -1)] == 0.0)
    iu = np.triu_indices(m)
    assert np.max(np.abs(km[iu] - Km[iu])) <= 4e-16 * np.max(np.abs(Km[iu]))  # exp() within 1-2 ulp of libm's
    rows = min(n, 300)
    knm = p.debug_fetch_matrix("knm_rows", rows)
    assert knm.shape == (rows, m)
    assert np.max(np.abs(knm - Knm[:rows])) <= 4e-16 * np.max(np.abs(Knm))
    p.close()


def _hyper_args(g):
    args = dict(log_sf2=float(g["log_sf2"]), sigma2=float(g["sigma2"]), inducing=g["Z"].copy(),
                variational=bool(g.get("variational", False)))
    if g["kind"] == "iso":
        args["log_ell"] = float(g["log_ell"])
    else:
        if "tproj" in g:
            args["tproj"] = g["tproj"].copy()
        if "log_hetero" in g:
            args["log_hetero_skedasticity"] = g["log_hetero"].copy()
        if "log_multiscales" in g:
            args["log_multiscales_m05"] = g["log_multiscales"].copy()
    return args


def _device_covariances(p, args, n):
    """K_m (full symmetric, heteroskedastic noise included -- without the jitter, like Inducing.calc_upper) and K_nm as the
    device kernels build them for `args`."""
    p.eval(want_grad=False, **args)
    km = p.debug_fetch_matrix("km")
    km = km + np.triu(km, 1).T
    if args.get("log_hetero_skedasticity") is not None:
        km = km + np.diag(np.exp(args["log_hetero_skedasticity"]))
    return km, p.debug_fetch_matrix("knm_rows", n)


@pytest.mark.parametrize("name", ["iso_c1", "iso_c1_var", "fat_all", "fat_proj_var"])
def test_gradient_factors_against_differences_of_the_device_covariances(name):
    """The device counterpart of Test.check_deriv_hyper + Shared.calc_log_evidence (lib/fitc_gp.ml:1223-1396, :1005-1021):
    the derivative matrices of the spec never exist on the device (they are contracted inside the gradient kernels), so
    the check contracts central differences of the covariance matrices the device kernels produce with the device's own
    W, X and v,   dl/dtheta = -1/2 (v . diag K'_n - tr(W K'_m)) - tr(X^T K'_nm),   for one hyper of every family, and
    compares with the gradient entry the fused kernels returned.  No oracle on either side."""
    g = load_golden(name)
    p = _problem_for(g)
    n, m = g["X"].shape[1], g["Z"].shape[1]
    d = g["Z"].shape[0]
    args = _hyper_args(g)
    ev = p.eval(**args)
    W = p.debug_fetch_matrix("w_mat")
    X = p.debug_fetch_matrix("x_rows", n)
    v = p.debug_fetch("v")
    assert np.max(np.abs(W - W.T)) <= 1e-12 * np.max(np.abs(W))
    sf2 = np.exp(args["log_sf2"])
    iso = g["kind"] == "iso"
    # (position in the gradient, perturbation, diag K'_n) per hyper family, in Hyper.get_all order
    cases = []
    pos = 0
    if iso:
        cases.append(("Log_ell", pos, ("log_ell", None), 0.0)); pos += 1
    cases.append(("Log_sf2", pos, ("log_sf2", None), sf2)); pos += 1
    ind, dim = m // 2, d - 1
    cases.append(("Inducing_hyper", pos + ind * d + dim, ("inducing", (dim, ind)), 0.0)); pos += m * d
    if "tproj" in args:
        D = g["X"].shape[0]
        big, small = D - 2, 1
        cases.append(("Proj", pos + big * d + small, ("tproj", (big, small)), 0.0)); pos += D * d
    if "log_hetero_skedasticity" in args:
        cases.append(("Log_hetero_skedasticity", pos + 3, ("log_hetero_skedasticity", 3), 0.0)); pos += m
    if "log_multiscales_m05" in args:
        cases.append(("Log_multiscale_m05", pos + ind * d + dim, ("log_multiscales_m05", (dim, ind)), 0.0)); pos += m * d
    assert pos == ev.grad.shape[0]
    h = 1e-5
    for label, gi, (key, idx), dkn_diag in cases:
        mats = []
        for sgn in (+1.0, -1.0):
            a = {k: (val.copy() if isinstance(val, np.ndarray) else val) for k, val in args.items()}
            if idx is None:
                a[key] = a[key] + sgn * h
            else:
                a[key][idx] += sgn * h
            mats.append(_device_covariances(p, a, n))
        dkm = (mats[0][0] - mats[1][0]) / (2 * h)
        dknm = (mats[0][1] - mats[1][1]) / (2 * h)
        terms = (-0.5 * dkn_diag * np.sum(v), 0.5 * np.sum(W * dkm), -np.sum(X * dknm))
        fd = sum(terms)
        scale = max(abs(t) for t in terms) + 1e-300
        assert abs(fd - ev.grad[gi]) <= 2e-6 * scale + 1e-9, (label, fd, ev.grad[gi], terms)
    p.close()


def test_fp32_bulk_refuses_coefficients_it_cannot_stand_behind(monkeypatch):
    """fp32-bulk mean coefficients inherit cond(K_m + jitter) * 2^-24 (profiles/r04_f32_guard.txt): with many inducing
    points in few dimensions they are wrong in the first digit, and the library refuses to predict from them
    (GPRHIP_EPRECISION) instead of returning numbers -- the evidence and the gradient stay within their fp32-bulk
    tolerances; the fp64 problem predicts; GPRHIP_F32_COEFF_TOL=0 lifts the guard; well-conditioned problems pass it."""
    n, m, d = 4000, 200, 3
    X, y, Z = synth(11, n, m, d)
    hyp = dict(log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
    Xt = X[:, :50]
    p64 = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m)
    p64.set_inputs(X)
    p64.set_targets(y)
    e64 = p64.eval(**hyp)
    cond64, bound64 = p64.condition()
    km = p64.debug_fetch_matrix("km")
    w = np.linalg.eigvalsh(km + np.triu(km, 1).T + gpr_amd.CHOLESKY_JITTER * np.eye(m))
    assert 0.5 * w[-1] / w[0] <= cond64 <= 1.001 * w[-1] / w[0]  # a lower bound, close
    assert bound64 < 1e-7
    mean64, _ = p64.predict(Xt)
    p32 = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, precision=gpr_amd.F32_BULK)
    p32.set_inputs(X)
    p32.set_targets(y)
    e32 = p32.eval(**hyp)
    # (few dimensions, hundreds of inducing points: outside the mode's regime -- the gradient as one family, as the sweeps do)
    assert M.rel_ok("l", e32.l, e64.l, 3e-4) and M.grad_ok(e32.grad, e64.grad, [("whole", slice(0, e64.grad.shape[0]))], 1e-2)
    cond32, bound32 = p32.condition()
    assert abs(cond32 - cond64) <= 1e-3 * cond64 and bound32 > 0.25
    with pytest.raises(gpr_amd.UntrustworthyCoefficients) as ei:
        p32.predict(Xt)
    assert ei.value.status == gpr_amd._lib.EPRECISION and "cond(K_m + jitter)" in str(ei.value)
    with pytest.raises(gpr_amd.UntrustworthyCoefficients):
        p32.train_stats()
    p32.close()
    monkeypatch.setenv("GPRHIP_F32_COEFF_TOL", "0")
    q = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, precision=gpr_amd.F32_BULK)
    q.set_inputs(X)
    q.set_targets(y)
    q.eval(**hyp)
    q.predict(Xt)  # no refusal with the guard off
    q.close()
    monkeypatch.delenv("GPRHIP_F32_COEFF_TOL")
    # a well-conditioned problem (8 dimensions) passes the guard and its predictions agree with fp64
    n, m, d = 4000, 200, 8
    X, y, Z = synth(12, n, m, d)
    hyp = dict(log_ell=0.5 * np.log(d), log_sf2=0.0, sigma2=0.1, inducing=Z)
    res = {}
    for prec in (gpr_amd.F64, gpr_amd.F32_BULK):
        r = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, d, d, m, precision=prec)
        r.set_inputs(X)
        r.set_targets(y)
        r.eval(**hyp)
        res[prec] = (r.predict(X[:, :50])[0], r.condition())
        r.close()
    assert res[gpr_amd.F32_BULK][1][1] <= 0.25
    assert M.vec_ok("res_gpr_amd_F64_0", res[gpr_amd.F32_BULK][0], res[gpr_amd.F64][0], 5e-3)
    p64.close()
