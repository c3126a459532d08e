"""The host surfaces of gprhip_observe above `Problem`: `Eval.Observe` of the Python functor (gpr_amd/fitc_gp.py) and
`Observe` of the C++ mirror (include/gprhip.hpp; tests/cpp/observe_mirror_check.cpp).  The OCaml module and its stubs are
type-checked with the rest of the stub file by tests/test_abi.py."""
import os
import subprocess

import numpy as np
import pytest

import gpr_amd
from tests.test_gpu_input_grads import Case, data

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA2 = 0.1
N = 200


def _build(tmp_path):
    exe = tmp_path / "observe_mirror_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "observe_mirror_check.cpp"), "-L", os.path.join(ROOT, "gpr_amd"), "-lgprhip",
                           "-Wl,-rpath," + os.path.join(ROOT, "gpr_amd"), "-o", str(exe)])
    return exe


def test_cpp_mirror_observe_compiles_and_links(tmp_path):
    out = subprocess.run([str(_build(tmp_path))], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr


def test_a_flat_list_of_several_points_is_refused_by_problem_observe():
    """(checked before the library is entered: no device needed)"""
    class P(gpr_amd.Problem):
        def __init__(self):
            self.D = 3
    with pytest.raises(ValueError):
        P().observe(np.zeros(6), np.zeros(2))


@gpu
def test_cpp_mirror_observe_save_restore(tmp_path):
    out = subprocess.run([str(_build(tmp_path)), "run"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0 and "observe_mirror_check: ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


@gpu
def test_functor_observe_equals_problem_observe_bit_for_bit():
    from gpr_amd import cov_se_iso, fitc_gp
    c = Case("iso", N + 8, 65, 3)
    X, y, Z, args = data(c)
    Xs, ys = np.asfortranarray(X[:, :N]), y[:N].copy()
    Xn, yn, Xt = np.asfortranarray(X[:, N:N + 3]), y[N:N + 3].copy(), np.asfortranarray(X[:, N + 3:N + 8])
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, N, 3, 3, 65)
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    try:
        p.set_inputs(Xs)
        p.set_targets(ys)
        p.eval(sigma2=SIGMA2, inducing=Z, **args)
        before = p.predict(Xt)
        want_dl = p.observe(Xn, yn, want_dlog_evidence=True)
        want = p.predict(Xt)
        kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(log_ell=args["log_ell"], log_sf2=args["log_sf2"]))
        inputs = F.Deriv.Inputs.calc(F.Deriv.Inducing.calc(kernel, Z), Xs)
        model = F.Deriv.Model.calc(inputs, SIGMA2)
        trained = F.Deriv.Trained.calc(model, ys)
        tin, nin = F.Eval.Inputs.calc(Xt, inputs.inducing), F.Eval.Inputs.calc(Xn, inputs.inducing)
        m0 = F.Eval.Means.calc(trained, tin)
        assert np.array_equal(m0, before[0]) and F.Eval.Observe.count(trained) == 0
        F.Eval.Observe.save(trained)
        dl = F.Eval.Observe.observe(trained, nin, yn, want_dlog_evidence=True)
        assert dl == want_dl and F.Eval.Observe.count(trained) == 3
        m1 = F.Eval.Means.calc(trained, tin)
        assert np.array_equal(m1, want[0]) and not np.array_equal(m1, m0)
        F.Eval.Observe.restore(trained)
        assert F.Eval.Observe.count(trained) == 0
        assert np.array_equal(F.Eval.Means.calc(trained, tin), m0)
        # a model's own state takes no targets: the factors alone
        lone = F.Deriv.Model.calc(inputs, 2 * SIGMA2)
        v0 = F.Eval.Variances.get(F.Eval.Variances.calc(lone, 2 * SIGMA2, tin), predictive=False)
        assert np.isfinite(F.Eval.Observe.observe(lone, nin, want_dlog_evidence=True)) and F.Eval.Observe.count(lone) == 3
        v1 = F.Eval.Variances.get(F.Eval.Variances.calc(lone, 2 * SIGMA2, tin), predictive=False)
        assert np.all(v1 <= v0 * (1 + 1e-12)) and np.any(v1 < v0)
        # ... and its evaluation on the shared problem dropped the slot saved above
        with pytest.raises(gpr_amd.GprHipError):
            F.Eval.Observe.restore(trained)
        with pytest.raises(TypeError):
            F.Eval.Observe.observe(object(), nin)
    finally:
        p.close()
        GP.close()
