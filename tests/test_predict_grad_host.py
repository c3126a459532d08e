"""Gradients of the predictive mean and variance with respect to the test inputs: what can be checked without a GPU -- the
reference the GPU tests use (tests/predict_grad_ref.py) against the oracle's own predictions and central differences of them,
the declarations of the new entry point in every layer, and the argument refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import fitc_oracle as O
from tests.predict_grad_ref import predict_grad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_predict_input_grad"
LD = np.longdouble

N, M, NT, SIGMA2 = 12, 4, 5, 0.3
H = 2.0 ** -13


def _case(kind):
    rng = np.random.default_rng(5)
    D = 3 if kind in ("fat_proj", "fat_proj_het") else 2
    X = np.asfortranarray(rng.normal(size=(D, N)))
    Xt = np.asfortranarray(rng.normal(size=(D, NT)))
    if kind == "iso":
        k = O.SeIsoKernel(0.2, 0.1)
    elif kind == "fat":
        k = O.SeFatKernel(2, 0.1, None)
    else:
        het = rng.uniform(-3.0, -1.0, size=M) if kind == "fat_proj_het" else None
        k = O.SeFatKernel(2, 0.1, np.asfortranarray(0.7 * rng.normal(size=(3, 2))), het)
    Z = np.asfortranarray(rng.normal(size=(2, M)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=N)
    return k, Z, X, y, Xt


@pytest.mark.parametrize("variational", [False, True], ids=["standard", "variational"])
@pytest.mark.parametrize("kind", ["iso", "fat", "fat_proj", "fat_proj_het"])
def test_reference_equals_the_oracle_and_its_central_differences(kind, variational):
    """The means and variances of the reference against the oracle's predict_means / predict_variances of a model from a
    standard and from a variational evaluation (1e-12 of the largest entry: two fp64 evaluation orders of a small,
    well-conditioned case), and every entry of both D x nt gradient matrices against D(h) = (f(x + h) - f(x - h)) / 2h of those
    predictions, the steps formed in 80-bit arithmetic and rounded (h = 2^-13: the points move by exactly h).

    What the quotient supports: D(h) - f' = h^2 f''' / 6 + O(h^4).  The third-derivative term is measured per entry from a
    second stencil, T = |D(2h) - D(h)| / 3; on top of it comes the rounding of the two fp64 predictions, 2^-53 times the size of
    the terms they sum (sf2 for a variance, sum |K t| for a mean) through a few hundred operations (the factor 256), divided by
    2h.  Bound per entry: 2 T + 256 * 2^-53 scale / h."""
    k, Z, X, y, Xt = _case(kind)
    out = O.evaluate(k, Z, X, y, SIGMA2, variational=variational, want_grad=False, keep=True)
    model, coeffs = out["model"], out["coeffs"]
    got = predict_grad_ref(k, Z, X, y, SIGMA2, Xt, predictive=True)
    D, nt = Xt.shape
    assert got["dmeans"].shape == (D, nt) and got["dvariances"].shape == (D, nt)

    def mean_of(P):
        return O.predict_means(k, Z, coeffs, P)

    def var_of(P):
        return O.predict_variances(k, Z, model, P, predictive=True)

    assert np.max(np.abs(got["means"] - mean_of(Xt))) <= 1e-12 * np.max(np.abs(got["means"]))
    assert np.max(np.abs(got["variances"] - var_of(Xt))) <= 1e-12 * np.max(np.abs(got["variances"]))
    latent = predict_grad_ref(k, Z, X, y, SIGMA2, Xt, predictive=False)
    assert np.allclose(latent["variances"] + SIGMA2, got["variances"], rtol=0, atol=1e-15)
    assert np.array_equal(latent["dvariances"], got["dvariances"]) and np.array_equal(latent["dmeans"], got["dmeans"])
    ktm, _ = O.spec_calc_shared_cross(k, Xt, Z)
    scale = {"dmeans": float(np.max(np.abs(ktm) @ np.abs(coeffs))), "dvariances": float(np.exp(k.log_sf2)) + SIGMA2}
    for name, fn in (("dmeans", mean_of), ("dvariances", var_of)):
        worst = 0.0
        for r in range(nt):
            for b in range(D):
                vals = {}
                for step in (-2, -1, 1, 2):
                    Xs = np.array(Xt, dtype=LD)
                    Xs[b, r] = Xs[b, r] + LD(step) * LD(H)
                    vals[step] = fn(np.asfortranarray(Xs.astype(np.float64)))[r]
                d1 = (vals[1] - vals[-1]) / (2 * H)
                d2 = (vals[2] - vals[-2]) / (4 * H)
                third = abs(d2 - d1) / 3.0
                bound = 2.0 * third + 256 * 2.0 ** -53 * scale[name] / H
                err = abs(got[name][b, r] - d1)
                worst = max(worst, err / bound)
                assert err <= bound, (kind, variational, name, r, b, got[name][b, r], d1, err, bound)
        assert np.max(np.abs(got[name])) > 1e-3  # (the comparison is not one of zeros)
        print("prediction-gradient reference vs central differences (%s, %s): worst error / bound %.3f" % (kind, name, worst))


def test_symbol_is_declared_in_every_layer_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gprhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+double\s*\*\s*test_inputs,\s*int64_t\s+ld,\s*int64_t\s+nt,"
                     r"\s*int\s+predictive,\s*double\s*\*\s*means,\s*double\s*\*\s*variances,\s*double\s*\*\s*dmeans,"
                     r"\s*double\s*\*\s*dvariances,\s*int64_t\s+ldg,\s*int\s+on_device\s*\)" % NAME, header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 11
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    assert NAME + "(" in open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    assert NAME + "(" in open(os.path.join(ROOT, "bindings", "gpr_hip_stubs.c")).read()
    assert '"gprhip_ml_predict_input_grad"' in open(os.path.join(ROOT, "bindings", "gpr_hip.ml")).read()


def test_python_layers_carry_the_feature():
    import sys
    from gpr_amd import cov_se_fat, cov_se_iso, fitc_gp
    from gpr_amd.problem import Problem
    assert callable(Problem.predict_input_grad)
    assert Problem.PREDICT_OUTPUTS == ("means", "variances", "dmeans", "dvariances")
    for spec in (cov_se_iso, cov_se_fat):
        GP = fitc_gp.Make_deriv(spec)
        for variant in (GP.FITC, GP.Variational_FITC):
            assert callable(variant.Eval.Means.calc_input_gradient)
            assert callable(variant.Eval.Variances.calc_input_gradient)
    # the torch front end is found, and importing the package does not pull torch in
    code = ("import sys, gpr_amd, importlib.util as u; assert 'torch' not in sys.modules; "
            "import gpr_amd.autograd as a; assert 'torch' not in sys.modules and callable(a.predict)")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_refusals_that_need_no_device():
    """A NULL problem, NULL test inputs and an unknown output name are refused before anything touches a device."""
    from gpr_amd import _lib
    from gpr_amd.problem import Problem
    lib = _lib.load()
    buf = np.zeros(4)
    vp = ctypes.c_void_p
    st = lib.gprhip_predict_input_grad(None, vp(buf.ctypes.data), 1, 1, 1, vp(buf.ctypes.data), None, None, None, 1, 0)
    assert st == _lib.EBADARG
    assert b"gprhip_predict_input_grad" in lib.gprhip_last_error()
    p = Problem.__new__(Problem)
    p._h = ctypes.c_void_p()  # (nothing to destroy)
    p.D = 2
    with pytest.raises(ValueError):
        Problem.predict_input_grad(p, np.zeros((2, 3)), want=("means", "gradients"))
    with pytest.raises(ValueError):
        Problem.predict_input_grad(p, np.zeros((3, 3)), want=("means",))


def test_cpp_mirror_methods_build(tmp_path):
    """tests/cpp/predict_grad_check.cpp -- Means::calc_input_gradient and Variances::calc_input_gradient of the C++ mirror --
    compiles and links; without arguments it only prints its usage (no device call)."""
    exe = tmp_path / "predict_grad_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "predict_grad_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr
