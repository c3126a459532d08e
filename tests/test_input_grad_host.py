"""Gradient of the log evidence with respect to the training inputs: what can be checked without a GPU -- the reference the
GPU tests use (tests/input_grad_ref.py) against central differences of the oracle's own evidence, the declarations of the new
entry point in every layer, and the argument refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import fitc_oracle as O
from tests.input_grad_ref import input_grad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_eval_input_grad"
LD = np.longdouble

N, M, SIGMA2 = 12, 4, 0.3
H = 2.0 ** -13


def _case(kind):
    rng = np.random.default_rng(5)
    if kind == "iso":
        X = np.asfortranarray(rng.normal(size=(2, N)))
        k = O.SeIsoKernel(0.2, 0.1)
        d = 2
    elif kind == "fat":
        X = np.asfortranarray(rng.normal(size=(2, N)))
        k = O.SeFatKernel(2, 0.1, None)
        d = 2
    else:
        X = np.asfortranarray(rng.normal(size=(3, N)))
        k = O.SeFatKernel(2, 0.1, np.asfortranarray(0.7 * rng.normal(size=(3, 2))))
        d = 2
    Z = np.asfortranarray(rng.normal(size=(d, M)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=N)
    return k, Z, X, y


def _evidence(k, Z, X, y, variational, model_only):
    out = O.evaluate(k, Z, X, y, SIGMA2, variational=variational, want_grad=False)
    return out["l1"] if model_only else out["l"]


@pytest.mark.parametrize("model_only", [False, True], ids=["trained", "model"])
@pytest.mark.parametrize("variational", [False, True], ids=["standard", "variational"])
@pytest.mark.parametrize("kind", ["iso", "fat", "fat_proj"])
def test_reference_equals_central_differences_of_the_oracle(kind, variational, model_only):
    """Every entry of the D x n matrix against D(h) = (l(x + h) - l(x - h)) / 2h of the oracle's own evidence, the steps x +- h
    formed in 80-bit arithmetic and rounded (h = 2^-13 is a power of two: the points move by exactly h).

    What the quotient supports: D(h) - l' = h^2 l''' / 6 + O(h^4).  The third-derivative term is measured per entry from a
    second stencil, T = |D(2h) - D(h)| / 3 (= h^2 |l'''| / 6 to O(h^4)); on top of it comes the rounding of the two fp64
    evidences, 2^-53 |l| each through a few hundred operations (the factor 256 below), divided by 2h.  Bound per entry:
    2 T + 256 * 2^-53 max|l| / h -- about 1e-8 absolute here, on entries of order 0.1 .. 1: sign, factor and every term of the
    formula are pinned."""
    k, Z, X, y = _case(kind)
    got = input_grad_ref(k, Z, X, y, SIGMA2, variational, model_only)
    D, n = X.shape
    assert got.shape == (D, n)
    worst = 0.0
    for r in range(n):
        for b in range(D):
            vals = {}
            for step in (-2, -1, 1, 2):
                Xs = np.array(X, dtype=LD)
                Xs[b, r] = Xs[b, r] + LD(step) * LD(H)
                vals[step] = _evidence(k, Z, np.asfortranarray(Xs.astype(np.float64)), y, variational, model_only)
            d1 = (vals[1] - vals[-1]) / (2 * H)
            d2 = (vals[2] - vals[-2]) / (4 * H)
            third = abs(d2 - d1) / 3.0
            bound = 2.0 * third + 256 * 2.0 ** -53 * max(abs(v) for v in vals.values()) / H
            err = abs(got[b, r] - d1)
            worst = max(worst, err / bound)
            assert err <= bound, (kind, variational, model_only, r, b, got[b, r], d1, err, bound)
    assert np.max(np.abs(got)) > 1e-3  # (the comparison is not one of zeros)
    print("input-gradient reference vs central differences (%s): worst error / bound %.3f" % (kind, worst))


def test_symbol_is_declared_in_every_layer_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gprhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+gprhip_hypers\s*\*\s*h,\s*gprhip_result\s*\*\s*res,"
                     r"\s*double\s*\*\s*grad,\s*double\s*\*\s*coeffs,\s*double\s*\*\s*dl_dinputs,\s*int64_t\s+ld,\s*int\s+on_device\s*\)"
                     % NAME, header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 8
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    assert NAME + "(" in open(os.path.join(ROOT, "include", "gprhip.hpp")).read()


def test_python_layers_carry_the_feature():
    import sys
    from gpr_amd import cov_se_fat, cov_se_iso, fitc_gp
    from gpr_amd.problem import Problem
    assert callable(Problem.eval_input_grad)
    for spec in (cov_se_iso, cov_se_fat):
        GP = fitc_gp.Make_deriv(spec)
        for variant in (GP.FITC, GP.Variational_FITC):
            assert callable(variant.Deriv.Trained.calc_input_gradient)
            assert callable(variant.Deriv.Model.calc_input_gradient)
            assert callable(variant.Deriv.Trained.calc_many)
    # the torch front end is found, and importing the package does not pull torch in
    code = ("import sys, gpr_amd, importlib.util as u; assert 'torch' not in sys.modules; "
            "assert u.find_spec('gpr_amd.autograd') is not None; import gpr_amd.autograd as a; "
            "assert 'torch' not in sys.modules and callable(a.log_evidence)")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_refusals_that_need_no_device():
    """A NULL problem is refused with GPRHIP_EBADARG before anything touches a device."""
    from gpr_amd import _lib
    lib = _lib.load()
    res = _lib.Result()
    h = _lib.Hypers()
    buf = np.zeros(4)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    st = lib.gprhip_eval_input_grad(None, ctypes.byref(h), ctypes.byref(res), ptr, ptr, ctypes.c_void_p(buf.ctypes.data), 1, 0)
    assert st == _lib.EBADARG
    assert b"gprhip_eval_input_grad" in lib.gprhip_last_error()


def test_cpp_mirror_method_builds(tmp_path):
    src = tmp_path / "xg.cpp"
    src.write_text('#include "gprhip.hpp"\n'
                   "int main() {\n"
                   "  auto f = &gpr::Make_deriv<gpr::Cov_se_iso>::run_input_grad;   // (instantiates the templates)\n"
                   "  auto g = &gpr::Make_deriv<gpr::Cov_se_fat>::run_input_grad;\n"
                   "  return (f == nullptr) + (g == nullptr);\n"
                   "}\n")
    exe = tmp_path / "xg"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lgprhip", "-Wl,-rpath," + libdir, "-o", str(exe)])
