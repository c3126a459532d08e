"""The acquisition criteria of gprhip_acquire: what can be checked without a GPU -- the reference formulas the GPU tests use
(tests/acquire_ref.py, mpmath at 50 digits) against derivatives of themselves, LOG_EI against the logarithm of EI, the
declarations of the entry point in every layer, and the argument refusals that need no device."""
import ctypes
import os
import re
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

from tests import acquire_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_acquire"
US = (-40, -8, -1, 0, 1, 8)
XIS = (0.0, 0.3)
BEST, VAR, KAPPA = 0.3, 0.04, 1.7


def _mu_at(u, maximise, xi, var=VAR):
    """the mean at which delta / sigma = u"""
    s = 1 if maximise else -1
    return mp.mpf(BEST) + s * (mp.mpf(u) * mp.sqrt(mp.mpf(var)) + mp.mpf(xi))


@pytest.mark.parametrize("maximise", [True, False], ids=["max", "min"])
@pytest.mark.parametrize("kind", R.KINDS, ids=[R.KIND_NAMES[k] for k in R.KINDS])
def test_coefficients_are_the_derivatives_of_the_value(kind, maximise):
    """c_mu and c_v of the table equal mpmath.diff of the value in mu and in sigma2 (relative 1e-25 at 60 digits; where the
    coefficient is exactly 0 -- c_v of PI at u = 0 -- the derivative is below 1e-25 of the value's scale); a clamped point has
    c_v = 0 and the value and c_mu of the point (mu, var_floor)."""
    with mp.workdps(60):
        for u in US:
            for xi in XIS:
                kw = dict(maximise=maximise, best=BEST, xi=xi, kappa=KAPPA, var_floor=1e-12)
                mu = _mu_at(u, maximise, xi)
                a, cmu, cv, uu = R.point(kind, mu, mp.mpf(VAR), **kw)
                assert abs(uu - u) < mp.mpf(10) ** -40
                dmu = mp.diff(lambda t: R.value(kind, t, mp.mpf(VAR), **kw), mu)
                dv = mp.diff(lambda t: R.value(kind, mu, t, **kw), mp.mpf(VAR))
                for got, ref in ((cmu, dmu), (cv, dv)):
                    scale = abs(ref) if ref != 0 else 1
                    assert abs(got - ref) <= mp.mpf(10) ** -25 * max(scale, abs(got)), (kind, u, xi, got, ref)
                # clamped: the variance lies below the floor
                kc = dict(kw, var_floor=VAR)
                ac, cmuc, cvc, uc = R.point(kind, mu, mp.mpf(VAR) / 7, **kc)
                assert cvc == 0 and abs(ac - a) <= mp.mpf(10) ** -45 * max(abs(a), 1) and abs(cmuc - cmu) <= mp.mpf(10) ** -45 * abs(cmu)
                assert abs(uc - u) < mp.mpf(10) ** -40


@pytest.mark.parametrize("maximise", [True, False], ids=["max", "min"])
def test_log_ei_is_the_logarithm_of_ei(maximise):
    """wherever EI does not underflow -- at 50 digits everywhere on the grid -- and its coefficients are EI's over EI"""
    for u in US:
        for xi in XIS:
            kw = dict(maximise=maximise, best=BEST, xi=xi, var_floor=1e-12)
            mu = _mu_at(u, maximise, xi)
            a, cmu, cv, _ = R.point(R.EI, mu, VAR, **kw)
            la, lcmu, lcv, _ = R.point(R.LOG_EI, mu, VAR, **kw)
            with mp.workdps(R.DPS):
                assert a > 0
                assert abs(la - mp.log(a)) <= mp.mpf(10) ** -40 * max(1, abs(la))
                assert abs(lcmu - cmu / a) <= mp.mpf(10) ** -40 * abs(lcmu) and abs(lcv - cv / a) <= mp.mpf(10) ** -40 * abs(lcv)
    # EI at u = -40 lies below the float64 range, LOG_EI does not
    a, la = (R.point(k, _mu_at(-40, maximise, 0.0), VAR, maximise=maximise, best=BEST)[0] for k in (R.EI, R.LOG_EI))
    assert float(a) == 0.0 and np.isfinite(float(la)) and float(la) < -800


def test_symbol_is_declared_in_every_layer_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gprhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+gprhip_acquisition\s*\*\s*acq,\s*const\s+double\s*\*"
                     r"\s*test_inputs,\s*int64_t\s+ld,\s*int64_t\s+nt,\s*double\s*\*\s*values,\s*double\s*\*\s*dvalues,\s*int64_t\s+ldg,"
                     r"\s*double\s*\*\s*means,\s*double\s*\*\s*variances,\s*int\s+top_k,\s*int64_t\s*\*\s*top_index,\s*double\s*\*"
                     r"\s*top_values,\s*double\s*\*\s*top_dvalues,\s*int\s+on_device\s*\)" % NAME, header)
    assert re.search(r"GPRHIP_ACQ_EI = 0, GPRHIP_ACQ_LOG_EI = 1, GPRHIP_ACQ_PI = 2, GPRHIP_ACQ_BOUND = 3", header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 15
    assert [f for f, _ in _lib.Acquisition._fields_] == ["kind", "maximise", "predictive", "best", "xi", "kappa", "var_floor"]
    assert (_lib.ACQ_EI, _lib.ACQ_LOG_EI, _lib.ACQ_PI, _lib.ACQ_BOUND) == (R.EI, R.LOG_EI, R.PI, R.BOUND)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    assert NAME + "(" in open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    assert NAME + "(" in open(os.path.join(ROOT, "bindings", "gpr_hip_stubs.c")).read()
    assert '"gprhip_ml_acquire"' in open(os.path.join(ROOT, "bindings", "gpr_hip.ml")).read()


def test_python_layers_carry_the_feature():
    from gpr_amd import cov_se_fat, cov_se_iso, fitc_gp
    from gpr_amd.problem import Problem
    assert callable(Problem.acquire)
    assert Problem.ACQUIRE_OUTPUTS == ("values", "dvalues", "means", "variances")
    for spec in (cov_se_iso, cov_se_fat):
        GP = fitc_gp.Make_deriv(spec)
        for variant in (GP.FITC, GP.Variational_FITC):
            assert callable(variant.Eval.Acquisition.calc)
    code = ("import sys, gpr_amd, importlib.util as u; assert 'torch' not in sys.modules; "
            "import gpr_amd.autograd as a; assert 'torch' not in sys.modules and callable(a.acquire)")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def _acq(**kw):
    from gpr_amd import _lib
    base = dict(kind=R.EI, maximise=1, predictive=0, best=0.0, xi=0.0, kappa=0.0, var_floor=1e-10)
    base.update(kw)
    return _lib.Acquisition(*[base[f] for f, _ in _lib.Acquisition._fields_])


def test_refusals_that_need_no_device():
    """Every argument refusal of the criterion and of top_k comes before anything touches a problem or a device: checked with
    a NULL problem (itself refused, last, once the rest is in order) -- the status, the function's name and the reason in
    gprhip_last_error()."""
    from gpr_amd import _lib
    from gpr_amd.problem import Problem
    lib = _lib.load()
    buf = np.zeros(8)
    idx = np.zeros(64, dtype=np.int64)
    vp = ctypes.c_void_p
    ip = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def call(acq, values=True, top_k=0, top_index=None):
        return lib.gprhip_acquire(None, ctypes.byref(acq) if acq is not None else None, vp(buf.ctypes.data), 1, 1,
                                  vp(buf.ctypes.data) if values else None, None, 1, None, None, top_k, top_index, None, None, 0)

    cases = [
        (dict(acq=_acq(kind=4)), b"kind"), (dict(acq=_acq(kind=-1)), b"kind"),
        (dict(acq=_acq(xi=-1e-3)), b"xi"), (dict(acq=_acq(kind=R.BOUND, kappa=-1.0)), b"kappa"),
        (dict(acq=_acq(xi=float("nan"))), b"xi"),
        (dict(acq=_acq(var_floor=0.0)), b"var_floor"), (dict(acq=_acq(var_floor=-1.0)), b"var_floor"),
        (dict(acq=_acq(var_floor=float("inf"))), b"var_floor"), (dict(acq=_acq(var_floor=float("nan"))), b"var_floor"),
        (dict(acq=_acq(best=float("inf"))), b"best"), (dict(acq=_acq(best=float("nan"))), b"best"),
        (dict(acq=_acq(), top_k=-1, top_index=ip), b"top_k"), (dict(acq=_acq(), top_k=65, top_index=ip), b"top_k"),
        (dict(acq=_acq(), top_k=3, top_index=None), b"top_index"),
        (dict(acq=_acq(), values=False), b"nothing is requested"),
        (dict(acq=None), b"invalid arguments"),
        (dict(acq=_acq()), b"invalid arguments"),                 # all in order but the problem
        (dict(acq=_acq(), top_k=64, top_index=ip), b"invalid arguments"),
    ]
    for kw, reason in cases:
        assert call(**kw) == _lib.EBADARG, kw
        msg = lib.gprhip_last_error()
        assert msg.startswith(b"gprhip_acquire") and reason in msg, (kw, msg)
    p = Problem.__new__(Problem)
    p._h = ctypes.c_void_p()  # (nothing to destroy)
    p.D = 2
    with pytest.raises(ValueError):
        Problem.acquire(p, np.zeros((2, 3)), "ei", maximise=True, var_floor=1e-10, want=("values", "gradients"))
    with pytest.raises(ValueError):
        Problem.acquire(p, np.zeros((2, 3)), "mpi", maximise=True, var_floor=1e-10)
    with pytest.raises(ValueError):
        Problem.acquire(p, np.zeros((3, 3)), "ei", maximise=True, var_floor=1e-10)
    with pytest.raises(ValueError):
        Problem.acquire(p, np.zeros((2, 3)), "ei", maximise=True)   # no model state seen: var_floor has no default


def test_cpp_mirror_method_builds(tmp_path):
    """tests/cpp/acquire_check.cpp -- Eval::Acquisition::calc of the C++ mirror -- compiles and links; without arguments it
    only prints its usage (no device call)."""
    exe = tmp_path / "acquire_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "acquire_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr
