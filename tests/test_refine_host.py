"""gprhip_acquire_refine: what can be checked without a GPU -- the declarations of the entry point in every layer, the
argument refusals that need no device, the C++ mirror method, and the step rule itself: gpr_amd/csrc/refine_step.h driven on
analytic objectives by tests/cpp/refine_step_check.cpp (a program of its own under the address and undefined-behaviour
sanitizers), held step for step against tests/refine_ref.py, the same rule in Python."""
import ctypes
import math
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

from tests import acquire_ref as R
from tests import refine_cases as RC
from tests import refine_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_acquire_refine"


def test_symbol_is_declared_in_every_layer_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gprhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+gprhip_acquisition\s*\*\s*acq,\s*const\s+"
                     r"gprhip_refine_options\s*\*\s*opt,\s*const\s+double\s*\*\s*lower,\s*const\s+double\s*\*\s*upper,\s*const\s+"
                     r"double\s*\*\s*scale,\s*const\s+double\s*\*\s*starts,\s*int64_t\s+ld,\s*int64_t\s+ns,\s*double\s*\*\s*x_out,"
                     r"\s*int64_t\s+ldx,\s*double\s*\*\s*values,\s*double\s*\*\s*dvalues,\s*int64_t\s+ldg,\s*int\s*\*\s*evals,"
                     r"\s*int\s*\*\s*accepted,\s*int\s*\*\s*status,\s*double\s*\*\s*trace,\s*int\s+on_device\s*\)" % NAME, header)
    assert re.search(r"GPRHIP_REFINE_ST_CONVERGED = 0, GPRHIP_REFINE_ST_MAX_EVALS = 1, GPRHIP_REFINE_ST_NAN = 2", header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 19
    assert [f for f, _ in _lib.RefineOptions._fields_] == ["max_evals", "step0", "c1", "shrink", "grow", "xtol"]
    assert (_lib.REFINE_ST_CONVERGED, _lib.REFINE_ST_MAX_EVALS, _lib.REFINE_ST_NAN) == (RR.CONVERGED, RR.MAX_EVALS, RR.NAN)
    for name, value in (("GPRHIP_REFINE_MAX_EVALS", _lib.REFINE_MAX_EVALS), ("GPRHIP_REFINE_MAX_STARTS", _lib.REFINE_MAX_STARTS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    step = open(os.path.join(ROOT, "gpr_amd", "csrc", "refine_step.h")).read()
    assert re.search(r"REFINE_CONVERGED = 0, REFINE_MAX_EVALS = 1, REFINE_NAN = 2", step)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    assert NAME + "(" in open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    assert NAME + "(" in open(os.path.join(ROOT, "bindings", "gpr_hip_stubs.c")).read()
    assert '"gprhip_ml_acquire_refine"' in open(os.path.join(ROOT, "bindings", "gpr_hip.ml")).read()
    from gpr_amd.problem import Problem
    assert callable(Problem.acquire_refine)
    assert Problem.REFINE_OUTPUTS == ("x", "values", "dvalues", "evals", "accepted", "status", "trace")


def _acq(**kw):
    from gpr_amd import _lib
    base = dict(kind=R.EI, maximise=1, predictive=0, best=0.0, xi=0.0, kappa=0.0, var_floor=1e-10)
    base.update(kw)
    return _lib.Acquisition(*[base[f] for f, _ in _lib.Acquisition._fields_])


def _opt(**kw):
    from gpr_amd import _lib
    base = dict(RR.DEFAULTS)
    base.update(kw)
    return _lib.RefineOptions(*[base[f] for f, _ in _lib.RefineOptions._fields_])


def test_refusals_that_need_no_device():
    """The refusals of the criterion, of the options, of ns and of the outputs come before anything touches a problem or a
    device: checked with a NULL problem (itself refused, last, once the rest is in order)."""
    from gpr_amd import _lib
    from gpr_amd.problem import Problem
    lib = _lib.load()
    buf = np.zeros(8)
    dp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    vp = ctypes.c_void_p
    nan, inf = float("nan"), float("inf")

    def call(acq=None, opt=None, ns=1, out=True):
        acq = _acq() if acq is None else acq
        opt = _opt() if opt is None else opt
        return lib.gprhip_acquire_refine(None, ctypes.byref(acq) if acq != "null" else None,
                                         ctypes.byref(opt) if opt != "null" else None, dp, dp, None, vp(buf.ctypes.data), 1, ns,
                                         vp(buf.ctypes.data) if out else None, 1, None, None, 1, None, None, None, None, 0)

    cases = [
        (dict(acq=_acq(kind=4)), b"kind"), (dict(acq=_acq(xi=-1e-3)), b"xi"), (dict(acq=_acq(kind=R.BOUND, kappa=-1.0)), b"kappa"),
        (dict(acq=_acq(var_floor=0.0)), b"var_floor"), (dict(acq=_acq(best=nan)), b"best"), (dict(acq="null"), b"acq is NULL"),
        (dict(opt="null"), b"opt is NULL"),
        (dict(opt=_opt(max_evals=0)), b"max_evals"), (dict(opt=_opt(max_evals=_lib.REFINE_MAX_EVALS + 1)), b"max_evals"),
        (dict(opt=_opt(step0=0.0)), b"step0"), (dict(opt=_opt(step0=1.5)), b"step0"), (dict(opt=_opt(step0=nan)), b"step0"),
        (dict(opt=_opt(c1=-0.1)), b"c1"), (dict(opt=_opt(c1=1.0)), b"c1"), (dict(opt=_opt(c1=nan)), b"c1"),
        (dict(opt=_opt(shrink=0.0)), b"shrink"), (dict(opt=_opt(shrink=1.0)), b"shrink"), (dict(opt=_opt(shrink=nan)), b"shrink"),
        (dict(opt=_opt(grow=0.5)), b"grow"), (dict(opt=_opt(grow=inf)), b"grow"), (dict(opt=_opt(grow=nan)), b"grow"),
        (dict(opt=_opt(xtol=-1e-9)), b"xtol"), (dict(opt=_opt(xtol=nan)), b"xtol"),
        (dict(ns=0), b"ns"), (dict(ns=_lib.REFINE_MAX_STARTS + 1), b"ns"),
        (dict(out=False), b"nothing is requested"),
        (dict(), b"invalid arguments"),                                  # all in order but the problem
        (dict(opt=_opt(max_evals=1, step0=1.0, c1=0.0, grow=1.0, xtol=0.0), ns=_lib.REFINE_MAX_STARTS), b"invalid arguments"),
    ]
    for kw, reason in cases:
        assert call(**kw) == _lib.EBADARG, kw
        msg = lib.gprhip_last_error()
        assert msg.startswith(NAME.encode()) and reason in msg, (kw, msg)
    p = Problem.__new__(Problem)
    p._h = ctypes.c_void_p()  # (nothing to destroy)
    p.D = 2
    box = dict(lower=np.zeros(2), upper=np.ones(2), maximise=True, var_floor=1e-10)
    with pytest.raises(ValueError):
        Problem.acquire_refine(p, np.zeros((2, 3)), "ei", want=("x", "gradients"), **box)
    with pytest.raises(ValueError):
        Problem.acquire_refine(p, np.zeros((2, 3)), "mpi", **box)
    with pytest.raises(ValueError):
        Problem.acquire_refine(p, np.zeros((3, 3)), "ei", **box)
    with pytest.raises(ValueError):
        Problem.acquire_refine(p, np.zeros((2, 3)), "ei", **dict(box, lower=np.zeros(3)))
    with pytest.raises(ValueError):
        Problem.acquire_refine(p, np.zeros((2, 3)), "ei", lower=np.zeros(2), upper=np.ones(2), maximise=True)  # no var_floor


def test_cpp_mirror_method_builds(tmp_path):
    """tests/cpp/refine_check.cpp -- Eval::Acquisition::refine of the C++ mirror -- compiles and links; without arguments it
    only prints its usage (no device call)."""
    exe = tmp_path / "refine_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "refine_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr


# ---- the rule: the header under the sanitizers against the Python reference ------------------------------------------------------
LO, HI = (0.0, -1.0), (1.0, 1.0)
STARTS = ((0.1, -0.9), (0.95, 0.7), (0.5, 0.0), (-3.0, 5.0))
SCALE = (1.0, 0.5)
OBJECTIVES = {  # name: (kind, c, m) as in tests/cpp/refine_step_check.cpp
    "inside": (0, (1.0, 1.0), (0.3, 0.4)), "aniso": (0, (1.0, 2.0), (0.3, 0.4)), "face": (0, (1.0, 1.0), (1.7, 0.25)),
    "corner": (0, (1.0, 2.0), (-0.5, 1.5)), "linear": (1, (0.7, -0.2), (0.0, 0.0)), "constant": (2, (0.0, 0.0), (0.0, 0.0)),
    "plateau": (3, (1.0, 1.0), (0.3, 0.4)),
}
OPTS = dict(max_evals=400, step0=0.25, c1=1e-4, shrink=0.5, grow=2.0, xtol=1e-6)
SPECIAL = {"plateau": dict(OPTS, max_evals=200, step0=1.0), "one": dict(OPTS, max_evals=1), "few": dict(OPTS, max_evals=4)}
ALIAS = {"one": "inside", "few": "aniso"}


def _objective(name):
    kind, c, m = OBJECTIVES[name]

    def f(x):
        if kind == 1:
            a = 0.0
            for k in range(2):
                a += c[k] * x[k]
            return a, list(c)
        if kind == 2:
            return 1.5, [0.0, 0.0]
        s, g = 0.0, []
        for k in range(2):
            t = float(x[k]) - m[k]
            s += c[k] * t * t
            g.append(-2.0 * c[k] * t)
        if kind == 3 and x[0] > 0.6:
            return float("nan"), [float("nan")] * 2
        return -s, g
    return f


def _same(a, b):
    return a == b or (a != a and b != b)


def test_rule_under_the_sanitizers_agrees_with_the_python_reference_step_for_step(tmp_path):
    """tests/cpp/refine_step_check.cpp asserts, per case, the status, the known maximiser to xtol w, monotone accepted
    values and evals <= max_evals (and max_evals = 1: the clipped start); its printed trace -- every y, g_y, a_y, alpha and
    accepted flag in hexadecimal floats -- equals refine_ref.refine's bit for bit."""
    exe = tmp_path / "refine_step_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "refine_step_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refine_step_check: ok" in out.stdout, out.stderr[-2000:]
    cases, cur = [], None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "case":
            cur = dict(name=w[1], recs=[])
            cases.append(cur)
        elif w[0] == "rec":
            v = [float.fromhex(t) for t in w[1:-1]]
            cur["recs"].append((v[0:2], v[2:4], v[4], v[5], w[-1] == "1"))
        elif w[0] == "end":
            cur["end"] = (int(w[1]), int(w[2]), int(w[3]), [float.fromhex(t) for t in w[4:6]], float.fromhex(w[6]))
    assert len(cases) == 5 * 4 * 2 + 1 + 2 + 2
    statuses = set()
    for c in cases:
        parts = c["name"].split(".")
        opts = SPECIAL.get(parts[0], OPTS)
        ref = RR.refine(_objective(ALIAS.get(parts[0], parts[0])), STARTS[int(parts[1])], LO, HI,
                        SCALE if parts[-1] == "scaled" else None, **opts)
        assert len(ref["trace"]) == len(c["recs"]) == ref["evals"], c["name"]
        for j, (want, got) in enumerate(zip(ref["trace"], c["recs"])):
            for a, b in zip(list(want[0]) + list(want[1]) + [want[2], want[3]], list(got[0]) + list(got[1]) + [got[2], got[3]]):
                assert _same(a, b), (c["name"], j, want, got)
            assert want[4] == got[4], (c["name"], j)
        status, evals, accepted, x, a = c["end"]
        assert (status, evals, accepted) == (ref["status"], ref["evals"], ref["accepted"]), c["name"]
        assert all(_same(u, v) for u, v in zip(x, ref["x"])) and _same(a, ref["a"]), c["name"]
        statuses.add(status)
    assert statuses == {RR.CONVERGED, RR.MAX_EVALS, RR.NAN}


# ---- PI's coefficients where phi(u) is subnormal ---------------------------------------------------------------------------------
def test_pi_coefficients_where_phi_is_subnormal(tmp_path):
    """acq_point on the host (tests/cpp/acq_point_check.cpp, under the sanitizers) against tests/acquire_ref.py over
    37.2 < |u| < 38.8 -- phi(u) is a subnormal double for 37.6 < |u| < 38.6 -- and across the normal range, with sigma from
    1e-5 to 1: the gradient c_mu dmu + c_v dsigma2 for three (dmu, dsigma2) pairs under the bound that
    tests/test_gpu_acquire.py puts on dvalues, constant and absolute floor included.  Formed from phi itself, the two
    quotients phi / sigma and u phi / (2 v) carried its few bits: a ratio of 6e12 against the constant 30 on this sweep."""
    exe = tmp_path / "acq_point_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "acq_point_check.cpp"), "-o", str(exe)])
    c_pi, eps, tiny = 30.0, 2.0 ** -53, 2.0 ** -1074   # C["pi"], EPS and TINY of tests/test_gpu_acquire.py
    pts = [(float(u * sigma), float(sigma * sigma)) for sigma in (1e-5, 1e-3, 0.03, 0.3, 1.0)
           for u in np.concatenate([np.linspace(-38.8, -37.2, 60), np.linspace(-37.0, 3.0, 20)])]
    inp = "\n".join("%d %s %s" % (R.PI, float.hex(m), float.hex(v)) for m, v in pts) + "\n"
    out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split()
    assert len(lines) == 3 * len(pts)
    worst, subnormal = 0.0, 0
    for i, (m, v) in enumerate(pts):
        a, cmu, cv = (float.fromhex(t) for t in lines[3 * i:3 * i + 3])
        ra, rcmu, rcv, u = R.point(R.PI, m, v, maximise=True, best=0.0, xi=0.0, var_floor=1e-10)
        sigma, f = math.sqrt(v), 1 + u * u
        subnormal += 0 < float(mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi)) < 2.0 ** -1022
        assert abs(mp.mpf(a) - ra) <= c_pi * eps * f * abs(ra) + 8 * tiny
        for dm, ds in ((1.0, 1.0), (3.0, -0.01), (0.1, 5.0)):
            t1, t2 = rcmu * dm, rcv * ds
            floor = 8 * tiny * max(1.0, sigma, abs(dm) + abs(ds) / sigma)
            err = abs(mp.mpf(cmu * dm + cv * ds) - (t1 + t2)) - floor
            if err > 0:
                worst = max(worst, float((err / (mp.mpf(eps) * (abs(t1) + abs(t2))) - 4) / f))
    print("PI gradient ratio c over the sweep: %.3g (bound %g); %d points with a subnormal phi" % (worst, c_pi, subnormal))
    assert subnormal >= 100 and worst <= c_pi, worst


# ---- the seeds of the GPU tests, on the CPU --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
def test_bump_model_has_its_maximiser_inside_and_refinement_beats_both_grids(d):
    """Check 5 of tests/test_gpu_refine.py before the device sees it: on the 80-bit posterior of the bump model the bound
    mu + sigma has its best fine-grid point (64 x finer than the coarse grid) strictly inside the box and off the coarse
    grid, and refine_ref.refine from the coarse grid's top 16 ends above both grids within 40 evaluations."""
    X, y, Z, args = RC.bump(d)
    post = RC.posterior(X, y, Z, args)
    nc = RC.COARSE[d]
    coarse, fine = RC.grid(d, nc), RC.grid(d, 64 * (nc - 1) + 1)
    vc = RC.bound_values(post(coarse))
    vf = np.concatenate([RC.bound_values(post(fine[:, i:i + 20000])) for i in range(0, fine.shape[1], 20000)])
    top = np.argsort(-vc, kind="stable")[:16]
    xf = fine[:, int(np.argmax(vf))]
    assert np.all(xf > 0.02) and np.all(xf < 0.98), xf
    assert float(np.max(vf)) > float(vc[top[0]])
    f = RC.evaluator(post, "bound", maximise=True, kappa=RC.BOUND_KAPPA, var_floor=1e-10)
    runs = [RR.refine(f, coarse[:, i], np.zeros(d), np.ones(d), **dict(RR.DEFAULTS, max_evals=40)) for i in top]
    best = max(runs, key=lambda r: r["a"])
    print("d = %d: coarse %.12g, fine %.12g at %s, refined %.12g at %s" % (d, vc[top[0]], np.max(vf), xf, best["a"], best["x"]))
    assert best["a"] > float(np.max(vf)) > float(vc[top[0]])
    assert np.all(best["x"] > 0.0) and np.all(best["x"] < 1.0) and np.max(np.abs(best["x"] - xf)) < 1.0 / (nc - 1)
