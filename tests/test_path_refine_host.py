"""gprhip_sample_paths_refine: what can be checked without a GPU -- the declarations of the entry point in every layer, the
argument refusals that need no device (the checks live in the entry point itself, not in a host header), the C++ mirror
method, and the seeds of the GPU tests: on the 80-bit evaluator of tests/path_refine_cases.py the reference run of the rule
stays outside the Armijo tie band, and on the bump model every draw's maximiser lies inside the box and off the coarse grid
while the refined top 16 beat both grids."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import path_refine_cases as PC
from tests import refine_cases as RC
from tests import refine_ref as RR
from tests import sample_paths_ref as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_sample_paths_refine"


def test_symbol_is_declared_in_every_layer_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gprhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+double\s*\*\s*z,\s*int64_t\s+ldz,\s*int\s+nd,\s*int\s+"
                     r"maximise,\s*const\s+gprhip_refine_options\s*\*\s*opt,\s*const\s+double\s*\*\s*lower,\s*const\s+double\s*\*\s*"
                     r"upper,\s*const\s+double\s*\*\s*scale,\s*const\s+double\s*\*\s*starts,\s*int64_t\s+ld,\s*int64_t\s+ns,\s*const\s+"
                     r"int\s*\*\s*draw_of,\s*double\s*\*\s*x_out,\s*int64_t\s+ldx,\s*double\s*\*\s*values,\s*double\s*\*\s*dvalues,"
                     r"\s*int64_t\s+ldg,\s*int\s*\*\s*evals,\s*int\s*\*\s*accepted,\s*int\s*\*\s*status,\s*double\s*\*\s*trace,\s*"
                     r"int\s+on_device\s*\)" % NAME, header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 23
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    assert NAME + "(" in open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    assert NAME + "(" in open(os.path.join(ROOT, "bindings", "gpr_hip_stubs.c")).read()
    assert '"gprhip_ml_sample_paths_refine"' in open(os.path.join(ROOT, "bindings", "gpr_hip.ml")).read()
    assert "path_refine.hip" in open(os.path.join(ROOT, "gpr_amd", "csrc", "Makefile")).read()
    from gpr_amd.problem import Problem
    assert callable(Problem.sample_paths_refine)
    # the contract's words: the objective, not the unsigned path; the old limit sentence points at the new call
    full = open(os.path.join(ROOT, "include", "gprhip.h")).read()
    assert "drawn sample paths are not refined" not in full and "not the unsigned path" in full


def _opt(**kw):
    from gpr_amd import _lib
    base = dict(RR.DEFAULTS)
    base.update(kw)
    return _lib.RefineOptions(*[base[f] for f, _ in _lib.RefineOptions._fields_])


def test_refusals_that_need_no_device():
    """nd, the options, ns and the outputs are refused before anything touches a problem or a device: checked with a NULL
    problem (itself refused, last, once the rest is in order)."""
    from gpr_amd import _lib
    from gpr_amd.problem import Problem
    lib = _lib.load()
    buf = np.zeros(8)
    dr = np.zeros(8, dtype=np.int32)
    dp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = dr.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    vp = ctypes.c_void_p
    nan, inf = float("nan"), float("inf")

    def call(opt=None, ns=1, nd=1, out=True):
        opt = _opt() if opt is None else opt
        return lib.gprhip_sample_paths_refine(None, dp, 1, nd, 1, ctypes.byref(opt) if opt != "null" else None, dp, dp, None,
                                              vp(buf.ctypes.data), 1, ns, ip, vp(buf.ctypes.data) if out else None, 1, None, None, 1,
                                              None, None, None, None, 0)

    cases = [
        (dict(nd=0), b"nd"), (dict(nd=65), b"nd"), (dict(opt="null"), b"opt is NULL"),
        (dict(opt=_opt(max_evals=0)), b"max_evals"), (dict(opt=_opt(max_evals=_lib.REFINE_MAX_EVALS + 1)), b"max_evals"),
        (dict(opt=_opt(step0=0.0)), b"step0"), (dict(opt=_opt(step0=1.5)), b"step0"), (dict(opt=_opt(step0=nan)), b"step0"),
        (dict(opt=_opt(c1=-0.1)), b"c1"), (dict(opt=_opt(c1=1.0)), b"c1"), (dict(opt=_opt(c1=nan)), b"c1"),
        (dict(opt=_opt(shrink=0.0)), b"shrink"), (dict(opt=_opt(shrink=1.0)), b"shrink"), (dict(opt=_opt(shrink=nan)), b"shrink"),
        (dict(opt=_opt(grow=0.5)), b"grow"), (dict(opt=_opt(grow=inf)), b"grow"), (dict(opt=_opt(grow=nan)), b"grow"),
        (dict(opt=_opt(xtol=-1e-9)), b"xtol"), (dict(opt=_opt(xtol=nan)), b"xtol"),
        (dict(ns=0), b"ns"), (dict(ns=_lib.REFINE_MAX_STARTS + 1), b"ns"),
        (dict(out=False), b"nothing is requested"),
        (dict(), b"invalid arguments"),                                  # all in order but the problem
        (dict(nd=64, opt=_opt(max_evals=1, step0=1.0, c1=0.0, grow=1.0, xtol=0.0)), b"invalid arguments"),
    ]
    for kw, reason in cases:
        assert call(**kw) == _lib.EBADARG, kw
        msg = lib.gprhip_last_error()
        assert msg.startswith(NAME.encode()) and reason in msg, (kw, msg)
    p = Problem.__new__(Problem)
    p._h = ctypes.c_void_p()  # (nothing to destroy)
    p.D, p.m = 2, 4
    box = dict(lower=np.zeros(2), upper=np.ones(2))
    z, d3 = np.zeros((4, 2)), np.zeros(3, dtype=np.int32)
    with pytest.raises(ValueError):
        Problem.sample_paths_refine(p, np.zeros((2, 3)), z, d3, want=("x", "gradients"), **box)
    with pytest.raises(ValueError):
        Problem.sample_paths_refine(p, np.zeros((2, 3)), np.zeros((5, 2)), d3, **box)     # z is not m x nd
    with pytest.raises(ValueError):
        Problem.sample_paths_refine(p, np.zeros((3, 3)), z, d3, **box)                    # starts are not D x ns
    with pytest.raises(ValueError):
        Problem.sample_paths_refine(p, np.zeros((2, 3)), z, d3[:2], **box)                # draw_of is not ns long
    with pytest.raises(ValueError):
        Problem.sample_paths_refine(p, np.zeros((2, 3)), z, d3, **dict(box, lower=np.zeros(3)))
    with pytest.raises(ValueError):
        Problem.sample_paths_refine(p, 0, z, d3, out_device_ptrs={}, **box)               # device buffers need ns


def test_cpp_mirror_method_builds(tmp_path):
    """tests/cpp/path_refine_check.cpp -- Eval::Path_sampler::refine of the C++ mirror -- compiles and links; without
    arguments it only prints its usage (no device call)."""
    exe = tmp_path / "path_refine_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "path_refine_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr


def reference_ties(key, nd, ns, form, opts, cases=((True, False), (False, True), (True, True), (False, False))):
    """(records, records inside the tie band) of tests/refine_ref.py over the 80-bit evaluator on the GPU test's own calls of
    one shape (tools/path_refine_precheck.py prints them per shape)"""
    lo, hi = PC.box(key)
    D = len(lo)
    m = PC.model(key)[2].shape[1]
    z, dr = PC.draws(m, nd), PC.draw_of(ns, nd, form)
    records = ties = 0
    for ci, (maximise, scaled) in enumerate(cases):
        scale = np.linspace(0.5, 1.5, D) if scaled else None
        S = PC.starts(key, ns, 7 * ns + ci)
        f = PC.evaluator(key, z, 1.0 if maximise else -1.0)
        for i in range(ns):
            run = RR.refine(lambda x, j=int(dr[i]): f(x, j), S[:, i], lo, hi, scale, **opts)
            x, g, a = (np.array(v) if k < 2 else v for k, v in enumerate(run["trace"][0][:3]))
            for y, gy, ay, al, acc in run["trace"][1:]:
                delta = np.array(y) - x
                records += 1
                if abs(ay - (a + opts["c1"] * float(np.dot(g, delta)))) < PC.tie_band(a, ay, opts["c1"], g, delta):
                    ties += 1
                if acc:
                    x, g, a = np.array(y), np.array(gy), ay
    return records, ties


def test_reference_run_of_a_gpu_case_stays_outside_the_tie_band():
    """one small shape of each route's kind here (all of them: tools/path_refine_precheck.py -> profiles/path_refine_precheck.txt);
    the projection case runs the evaluator through tproj as the device does"""
    opts = dict(max_evals=12, step0=0.1, c1=1e-4, shrink=0.5, grow=2.0, xtol=1e-7)
    for key, nd, ns, form in ((PC.key_of(5, 3), 17, 17, "i"), (PC.key_of(20, 2, 5), 17, 17, "i")):
        records, ties = reference_ties(key, nd, ns, form, opts, cases=((True, False), (False, True)))
        print(key, records, ties)
        assert records > 100 and ties <= 0.01 * records, (key, records, ties)


BUMP_DRAWS, BUMP_SEED = 4, 0   # as tests/test_gpu_path_refine.py


@pytest.mark.parametrize("d", [1, 2])
def test_bump_draws_have_their_maximisers_inside_and_refinement_beats_both_grids(d):
    """Check 5 of tests/test_gpu_path_refine.py before the device sees it: on the 80-bit weights of the bump model every one
    of the 4 draws has its best fine-grid point (64 x finer than the coarse grid) strictly inside the box and off the coarse
    grid, and refine_ref.refine from the coarse grid's top 16 of that draw ends above both grids within 40 evaluations."""
    X, y, Z, args = RC.bump(d)
    k = RC.oracle_kernel(args)
    state = SP.path_state(k, Z, X, y, RC.SIGMA2)
    z = PC.draws(RC.BUMP_M, BUMP_DRAWS, BUMP_SEED)
    nc = RC.COARSE[d]
    coarse, fine = RC.grid(d, nc), RC.grid(d, 64 * (nc - 1) + 1)
    Fc = SP.sample_paths_from_state(k, Z, state, coarse, z, RC.SIGMA2)["paths"]
    Ff = np.concatenate([SP.sample_paths_from_state(k, Z, state, fine[:, i:i + 20000], z, RC.SIGMA2)["paths"]
                         for i in range(0, fine.shape[1], 20000)])
    for j in range(BUMP_DRAWS):
        def f(x, j=j):
            r = SP.sample_paths_from_state(k, Z, state, np.asarray(x, dtype=np.float64).reshape(-1, 1), z[:, j], RC.SIGMA2,
                                           grad_at=[(0, 0)])
            return float(r["paths"][0, 0]), [float(t) for t in r["grads"][:, 0]]
        top = np.argsort(-Fc[:, j], kind="stable")[:16]
        xf = fine[:, int(np.argmax(Ff[:, j]))]
        assert np.all(xf > 0.02) and np.all(xf < 0.98), (j, xf)
        assert float(np.max(Ff[:, j])) > float(Fc[top[0], j]), j
        runs = [RR.refine(f, coarse[:, i], np.zeros(d), np.ones(d), **dict(RR.DEFAULTS, max_evals=40)) for i in top]
        best = max(runs, key=lambda r: r["a"])
        print("d = %d, draw %d: coarse %.12g, fine %.12g at %s, refined %.12g at %s"
              % (d, j, Fc[top[0], j], np.max(Ff[:, j]), xf, best["a"], best["x"]))
        assert best["a"] > float(np.max(Ff[:, j])) > float(Fc[top[0], j]), j
        assert np.all(best["x"] > 0.0) and np.all(best["x"] < 1.0), j
