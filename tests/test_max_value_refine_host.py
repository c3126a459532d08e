"""gprhip_acquire_max_value_refine: what can be checked without a GPU -- the declarations of the entry point in every layer, the
argument refusals that need no device (every bad option of tests/test_refine_host.py, every bad extreme or count of
tests/test_max_value_host.py, var_floor), Problem.max_value_search's bookkeeping with refine_top_k on a stand-in problem, and
the seeds of the GPU test's "does its job" check on the 80-bit posterior (tests/max_value_refine_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import max_value_refine_cases as MC
from tests import refine_cases as RC
from tests import refine_ref as RR
from tests.test_max_value_host import _StandIn, mv_numpy
from tests.test_refine_host import _opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_acquire_max_value_refine"


def test_symbol_is_declared_in_every_layer_and_exported():
    text = open(os.path.join(ROOT, "include", "gprhip.h")).read()
    assert "gprhip_acquire_refine does not take this criterion" not in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+double\s*\*\s*extremes\s*,\s*int\s+n_extremes,\s*int\s+"
                     r"maximise,\s*double\s+var_floor,\s*const\s+gprhip_refine_options\s*\*\s*opt,\s*const\s+double\s*\*\s*lower,"
                     r"\s*const\s+double\s*\*\s*upper,\s*const\s+double\s*\*\s*scale,\s*const\s+double\s*\*\s*starts,\s*int64_t\s+ld,"
                     r"\s*int64_t\s+ns,\s*double\s*\*\s*x_out,\s*int64_t\s+ldx,\s*double\s*\*\s*values,\s*double\s*\*\s*dvalues,"
                     r"\s*int64_t\s+ldg,\s*int\s*\*\s*evals,\s*int\s*\*\s*accepted,\s*int\s*\*\s*status,\s*double\s*\*\s*trace,"
                     r"\s*int\s+on_device\s*\)" % NAME, header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 22
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    hpp = open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    assert NAME + "(" in hpp and "refine_max_value(" in hpp
    assert NAME + "(" in open(os.path.join(ROOT, "bindings", "gpr_hip_stubs.c")).read()
    assert '"gprhip_ml_acquire_max_value_refine"' in open(os.path.join(ROOT, "bindings", "gpr_hip.ml")).read()
    from gpr_amd.problem import Problem
    assert callable(Problem.acquire_max_value_refine)


def test_refusals_that_need_no_device():
    """The refusals of the extremes, of var_floor, of the options, of ns and of the outputs come before anything touches a
    problem or a device: checked with a NULL problem (itself refused, last, once the rest is in order)."""
    from gpr_amd import _lib
    from gpr_amd.problem import Problem
    lib = _lib.load()
    buf = np.zeros(8)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    vp = ctypes.c_void_p
    nan, inf = float("nan"), float("inf")
    ext = np.linspace(0.1, 0.9, 65)

    def call(extremes=ext, n=3, var_floor=1e-10, opt=None, ns=1, out=True):
        opt = _opt() if opt is None else opt
        return lib.gprhip_acquire_max_value_refine(None, dp(extremes) if extremes is not None else None, n, 1, var_floor,
                                                   ctypes.byref(opt) if opt != "null" else None, dp(buf), dp(buf), None,
                                                   vp(buf.ctypes.data), 1, ns, vp(buf.ctypes.data) if out else None, 1, None, None,
                                                   1, None, None, None, None, 0)

    def bad(j, v):
        e = ext.copy()
        e[j] = v
        return e

    cases = [
        # the extremes and their count, as tests/test_max_value_host.py
        (dict(n=0), b"n_extremes"), (dict(n=-1), b"n_extremes"), (dict(n=65), b"n_extremes"),
        (dict(extremes=None), b"extremes is NULL"),
        (dict(extremes=bad(2, nan)), b"extremes must be finite"), (dict(extremes=bad(0, inf)), b"extremes must be finite"),
        (dict(extremes=bad(63, -inf), n=64), b"extremes must be finite"),
        (dict(var_floor=0.0), b"var_floor"), (dict(var_floor=-1.0), b"var_floor"), (dict(var_floor=inf), b"var_floor"),
        (dict(var_floor=nan), b"var_floor"),
        # the options, ns and the outputs, as tests/test_refine_host.py
        (dict(opt="null"), b"opt is NULL"),
        (dict(opt=_opt(max_evals=0)), b"max_evals"), (dict(opt=_opt(max_evals=_lib.REFINE_MAX_EVALS + 1)), b"max_evals"),
        (dict(opt=_opt(step0=0.0)), b"step0"), (dict(opt=_opt(step0=1.5)), b"step0"), (dict(opt=_opt(step0=nan)), b"step0"),
        (dict(opt=_opt(c1=-0.1)), b"c1"), (dict(opt=_opt(c1=1.0)), b"c1"), (dict(opt=_opt(c1=nan)), b"c1"),
        (dict(opt=_opt(shrink=0.0)), b"shrink"), (dict(opt=_opt(shrink=1.0)), b"shrink"), (dict(opt=_opt(shrink=nan)), b"shrink"),
        (dict(opt=_opt(grow=0.5)), b"grow"), (dict(opt=_opt(grow=inf)), b"grow"), (dict(opt=_opt(grow=nan)), b"grow"),
        (dict(opt=_opt(xtol=-1e-9)), b"xtol"), (dict(opt=_opt(xtol=nan)), b"xtol"),
        (dict(ns=0), b"ns"), (dict(ns=_lib.REFINE_MAX_STARTS + 1), b"ns"),
        (dict(out=False), b"nothing is requested"),
        (dict(), b"invalid arguments"),                               # all in order but the problem
        (dict(extremes=bad(3, nan)), b"invalid arguments"),           # (a non-finite entry beyond n_extremes is not read)
        (dict(n=64, opt=_opt(max_evals=1, step0=1.0, c1=0.0, grow=1.0, xtol=0.0), ns=_lib.REFINE_MAX_STARTS), b"invalid arguments"),
    ]
    for kw, reason in cases:
        assert call(**kw) == _lib.EBADARG, kw
        msg = lib.gprhip_last_error()
        assert msg.startswith(NAME.encode() + b":") and reason in msg, (kw, msg)
    p = Problem.__new__(Problem)
    p._h = ctypes.c_void_p()  # (nothing to destroy)
    p.D = 2
    box = dict(lower=np.zeros(2), upper=np.ones(2), maximise=True, var_floor=1e-10)
    with pytest.raises(ValueError):
        Problem.acquire_max_value_refine(p, np.zeros((2, 3)), [0.1], want=("x", "gradients"), **box)
    with pytest.raises(ValueError):
        Problem.acquire_max_value_refine(p, np.zeros((2, 3)), [[0.1]], **box)
    with pytest.raises(ValueError):
        Problem.acquire_max_value_refine(p, np.zeros((3, 3)), [0.1], **box)
    with pytest.raises(ValueError):
        Problem.acquire_max_value_refine(p, np.zeros((2, 3)), [0.1], **dict(box, lower=np.zeros(3)))
    with pytest.raises(ValueError):   # var_floor missing: no model state seen, it has no default
        Problem.acquire_max_value_refine(p, np.zeros((2, 3)), [0.1], lower=np.zeros(2), upper=np.ones(2), maximise=True)


# ---- Problem.max_value_search(refine_top_k=...) on a stand-in problem ------------------------------------------------------------
class _StandInRefine(_StandIn):
    """tests/test_max_value_host.py's stand-in with the top_k outputs of acquire_max_value and the new call"""

    def __init__(self, *a, acq_top_index):
        super().__init__(*a)
        self.acq_top_index = np.asarray(acq_top_index, dtype=np.int64)

    def acquire_max_value(self, grid, extremes, **kw):
        out = super().acquire_max_value(grid, extremes, **kw)
        if kw["top_k"] > 0:
            out["top_index"] = self.acq_top_index[:kw["top_k"]]
        return out

    def acquire_max_value_refine(self, starts, extremes, **kw):
        self.calls.append(("acquire_max_value_refine", dict(kw, starts=np.array(starts), extremes=np.array(extremes))))
        ns = starts.shape[1]
        return dict(x=np.asfortranarray(starts + 0.25), values=np.arange(ns, dtype=np.float64),
                    dvalues=np.asfortranarray(np.zeros_like(starts)), status=np.zeros(ns, dtype=np.int32))


def _search(q, maximise, **kw):
    from gpr_amd.problem import Problem
    D, m, nt, nd = 2, 5, 9, 3
    grid = np.asfortranarray(np.arange(D * nt, dtype=np.float64).reshape(D, nt))
    out = Problem.max_value_search(q, np.zeros((m, nd)), np.zeros(D), np.ones(D), grid, 2, dict(max_evals=7), maximise=maximise,
                                   var_floor=1e-12, **kw)
    return grid, out


def _stand_in():
    top_index = np.asfortranarray(np.array([[4, 7, 2], [1, -1, 8]], dtype=np.int64))
    objective = np.array([0.25, 1.5, -0.75, 2.0, 2.0])
    return _StandInRefine(2, 5, objective, top_index, acq_top_index=[6, 3, -1, 0, 5])


@pytest.mark.parametrize("maximise", [True, False], ids=["max", "min"])
def test_max_value_search_refines_the_best_grid_candidates(maximise):
    """refine_top_k = 0: the three calls of today with today's arguments and keys, none of the new ones.  refine_top_k = k:
    acquire_max_value with top_k = max(acquire_top_k, k), then acquire_max_value_refine last, from the best k qualifying grid
    candidates (a -1 is no candidate) in their order, inside the search's box, with the extremes and var_floor of the grid
    call and candidate_refine_options."""
    q = _stand_in()
    grid, out = _search(q, maximise)
    assert [c[0] for c in q.calls] == ["sample_paths", "sample_paths_refine", "acquire_max_value"]
    assert q.calls[2][1]["top_k"] == 0 and set(out) == {"values", "extremes", "extreme_x"}
    q0 = _stand_in()
    _, out0 = _search(q0, maximise, refine_top_k=0, candidate_refine_options=dict(max_evals=3))
    assert [c[0] for c in q0.calls] == [c[0] for c in q.calls] and set(out0) == set(out)
    assert all(np.array_equal(out0[k], out[k]) for k in out)
    assert {k: v for k, v in q0.calls[2][1].items() if k != "extremes"} == {k: v for k, v in q.calls[2][1].items() if k != "extremes"}

    for k, acquire_top_k, want_starts in ((3, 0, [6, 3]), (2, 5, [6, 3]), (4, 1, [6, 3, 0])):
        q = _stand_in()
        grid, out = _search(q, maximise, refine_top_k=k, acquire_top_k=acquire_top_k, candidate_refine_options=dict(max_evals=9, xtol=1e-6))
        assert [c[0] for c in q.calls] == ["sample_paths", "sample_paths_refine", "acquire_max_value", "acquire_max_value_refine"]
        mv, rf = q.calls[2][1], q.calls[3][1]
        assert mv["top_k"] == max(acquire_top_k, k)
        assert np.array_equal(rf["starts"], grid[:, want_starts]) and np.array_equal(rf["extremes"], mv["extremes"])
        assert rf["maximise"] == maximise and rf["var_floor"] == 1e-12 and rf["max_evals"] == 9 and rf["xtol"] == 1e-6
        assert np.array_equal(rf["lower"], np.zeros(2)) and np.array_equal(rf["upper"], np.ones(2))
        assert set(rf["want"]) == {"x", "values", "dvalues", "status"}
        n = len(want_starts)
        assert np.array_equal(out["refined_x"], grid[:, want_starts] + 0.25) and np.array_equal(out["refined_values"], np.arange(n))
        assert out["refined_dvalues"].shape == (2, n) and out["refined_status"].shape == (n,)
        assert np.array_equal(out["values"], [mv_numpy(0.0, 1.0, mv["extremes"], maximise, 1e-12)[0]])
    with pytest.raises(ValueError):
        _search(_stand_in(), maximise, refine_top_k=-1)


# ---- the seeds of the GPU test's "does its job" check, on the CPU ----------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("d", [1, 2])
def test_bump_model_has_its_maximiser_inside_and_refinement_beats_both_grids(d, S):
    """On the 80-bit posterior of the bump model, with the extremes of tests/max_value_refine_cases.py's rule from the coarse
    grid: the criterion's best fine-grid point (64 x finer than the coarse grid) lies strictly inside the box and off the
    coarse grid, and refine_ref.refine from the coarse grid's top 16 ends above both grids within 40 evaluations."""
    X, y, Z, args = RC.bump(d)
    post = RC.posterior(X, y, Z, args)
    nc = RC.COARSE[d]
    coarse, fine = RC.grid(d, nc), RC.grid(d, 64 * (nc - 1) + 1)
    qc = post(coarse)
    ext = MC.extremes(qc["means"], qc["variances"], S, True)
    vc = MC.values_f64(qc["means"], qc["variances"], ext, True)
    vf = np.concatenate([MC.values_f64(q["means"], q["variances"], ext, True)
                         for q in (post(fine[:, i:i + 20000]) for i in range(0, fine.shape[1], 20000))])
    top = np.argsort(-vc, kind="stable")[:16]
    xf = fine[:, int(np.argmax(vf))]
    assert np.all(xf > 0.02) and np.all(xf < 0.98), xf
    assert float(np.max(vf)) > float(vc[top[0]])
    assert not np.any(np.all(np.abs(coarse - xf[:, None]) < 1e-12, axis=0))
    f = MC.evaluator(post, ext, True)
    runs = [RR.refine(f, coarse[:, i], np.zeros(d), np.ones(d), **dict(RR.DEFAULTS, max_evals=40)) for i in top]
    best = max(runs, key=lambda r: r["a"])
    print("d = %d, S = %d: coarse %.12g, fine %.12g at %s, refined %.12g at %s" % (d, S, vc[top[0]], np.max(vf), xf, best["a"], best["x"]))
    assert best["a"] > float(np.max(vf)) > float(vc[top[0]])
    assert np.all(best["x"] > 0.0) and np.all(best["x"] < 1.0) and np.max(np.abs(best["x"] - xf)) < 1.0 / (nc - 1)
