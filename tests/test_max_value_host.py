"""Max-value entropy search (gprhip_acquire_max_value): what can be checked without a GPU -- the point function of the kernels'
epilogue (gpr_amd/csrc/mv_math.h, compiled for the host by tests/cpp/mv_point_check.cpp under the address and
undefined-behaviour sanitizers) against mpmath at 50 digits (tests/max_value_ref.py) with planted defects that the bounds
must catch, the argument refusals that need no device, the declarations in every layer, and Problem.max_value_search's
bookkeeping on a stand-in problem."""
import ctypes
import math
import os
import re
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

from tests import margins as M
from tests import max_value_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_acquire_max_value"
FLOOR = 1e-12
SIGMAS = (1e-5, 0.03, 1.0)
MU = 0.3
# gamma in [-1000, 40]: 0, the switch points +-5 and +-8 of acq_mills with a neighbour on either side, the band 37.6 .. 38.6
# where phi goes subnormal.  At MU = 0.3 an extreme cannot carry a gamma below about 1e-16 sigma: +-1e-300 and the other tiny
# ones are TINY_GAMMAS, placed at mu = 0, sigma = 1 where the extreme is s gamma itself (_grid), and +-2^-50 / sigma is the
# smallest here that survives the rounding of MU + s gamma sigma
GAMMAS = ([0.0, 5.0, -5.0, 8.0, -8.0, -1000.0, -300.0, -100.0, -40.0, -30.0, -12.0, -7.9, -8.1, -5.1, -4.9, -2.0,
           -1.0, -0.3, 0.3, 1.0, 2.0, 4.9, 5.1, 7.9, 8.1, 12.0, 20.0, 30.0, 37.0, 40.0] + [37.6 + 0.1 * i for i in range(11)])
TINY_GAMMAS = (1e-300, -1e-300, 5e-324, -5e-324, 1e-160, -1e-160, 1e-20, -1e-20)
NEAR_ZERO = (2.0 ** -50, -2.0 ** -50)      # times 1 / sigma: the extreme is MU (1 +- 2^-50 / 0.3) to rounding, not MU
MIXED3 = ((-30.0, 0.5, 38.0), (-1000.0, -5.0, 5.0), (8.0, -8.0, 1e-300), (-2.0, -1.0, 3.0))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("mv") / "mv_point_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "mv_point_check.cpp"), "-o", str(path)])
    return str(path)


def _run(exe, pts, mode=None):
    """pts: (s, var_floor, mu, var, extremes) -> [(a, c_mu, c_v)] of the host program"""
    inp = "\n".join(" ".join([float.hex(float(s)), float.hex(vf), float.hex(mu), float.hex(var), str(len(e))]
                             + [float.hex(float(x)) for x in e]) for s, vf, mu, var, e in pts) + "\n"
    out = subprocess.run([exe] + ([mode] if mode else []), input=inp, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    t = [float.fromhex(x) for x in out.stdout.split()]
    assert len(t) == 3 * len(pts)
    return [t[3 * i:3 * i + 3] for i in range(len(pts))]


def _at(s, sigma, gammas):
    """the point whose extremes lie at about the given gamma (the reference takes the doubles as they are)"""
    return (s, FLOOR, MU, sigma * sigma, [MU + s * g * sigma for g in gammas])


def _grid():
    rng = np.random.default_rng(7)
    wide = list(np.linspace(-50.0, 40.0, 64))
    near = list(rng.uniform(-10.0, 10.0, size=64))
    pts = []
    for s in (1, -1):
        for sigma in SIGMAS:
            pts += [_at(s, sigma, [g]) for g in GAMMAS]
            pts += [_at(s, sigma, [g / sigma]) for g in NEAR_ZERO]
            pts += [_at(s, sigma, g3) for g3 in MIXED3]
            pts += [_at(s, sigma, wide), _at(s, sigma, near)]
        pts += [(s, FLOOR, 0.0, 1.0, [s * g]) for g in TINY_GAMMAS]
        pts += [(s, FLOOR, 0.0, 1.0, [s * g for g in (1e-300, -1e-300, -5e-324)])]
        # clamped: the variance below the floor, the criterion at (mu, var_floor)
        pts += [(s, 0.04, MU, 0.04 / 7, [MU + s * g * 0.2 for g in g3]) for g3 in MIXED3]
    return pts


def _ref(p):
    return R.point(p[2], p[3], p[4], maximise=p[0] == 1, var_floor=p[1])


def _worst(pts, got):
    worst = [0.0, 0.0, 0.0]
    for p, g in zip(pts, got):
        assert all(math.isfinite(x) for x in g), (p, g)
        worst = [max(w, r) for w, r in zip(worst, R.ratios(g, _ref(p)))]
    return worst


def test_the_grid_reaches_the_tiny_gammas_with_their_signs():
    """what the reference sees at the points meant for gamma = +-1e-300 and their like is not 0, and has the intended sign"""
    seen = set()
    for s in (1, -1):
        for g in TINY_GAMMAS:
            (got,) = _ref((s, FLOOR, 0.0, 1.0, [s * g]))[4]
            assert got == mp.mpf(g), (s, g, got)
            seen.add(float(got))
        for sigma in SIGMAS:
            for g in NEAR_ZERO:
                (got,) = _ref(_at(s, sigma, [g / sigma]))[4]
                assert got != 0 and (got > 0) == (g > 0) and abs(got) < mp.mpf(2) ** -48 / sigma, (s, sigma, g, got)
    assert {1e-300, -1e-300} <= seen
    in_grid = [float(g) for p in _grid() for g in _ref(p)[4] if len(p[4]) == 1]
    assert -1e-300 in in_grid and 1e-300 in in_grid


def test_point_function_against_mpmath(exe):
    """a and c_mu within C 2^-53 (1 + gamma_max^2) of themselves, c_v within that of mean_j |term_j| (max_value_ref.ratios);
    C per output is at most 10 x the worst ratio achieved here (profiles/max_value_margins.txt)."""
    pts = _grid()
    got = _run(exe, pts)
    worst = _worst(pts, got)
    print("mv.cpu: worst ratios a %.3g, c_mu %.3g, c_v %.3g (C = %s)" % (*worst, R.C))
    for name, w in zip(("a", "cmu", "cv"), worst):
        M._record("mv.cpu.%s" % name, w, R.C[name])
        assert w <= R.C[name], (name, w)
    # clamped points: c_v is exactly 0, and a / c_mu are those of the point (mu, var_floor)
    clamped = [(p, g) for p, g in zip(pts, got) if p[3] < p[1]]
    assert len(clamped) == 2 * len(MIXED3)
    for p, g in clamped:
        assert g[2] == 0.0
        assert g[:2] == _run(exe, [(p[0], p[1], p[2], p[1], p[4])])[0][:2]


def test_psi_is_positive_and_decreasing_and_the_coefficients_are_its_derivatives():
    """the reference itself: c_mu and c_v equal mpmath.diff of the value (relative 1e-25 at 60 digits)"""
    with mp.workdps(60):
        prev = None
        for g in (-40, -8, -1, 0, 1, 8, 30):
            v = R.psi(mp.mpf(g))
            assert v > 0 and (prev is None or v < prev)
            prev = v
        for maximise in (True, False):
            for ext in ([0.1], [0.9, -0.2, 0.35]):
                kw = dict(maximise=maximise, var_floor=1e-12)
                a, cmu, cv, _, _ = R.point(MU, 0.04, ext, **kw)
                dmu = mp.diff(lambda t: R.value(t, mp.mpf(0.04), ext, **kw), mp.mpf(MU))
                dv = mp.diff(lambda t: R.value(mp.mpf(MU), t, ext, **kw), mp.mpf(0.04))
                assert abs(cmu - dmu) <= mp.mpf(10) ** -25 * abs(dmu) and abs(cv - dv) <= mp.mpf(10) ** -25 * abs(dv)


@pytest.mark.parametrize("mode,pts,outputs", [
    ("naive", [_at(1, 1.0, [-30.0])], (0,)),                                        # gamma^2 / 2 = 450 cancels
    ("noclamp", [(1, 0.04, MU, 0.04 / 7, [MU + 0.2 * g for g in MIXED3[3]])], (2,)),  # c_v of the clamped point must be 0
    ("nomean", [_at(1, 1.0, MIXED3[3])], (0, 1, 2)),                                # S = 3 times too large
], ids=["naive", "noclamp", "nomean"])
def test_planted_defects_miss_the_bound(exe, mode, pts, outputs):
    good = _worst(pts, _run(exe, pts))
    bad = _worst(pts, _run(exe, pts, mode))
    names = ("a", "cmu", "cv")
    for i in outputs:
        assert good[i] <= R.C[names[i]] < bad[i], (mode, names[i], good[i], bad[i])


def test_symbol_is_declared_in_every_layer_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gprhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+double\s*\*\s*extremes\s*,\s*int\s+n_extremes,\s*int\s+"
                     r"maximise,\s*double\s+var_floor,\s*const\s+double\s*\*\s*test_inputs,\s*int64_t\s+ld,\s*int64_t\s+nt,\s*double"
                     r"\s*\*\s*values,\s*double\s*\*\s*dvalues,\s*int64_t\s+ldg,\s*double\s*\*\s*means,\s*double\s*\*\s*variances,\s*"
                     r"int\s+top_k,\s*int64_t\s*\*\s*top_index,\s*double\s*\*\s*top_values,\s*double\s*\*\s*top_dvalues,\s*int\s+"
                     r"on_device\s*\)" % NAME, header)
    assert re.search(r"#define\s+GPRHIP_MAX_EXTREMES\s+64\b", header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 18 and _lib.MAX_EXTREMES == 64
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    assert NAME + "(" in open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    assert NAME + "(" in open(os.path.join(ROOT, "bindings", "gpr_hip_stubs.c")).read()
    assert '"gprhip_ml_acquire_max_value"' in open(os.path.join(ROOT, "bindings", "gpr_hip.ml")).read()
    from gpr_amd import cov_se_fat, cov_se_iso, fitc_gp
    from gpr_amd.problem import Problem
    assert callable(Problem.acquire_max_value) and callable(Problem.max_value_search)
    for spec in (cov_se_iso, cov_se_fat):
        GP = fitc_gp.Make_deriv(spec)
        for variant in (GP.FITC, GP.Variational_FITC):
            assert callable(variant.Eval.Acquisition.calc_max_value)
    code = ("import sys, gpr_amd, importlib.util as u; assert 'torch' not in sys.modules; "
            "import gpr_amd.autograd as a; assert 'torch' not in sys.modules and callable(a.acquire_max_value)")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_cpp_mirror_method_builds(tmp_path):
    """tests/cpp/max_value_check.cpp -- Eval::Acquisition::calc_max_value of the C++ mirror -- compiles and links; without
    arguments it only prints its usage (no device call)."""
    exe = tmp_path / "max_value_check"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "max_value_check.cpp"), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr


def test_refusals_that_need_no_device():
    """Every argument refusal comes before anything touches a problem or a device: checked with a NULL problem (itself
    refused, last, once the rest is in order), and the leading dimensions with a problem that is only a handle's worth of
    Python -- the status, the function's name and the offending argument in gprhip_last_error()."""
    from gpr_amd import _lib
    from gpr_amd.problem import Problem
    lib = _lib.load()
    buf = np.zeros(8)
    idx = np.zeros(64, dtype=np.int64)
    vp = ctypes.c_void_p
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    ext = np.linspace(0.1, 0.9, 65)

    def call(extremes=ext, n=3, var_floor=1e-10, values=True, top_k=0, top_index=None):
        return lib.gprhip_acquire_max_value(None, dp(extremes) if extremes is not None else None, n, 1, var_floor,
                                            vp(buf.ctypes.data), 1, 1, vp(buf.ctypes.data) if values else None, None, 1, None,
                                            None, top_k, top_index, None, None, 0)

    def bad(j, v):
        e = ext.copy()
        e[j] = v
        return e

    cases = [
        (dict(n=0), b"n_extremes"), (dict(n=-1), b"n_extremes"), (dict(n=65), b"n_extremes"),
        (dict(extremes=None), b"extremes is NULL"),
        (dict(extremes=bad(2, float("nan"))), b"extremes must be finite"), (dict(extremes=bad(0, float("inf"))), b"extremes must be finite"),
        (dict(extremes=bad(63, -float("inf")), n=64), b"extremes must be finite"),
        (dict(var_floor=0.0), b"var_floor"), (dict(var_floor=-1.0), b"var_floor"), (dict(var_floor=float("inf")), b"var_floor"),
        (dict(var_floor=float("nan")), b"var_floor"),
        (dict(top_k=-1, top_index=ip), b"top_k"), (dict(top_k=65, top_index=ip), b"top_k"),
        (dict(top_k=3, top_index=None), b"top_index"),
        (dict(values=False), b"nothing is requested"),
        (dict(), b"invalid arguments"),                           # all in order but the problem
        (dict(extremes=bad(3, float("nan"))), b"invalid arguments"),  # (a non-finite entry beyond n_extremes is not read)
        (dict(n=64, top_k=64, top_index=ip), b"invalid arguments"),
    ]
    for kw, reason in cases:
        assert call(**kw) == _lib.EBADARG, kw
        msg = lib.gprhip_last_error()
        assert msg.startswith(NAME.encode() + b":") and reason in msg, (kw, msg)
    p = Problem.__new__(Problem)
    p._h = ctypes.c_void_p()  # (nothing to destroy)
    p.D = 2
    with pytest.raises(ValueError):
        Problem.acquire_max_value(p, np.zeros((2, 3)), [0.1], maximise=True, var_floor=1e-10, want=("values", "gradients"))
    with pytest.raises(ValueError):
        Problem.acquire_max_value(p, np.zeros((3, 3)), [0.1], maximise=True, var_floor=1e-10)   # bad ld: D is 2
    with pytest.raises(ValueError):
        Problem.acquire_max_value(p, np.zeros((2, 3)), [[0.1]], maximise=True, var_floor=1e-10)
    with pytest.raises(ValueError):
        Problem.acquire_max_value(p, np.zeros((2, 3)), [0.1], maximise=True)   # no model state seen: var_floor has no default


# ---- Problem.max_value_search on a stand-in problem ----------------------------------------------------------------------------
def mv_numpy(mu, var, extremes, maximise, var_floor):
    """the criterion restated in numpy / math as the header's table has it (moderate gamma only: nothing is guarded)"""
    s = 1.0 if maximise else -1.0
    clamped = var < var_floor
    v = max(var, var_floor)
    sigma = math.sqrt(v)
    g = s * (np.asarray(extremes, dtype=np.float64) - mu) / sigma
    Phi = np.array([0.5 * math.erfc(-x / math.sqrt(2.0)) for x in g])
    lam = np.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi) / Phi
    d = -0.5 * lam * (1.0 + g * (g + lam))
    return (float(np.mean(0.5 * g * lam - np.log(Phi))), float(np.mean(d) * (-s / sigma)),
            0.0 if clamped else float(np.mean(d * (-g / (2.0 * v)))))


@pytest.mark.parametrize("maximise", [True, False], ids=["max", "min"])
def test_numpy_restatement_against_finite_differences_and_the_reference(maximise):
    """da/dmu and da/dsigma2 of the restatement by central differences with h = 1e-5 of the argument: truncation
    h^2 |a'''| / 6 and rounding 2^-53 |a| / h are both below 1e-8 of a coefficient of order 1, the bound is 1e-7 relative;
    and the restatement agrees with the mpmath reference to 1e-12 at these moderate gamma."""
    ext = np.array([0.55, 0.7, 0.2, 0.9]) if maximise else np.array([0.05, -0.1, 0.4, -0.3])
    mu, var = MU, 0.04
    a, cmu, cv = mv_numpy(mu, var, ext, maximise, FLOOR)
    h = 1e-5
    fd_mu = (mv_numpy(mu + h * mu, var, ext, maximise, FLOOR)[0] - mv_numpy(mu - h * mu, var, ext, maximise, FLOOR)[0]) / (2 * h * mu)
    fd_v = (mv_numpy(mu, var * (1 + h), ext, maximise, FLOOR)[0] - mv_numpy(mu, var * (1 - h), ext, maximise, FLOOR)[0]) / (2 * h * var)
    assert abs(fd_mu - cmu) <= 1e-7 * abs(cmu) and abs(fd_v - cv) <= 1e-7 * abs(cv), (fd_mu, cmu, fd_v, cv)
    ref = R.point(mu, var, ext, maximise=maximise, var_floor=FLOOR)
    for got, want in zip((a, cmu, cv), ref[:3]):
        assert abs(got - float(want)) <= 1e-12 * abs(float(want))
    assert mv_numpy(mu, var / 4, ext, maximise, var)[2] == 0.0


class _StandIn:
    """records what Problem.max_value_search asks of the three calls it is made of"""

    def __init__(self, D, m, objective, top_index):
        self.D, self.m, self.objective, self.top_index, self.calls = D, m, objective, top_index, []

    def sample_paths(self, grid, z, **kw):
        self.calls.append(("sample_paths", kw))
        return dict(top_index=self.top_index)

    def sample_paths_refine(self, starts, z, draw_of, **kw):
        self.calls.append(("sample_paths_refine", dict(kw, starts=np.array(starts), draw_of=np.array(draw_of))))
        return dict(x=np.asfortranarray(starts + 0.5), values=self.objective[:starts.shape[1]])

    def acquire_max_value(self, grid, extremes, **kw):
        self.calls.append(("acquire_max_value", dict(kw, extremes=np.array(extremes))))
        return dict(values=np.array([mv_numpy(0.0, 1.0, extremes, kw["maximise"], 1e-12)[0]]))

    _extremes_of_refined = staticmethod(__import__("gpr_amd.problem", fromlist=["Problem"]).Problem._extremes_of_refined)


@pytest.mark.parametrize("maximise", [True, False], ids=["max", "min"])
def test_max_value_search_converts_the_objective_into_extremes(maximise):
    """sample_paths -> sample_paths_refine from its winners -> per draw the best refined objective o_j -> e_j = s o_j ->
    acquire_max_value, in this order; draw 1 has one qualifying grid point only (-1 in top_index), draw 2 a tie (the first)."""
    from gpr_amd.problem import Problem
    D, m, nt, nd = 2, 5, 9, 3
    grid = np.asfortranarray(np.arange(D * nt, dtype=np.float64).reshape(D, nt))
    top_index = np.asfortranarray(np.array([[4, 7, 2], [1, -1, 8]], dtype=np.int64))       # top_k x nd
    objective = np.array([0.25, 1.5, -0.75, 2.0, 2.0])     # starts: (draw 0: 4, 1) (draw 1: 7) (draw 2: 2, 8)
    q = _StandIn(D, m, objective, top_index)
    out = Problem.max_value_search(q, np.zeros((m, nd)), np.zeros(D), np.ones(D), grid, 2, dict(max_evals=7), maximise=maximise,
                                   var_floor=1e-12)
    assert [c[0] for c in q.calls] == ["sample_paths", "sample_paths_refine", "acquire_max_value"]
    sp, rf, mv = (c[1] for c in q.calls)
    assert sp["maximise"] == maximise and sp["top_k"] == 2 and sp["want_samples"] is False
    assert rf["maximise"] == maximise and rf["max_evals"] == 7
    assert np.array_equal(rf["draw_of"], [0, 0, 1, 2, 2]) and np.array_equal(rf["starts"], grid[:, [4, 1, 7, 2, 8]])
    s = 1.0 if maximise else -1.0
    assert np.array_equal(mv["extremes"], s * np.array([1.5, -0.75, 2.0])) and mv["maximise"] == maximise
    assert np.array_equal(out["extremes"], mv["extremes"])
    assert np.array_equal(out["extreme_x"], grid[:, [1, 7, 2]] + 0.5)
    assert np.array_equal(out["values"], [mv_numpy(0.0, 1.0, mv["extremes"], maximise, 1e-12)[0]])
