"""The cases of the gprhip_sample_paths_refine tests and an 80-bit evaluator of a draw on them, shared by the GPU tests
(tests/test_gpu_path_refine.py), the CPU checks (tests/test_path_refine_host.py) and tools/path_refine_precheck.py.

    model(key)            the well-conditioned cases of tests/test_gpu_input_grad.py (_case: cond(K_m + jitter) <= 1e5)
    draws(m, nd, seed)    z, m x nd standard normal
    draw_of(ns, nd, form) "c": the starts of one draw contiguous; "i": the draws interleaved -- the 16 rows of a wavefront hold
                          16 different draws where nd allows
    evaluator(key, z, s)  (x, j) -> (o, g): tests/sample_paths_ref.py's longdouble K a_j and its gradient, times s, rounded to
                          float64 once -- what tests/refine_ref.py runs over on the CPU
"""
import functools

import numpy as np

from tests import sample_paths_ref as SP
from tests.test_gpu_input_grad import _case

N = 200
SIGMA2 = 0.1
# (m, d, nd, ns, form): route 1 -- no projection.  m: one ragged panel (1, 5, 50), exactly one (64), one column past it (65),
# several panels at both panel widths (130, 200 at d <= 16: 64 columns; at d > 16: 32); d: every DT and the KS4 edges
ROUTE_1 = [(1, 1, 1, 1, "c"), (5, 3, 17, 17, "i"), (50, 3, 64, 130, "i"), (64, 16, 17, 65, "c"), (65, 3, 64, 64, "i"),
           (130, 17, 17, 16, "i"), (200, 64, 64, 17, "c"), (200, 1, 1, 130, "c"), (130, 16, 64, 65, "i"), (64, 64, 17, 64, "i"),
           (50, 17, 1, 16, "c"), (5, 1, 64, 130, "i")]
# (m, d, D, nd, ns, form): route 2 -- a D -> d projection
ROUTE_2 = [(20, 2, 5, 17, 1, "c"), (20, 2, 5, 17, 17, "i"), (20, 2, 5, 64, 130, "i"), (130, 3, 4, 17, 17, "c")]


def key_of(m, d, D=None):
    return ("proj", N, m, d, D) if D else ("iso", N, m, d)


@functools.lru_cache(maxsize=None)
def model(key):
    """(Xs, y, Zs, args, oracle kernel, cond)"""
    return _case(*key)


@functools.lru_cache(maxsize=None)
def state(key):
    Xs, y, Zs, args, ok, cond = model(key)
    return SP.path_state(ok, Zs, Xs, y, SIGMA2)


def draws(m, nd, seed=0):
    return np.asfortranarray(np.random.default_rng(9000 + 64 * m + nd + seed).standard_normal((m, nd)))


def draw_of(ns, nd, form):
    i = np.arange(ns)
    return ((i * nd) // ns if form == "c" else i % nd).astype(np.int32)


def box(key):
    """the bounding box of the training inputs"""
    Xs = model(key)[0]
    return Xs.min(1), Xs.max(1)


def starts(key, ns, seed):
    lo, hi = box(key)
    rng = np.random.default_rng(seed)
    return np.asfortranarray(lo[:, None] + (hi - lo)[:, None] * rng.uniform(-0.05, 1.05, size=(len(lo), ns)))


def paths_at(key, pts, zcol):
    """(f [nt], grad f (D x nt)) of the draw fixed by zcol at the columns of pts, from the 80-bit state"""
    Xs, y, Zs, args, ok, cond = model(key)
    nt = pts.shape[1]
    r = SP.sample_paths_from_state(ok, Zs, state(key), np.asfortranarray(pts), zcol, SIGMA2, grad_at=[(i, 0) for i in range(nt)])
    return r["paths"][:, 0], r["grads"]


def evaluator(key, z, s):
    def f(x, j):
        v, g = paths_at(key, np.asarray(x, dtype=np.float64).reshape(-1, 1), z[:, j])
        return s * float(v[0]), [s * float(t) for t in g[:, 0]]
    return f


def tie_band(a, ay, c1, g, delta):
    return 8 * 2.0 ** -53 * (abs(a) + abs(ay) + c1 * float(np.sum(np.abs(np.asarray(g) * np.asarray(delta)))))
