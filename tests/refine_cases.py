"""The models of the gprhip_acquire_refine tests and an 80-bit evaluator of a criterion on them, shared by the GPU tests
(tests/test_gpu_refine.py), the CPU check of the chosen seeds (tests/test_refine_host.py) and tools/refine_precheck.py.

    data(m, d, D, seed)  n = 200 points in [0, 1]^D of a smooth ridge (the trace tests: any criterion, any shape)
    bump(d)              n = 200 points in [0, 1]^d of one Gaussian bump with its top inside the box, m = 20 (check 5)
    evaluator(...)       x -> (a, g): tests/predict_grad_ref.py's longdouble posterior through tests/acquire_ref.py's mpmath
                         criterion, rounded to float64 once -- what tests/refine_ref.py runs over on the CPU
"""
import math

import numpy as np

from oracle import fitc_oracle as O
from tests import acquire_ref as R
from tests import predict_grad_ref as PG

N = 200
SIGMA2 = 1e-2
KIND_OF = {"ei": R.EI, "log_ei": R.LOG_EI, "pi": R.PI, "bound": R.BOUND}


def data(m, d, D=None, seed=0):
    """(X, y, Z, args): args are the keywords of Problem.eval beside sigma2 and inducing; with D a D -> d projection"""
    rng = np.random.default_rng(100 * m + d + seed)
    Dd = D or d
    X = np.asfortranarray(rng.uniform(0.0, 1.0, size=(Dd, N)))
    y = np.sin(3.0 * X.sum(0) / math.sqrt(Dd)) + 0.05 * rng.normal(size=N)
    if D:
        tproj = np.asfortranarray(rng.normal(size=(D, d)) / math.sqrt(D))
        Z = np.asfortranarray((tproj.T @ X)[:, rng.permutation(N)[:m]] + 0.01 * rng.normal(size=(d, m)))
        return X, y, Z, dict(log_sf2=0.0, tproj=tproj)
    Z = np.asfortranarray(X[:, rng.permutation(N)[:m]] + 0.01 * rng.normal(size=(d, m)))
    return X, y, Z, dict(log_sf2=0.0, log_ell=math.log(0.3 * math.sqrt(d)))


BUMP_TOP = (0.37, 0.62)
BUMP_M = 20


def bump(d):
    """(X, y, Z, args) of exp(-|x - top|^2 / 0.08) + noise: the posterior mean, and the bound mu + sigma with it, has its
    maximiser near `top`, inside [0, 1]^d and on no point of a 33- or 9-per-axis grid"""
    rng = np.random.default_rng(40 + d)
    X = np.asfortranarray(rng.uniform(0.0, 1.0, size=(d, N)))
    y = np.exp(-((X - np.array(BUMP_TOP[:d])[:, None]) ** 2).sum(0) / 0.08) + 0.02 * rng.normal(size=N)
    Z = np.asfortranarray(X[:, rng.permutation(N)[:BUMP_M]] + 0.01 * rng.normal(size=(d, BUMP_M)))
    return X, y, Z, dict(log_sf2=0.0, log_ell=math.log(0.25))


def oracle_kernel(args):
    assert "tproj" not in args, "the CPU evaluator covers Cov_se_iso"
    return O.SeIsoKernel(args["log_ell"], args["log_sf2"])


def posterior(X, y, Z, args):
    """pts (D x nt) -> the longdouble posterior and its input gradients (tests/predict_grad_ref.py), in float64"""
    k = oracle_kernel(args)
    state = PG.model_state(k, Z, X, y, SIGMA2)
    return lambda pts: PG.predict_grad_from_state(k, Z, state, np.asfortranarray(pts), SIGMA2, predictive=False)


def evaluator(post, kind, **kw):
    """x -> (a, g) of the criterion `kind` (a name) with the keywords of acquire_ref.point"""
    def f(x):
        q = post(np.asarray(x, dtype=np.float64).reshape(-1, 1))
        a, cmu, cv, _ = R.point(KIND_OF[kind], float(q["means"][0]), float(q["variances"][0]), **kw)
        g = [float(cmu * float(q["dmeans"][j, 0]) + cv * float(q["dvariances"][j, 0])) for j in range(q["dmeans"].shape[0])]
        return float(a), g
    return f


def grid(d, per_axis):
    axes = [np.linspace(0.0, 1.0, per_axis)] * d
    return np.asfortranarray(np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")]))


COARSE = {1: 33, 2: 9}   # points per axis of check 5's coarse grid; the fine one is 64 x finer
BOUND_KAPPA = 1.0        # check 5 refines the bound mu + kappa sigma


def bound_values(q, kappa=BOUND_KAPPA, var_floor=1e-10):
    """the bound (maximise) over a whole grid in float64: for picking grid points, not for a tolerance"""
    return q["means"] + kappa * np.sqrt(np.maximum(q["variances"], var_floor))
