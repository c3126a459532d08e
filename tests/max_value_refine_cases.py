"""The cases of the gprhip_acquire_max_value_refine tests, shared by the GPU tests (tests/test_gpu_max_value_refine.py), the
CPU checks (tests/test_max_value_refine_host.py) and tools/max_value_refine_precheck.py: the models and boxes of
tests/refine_cases.py, the rule that fixes the extremes, and an 80-bit / mpmath evaluator of the criterion.

    extremes(means, variances, S, maximise)   the extremes of a case from a posterior over its box
    evaluator(post, ext, maximise, var_floor) x -> (a, g): RC.posterior's longdouble posterior through tests/max_value_ref.py's
                                              mpmath criterion, rounded to float64 once -- what tests/refine_ref.py runs over
    values_f64(...)                           the criterion over a whole grid in float64: for picking grid points only

The extremes rule.  With mu the posterior means over a point set of the box, `top` the largest of them and sigma_top the
standard deviation at that point, maximising: S = 1 gives top + sigma_top; S > 1 a ladder of S equal steps from
top + sigma_top / 4 to top + sigma_top.  Minimising mirrors it below the smallest mean.  These are values that maxima of
drawn paths take -- a little above the best mean, by the uncertainty there.  (The rule first tried, top + sigma_max and a
ladder to top + 4 sigma_max with sigma_max the largest standard deviation over the box, puts the maximiser of the criterion of
the two-dimensional bump model into the corner (1, 1) of the box, where no data lie and the variance is largest: nothing is
left to refine.  With sigma_top the maximiser sits near the bump's top, inside the box and off the coarse grid, in both
dimensions: tests/test_max_value_refine_host.py.)  The numbers are rounded to a multiple of 2^-20, so that the CPU posterior
(here, the precheck) and the device's own (the GPU tests, which also cover the projection case that the CPU
evaluator does not) give the same doubles."""
import math

import numpy as np

from tests import max_value_ref as R
from tests import refine_cases as RC

VAR_FLOOR = 1e-10     # log_sf2 = 0 in every model of tests/refine_cases.py: the default 1e-10 sf2
BOX_POINTS = 256      # the point set of a box in more than 2 dimensions


def box(D):
    """the box of the trace cases (that of tests/test_gpu_refine.py's _run_shape)"""
    return np.full(D, 0.05), np.linspace(0.9, 1.1, D)


def box_points(lo, hi):
    """the points a case's extremes are fixed from: a 33- / 9-per-axis grid in 1 / 2 dimensions, else seeded uniform points"""
    D = len(lo)
    if D <= 2:
        unit = RC.grid(D, RC.COARSE[D])
    else:
        unit = np.random.default_rng(1000 + D).uniform(size=(D, BOX_POINTS))
    return np.asfortranarray(lo[:, None] + (hi - lo)[:, None] * unit)


def extremes(means, variances, S, maximise):
    mu = np.asarray(means, dtype=np.float64)
    s = 1.0 if maximise else -1.0
    i = int(np.argmax(s * mu))
    top, stop = float(mu[i]), math.sqrt(float(np.asarray(variances)[i]))
    e = np.array([top + s * stop]) if S == 1 else top + s * stop * np.linspace(0.25, 1.0, S)
    return np.round(e * 1048576.0) / 1048576.0


def evaluator(post, ext, maximise, var_floor=VAR_FLOOR):
    """x -> (a, g) of max-value entropy search over `ext` on the posterior `post` (RC.posterior)"""
    ext = [float(e) for e in ext]

    def f(x):
        q = post(np.asarray(x, dtype=np.float64).reshape(-1, 1))
        a, cmu, cv, _, _ = R.point(float(q["means"][0]), float(q["variances"][0]), ext, maximise=maximise, var_floor=var_floor)
        g = [float(cmu * float(q["dmeans"][j, 0]) + cv * float(q["dvariances"][j, 0])) for j in range(q["dmeans"].shape[0])]
        return float(a), g
    return f


_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def values_f64(means, variances, ext, maximise, var_floor=VAR_FLOOR):
    """the criterion over a grid in float64 (moderate gamma): for picking grid points, not for a tolerance"""
    s = 1.0 if maximise else -1.0
    sigma = np.sqrt(np.maximum(np.asarray(variances, dtype=np.float64), var_floor))
    g = s * (np.asarray(ext, dtype=np.float64)[:, None] - np.asarray(means, dtype=np.float64)[None, :]) / sigma[None, :]
    Phi = 0.5 * _erfc(-g / math.sqrt(2.0))
    lam = np.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi) / Phi
    return np.mean(0.5 * g * lam - np.log(Phi), axis=0)
