"""The step rule of gprhip_acquire_refine (gpr_amd/csrc/refine_step.h) in Python over any evaluator: projected gradient
ascent with Armijo backtracking on one start inside a box, operation for operation the header's arithmetic in float64 --
tests/test_refine_host.py holds the two together step for step (tests/cpp/refine_step_check.cpp prints the header's trace).

    evaluate(x) -> (a, g): the objective ("larger is better") and its gradient at x (length D)

Per start, with w = upper - lower: x = clip(start), dir_k = scale_k g_k (0 where the bound is active and dir_k points out of
the box, or g_k is NaN), alpha = (step0 min w) / max |dir|; a trial y = clip(x + alpha dir) (y_k = x_k where dir_k = 0) is
accepted when a_y >= a + c1 sum g_k (y_k - x_k) -- then alpha *= grow, else alpha *= shrink; the start ends CONVERGED on a zero
dir or a trial step of at most xtol w, MAX_EVALS when the evaluations run out, NAN on a NaN value at the start."""
import numpy as np

CONVERGED, MAX_EVALS, NAN = 0, 1, 2
STATUS_NAMES = {CONVERGED: "converged", MAX_EVALS: "max_evals", NAN: "nan"}
DEFAULTS = dict(max_evals=50, step0=0.1, c1=1e-4, shrink=0.5, grow=2.0, xtol=1e-8)


def clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def direction(g, scale, x, lo, hi):
    dk = scale * g
    if dk != dk:
        return 0.0
    if x <= lo and dk < 0.0:
        return 0.0
    if x >= hi and dk > 0.0:
        return 0.0
    return dk


def trial(x, alpha, dk, lo, hi):
    return x if dk == 0.0 else clip(x + alpha * dk, lo, hi)


def armijo(a, ay, c1, gd):
    return bool(ay >= a + c1 * gd)


def refine(evaluate, start, lower, upper, scale=None, *, max_evals, step0, c1, shrink, grow, xtol):
    """One start.  Returns a dict: x, a, g (the last accepted evaluation), evals, accepted, status, and trace -- a list of
    records (y, g_y, a_y, alpha, accepted), one per evaluation."""
    D = len(start)
    lo, hi = [float(v) for v in lower], [float(v) for v in upper]
    sc = [1.0] * D if scale is None else [float(v) for v in scale]
    w = [hi[k] - lo[k] for k in range(D)]

    def dirs(x, g):
        return [direction(g[k], sc[k], x[k], lo[k], hi[k]) for k in range(D)]

    def dmax_of(d):
        m = 0.0
        for v in d:
            m = abs(v) if abs(v) > m else m
        return m

    x = [clip(float(start[k]), lo[k], hi[k]) for k in range(D)]
    a, g = evaluate(np.array(x))
    a, g = float(a), [float(v) for v in g]
    out = dict(evals=1, accepted=0, trace=[(list(x), list(g), a, 0.0, True)])

    def done(status):
        out.update(x=np.array(x), a=a, g=np.array(g), status=status)
        return out

    if a != a:
        return done(NAN)
    d = dirs(x, g)
    if dmax_of(d) == 0.0:
        return done(CONVERGED)
    wmin = w[0]
    for k in range(1, D):
        wmin = w[k] if w[k] < wmin else wmin
    alpha = (step0 * wmin) / dmax_of(d)
    while out["evals"] < max_evals:
        y = [trial(x[k], alpha, d[k], lo[k], hi[k]) for k in range(D)]
        rel = 0.0
        for k in range(D):
            r = abs(y[k] - x[k]) / w[k]
            rel = r if r > rel else rel
        if rel <= xtol:
            return done(CONVERGED)
        ay, gy = evaluate(np.array(y))
        ay, gy = float(ay), [float(v) for v in gy]
        out["evals"] += 1
        gd = 0.0
        for k in range(D):
            gd += g[k] * (y[k] - x[k])
        acc = armijo(a, ay, c1, gd)
        out["trace"].append((list(y), list(gy), ay, alpha, acc))
        if acc:
            x, a, g = y, ay, gy
            out["accepted"] += 1
            d = dirs(x, g)
            if dmax_of(d) == 0.0:
                return done(CONVERGED)
            alpha *= grow
        else:
            alpha *= shrink
    return done(MAX_EVALS)
