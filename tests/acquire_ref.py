"""Reference of the acquisition criteria of gprhip_acquire in mpmath at 50 digits: the value a and its partial derivatives
c_mu = da/dmu, c_v = da/dsigma2 from a predictive mean and variance, by the table of include/gprhip.h.

    s = +1 (maximise) or -1,  v = max(variance, var_floor),  sigma = sqrt(v),  delta = s (mu - best) - xi,  u = delta / sigma,
    h(u) = phi(u) + u Phi(u)

    EI      a = delta Phi(u) + sigma phi(u)    c_mu = s Phi(u)                 c_v = phi(u) / (2 sigma)
    LOG_EI  a = log sigma + log h(u)           c_mu = s Phi(u) / (sigma h(u))  c_v = phi(u) / (2 v h(u))
    PI      a = Phi(u)                         c_mu = s phi(u) / sigma         c_v = -u phi(u) / (2 v)
    BOUND   a = s mu + kappa sigma             c_mu = s                        c_v = kappa / (2 sigma)

and c_v = 0 where the variance was clamped (variance < var_floor).  tests/test_acquire_host.py checks the two derivative columns
against mpmath.diff of the value column."""
import mpmath as mp
import numpy as np

EI, LOG_EI, PI, BOUND = 0, 1, 2, 3
KINDS = (EI, LOG_EI, PI, BOUND)
KIND_NAMES = {EI: "ei", LOG_EI: "log_ei", PI: "pi", BOUND: "bound"}
DPS = 50


def _phi(u):
    return mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi)


def _Phi(u):
    return mp.erfc(-u / mp.sqrt(2)) / 2


def point(kind, mu, var, *, maximise, best=0.0, xi=0.0, kappa=0.0, var_floor=0.0):
    """(a, c_mu, c_v, u) as mpf at one point (mu, var: floats or mpf; var is the variance before the clamp)"""
    with mp.workdps(max(DPS, mp.mp.dps)):  # (at least 50 digits: mpmath.diff raises the precision around its calls)
        mu, var = mp.mpf(mu), mp.mpf(var)
        s = mp.mpf(1 if maximise else -1)
        clamped = var < mp.mpf(var_floor)
        v = max(var, mp.mpf(var_floor))
        sigma = mp.sqrt(v)
        delta = s * (mu - mp.mpf(best)) - mp.mpf(xi)
        u = delta / sigma
        if kind == BOUND:
            a, cmu, cv = s * mu + mp.mpf(kappa) * sigma, s, mp.mpf(kappa) / (2 * sigma)
        elif kind == PI:
            a, cmu, cv = _Phi(u), s * _phi(u) / sigma, -u * _phi(u) / (2 * v)
        elif kind in (EI, LOG_EI):
            Phi, phi = _Phi(u), _phi(u)
            h = phi + u * Phi
            if kind == EI:
                a, cmu, cv = delta * Phi + sigma * phi, s * Phi, phi / (2 * sigma)
            else:
                a, cmu, cv = mp.log(sigma) + mp.log(h), s * Phi / (sigma * h), phi / (2 * v * h)
        else:
            raise ValueError("unknown kind %r" % (kind,))
        return a, cmu, (mp.mpf(0) if clamped else cv), u


def value(kind, mu, var, **kw):
    return point(kind, mu, var, **kw)[0]


def evaluate(kind, means, variances, **kw):
    """The criterion at every (means[r], variances[r]): lists of mpf (a, c_mu, c_v, u) -- mpf, because EI and PI lie below the
    float64 range in the deep tail"""
    rows = [point(kind, float(m), float(v), **kw)
            for m, v in zip(np.asarray(means, dtype=np.float64), np.asarray(variances, dtype=np.float64))]
    return tuple([r[i] for r in rows] for i in range(4))
