"""Reference of max-value entropy search (gprhip_acquire_max_value) in mpmath at 50 digits: the value a and its partial
derivatives c_mu = da/dmu, c_v = da/dsigma2 from a predictive mean and variance and the extremes e_j of S drawn paths, by the
table of include/gprhip.h.

    s = +1 (maximise) or -1,  v = max(variance, var_floor),  sigma = sqrt(v),  gamma_j = s (e_j - mu) / sigma,
    lambda = phi / Phi,  psi = gamma lambda / 2 - log Phi,  psi' = -(lambda / 2) (1 + gamma (gamma + lambda))
    a = mean_j psi(gamma_j),  c_mu = mean_j psi'(gamma_j) (-s / sigma),  c_v = mean_j psi'(gamma_j) (-gamma_j / (2 v))

and c_v = 0 where the variance was clamped.  `ratios` holds a result to the three error bounds: a and c_mu (sums of terms of one sign) to c 2^-53 (1 + gamma_max^2) of themselves, c_v (terms of both signs) to
c 2^-53 (1 + gamma_max^2) mean_j |term_j|; a result in the subnormal range is allowed the spacing of the subnormals on top
(FLOOR_ULPS 2^-1074: no double is closer)."""
import mpmath as mp
import numpy as np

DPS = 50
EPS = 2.0 ** -53
TINY = 2.0 ** -1074
FLOOR_ULPS = 2


def _phi(u):
    return mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi)


def _Phi(u):
    return mp.erfc(-u / mp.sqrt(2)) / 2


def _log_Phi(u):
    # (above 0 through the upper tail: 1 - 1e-60 is 1 at 50 digits)
    return mp.log1p(-mp.erfc(u / mp.sqrt(2)) / 2) if u > 0 else mp.log(_Phi(u))


def psi(gamma):
    lam = _phi(gamma) / _Phi(gamma)
    return gamma * lam / 2 - _log_Phi(gamma)


def dpsi(gamma):
    lam = _phi(gamma) / _Phi(gamma)
    return -(lam / 2) * (1 + gamma * (gamma + lam))


def point(mu, var, extremes, *, maximise, var_floor):
    """(a, c_mu, c_v, cv_abs, gammas) as mpf at one point (var: the variance before the clamp); cv_abs = mean_j |term_j| of
    c_v's sum (of the unclamped sum where the variance was clamped)"""
    with mp.workdps(max(DPS, mp.mp.dps)):
        mu, var = mp.mpf(mu), mp.mpf(var)
        s = mp.mpf(1 if maximise else -1)
        clamped = var < mp.mpf(var_floor)
        v = max(var, mp.mpf(var_floor))
        sigma = mp.sqrt(v)
        gammas = [s * (mp.mpf(e) - mu) / sigma for e in extremes]
        n = len(gammas)
        d = [dpsi(g) for g in gammas]
        a = mp.fsum(psi(g) for g in gammas) / n
        cmu = mp.fsum(d) / n * (-s / sigma)
        terms = [dj * (-g / (2 * v)) for dj, g in zip(d, gammas)]
        cv_abs = mp.fsum(abs(t) for t in terms) / n
        return a, cmu, (mp.mpf(0) if clamped else mp.fsum(terms) / n), cv_abs, gammas


def value(mu, var, extremes, **kw):
    return point(mu, var, extremes, **kw)[0]


def evaluate(means, variances, extremes, **kw):
    """the criterion at every (means[r], variances[r]): a list of `point` tuples"""
    return [point(float(m), float(v), extremes, **kw)
            for m, v in zip(np.asarray(means, dtype=np.float64), np.asarray(variances, dtype=np.float64))]


def unit(ref):
    """2^-53 (1 + gamma_max^2) of a reference point"""
    return mp.mpf(EPS) * (1 + max(abs(g) for g in ref[4]) ** 2)


def ratios(got, ref):
    """the constant c that (a, c_mu, c_v) of `got` (floats) need against `ref`, per output; the subnormal floor taken off"""
    u = unit(ref)
    out = []
    for x, r, scale in ((got[0], ref[0], abs(ref[0])), (got[1], ref[1], abs(ref[1])), (got[2], ref[2], ref[3])):
        err = abs(mp.mpf(float(x)) - r) - FLOOR_ULPS * mp.mpf(TINY)
        if err <= 0:
            out.append(0.0)
        elif scale == 0:
            out.append(float("inf"))
        else:
            out.append(float(err / (u * scale)))
    return out


# the constant c per output: at most 10 x the worst ratio achieved on the CPU grid of tests/test_max_value_host.py
# (profiles/max_value_margins.txt: 2.6, 111, 111 -- psi' loses two factors of about gamma^2 where acq_mills still forms
# g = 1 - x R as it stands, just below x = 5, against the one factor 1 + gamma^2 that the bound grants); the device is held to
# the same constants
C = {"a": 20.0, "cmu": 1000.0, "cv": 1000.0}
