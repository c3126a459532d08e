"""The posterior calls AFTER gprhip_observe: the states (routes to a posterior), their shapes, and the checks that hold every
output to the 80-bit contraction of the state's OWN operands (debug_fetch "t", "uinv", "rinv", "rtil", "bvec" taken after the
route).  Shared by tests/test_gpu_observe_after.py (the device) and tests/test_observe_after_host.py (HostDevice below plays
the device in float64, honest or with one of FAULTS planted).

Routes:  A eval, observe(k)          B eval, every downstream call once, observe(k)      C eval, observe(64), observe(3)
         D eval, save, observe(k), every downstream call once, restore                   E A on a donor, its export loaded
         F A, then eval(reuse_v=True) at another sigma2
Shapes:  n = 300 rows, d = 3, m = 17 | 64 (small row path), 65 | 129 (mid, one and two 128-blocks), 300 (engine), m = 17 with
the one-kernel paths off, d = 16 at m = 17; three variants of tests/test_gpu_observe.py at m = 129 on route A.
New rows: those of tests/test_gpu_observe.split, every third moved to a quarter of a length scale from an inducing point
that the test points (tests/test_gpu_posterior.points_of: inducing point 3 i mod m at entry i = 1 mod 5) sit on.

Every bound is the one the call's own pin test uses: posterior_ref's running-error bounds (predict, covariances, training
means), sample_paths_pin_ref's (weights, paths), observe_ref's (R~'^-1, t), TOL_POST / TOL_GRAD of tests/test_gpu_predict_grad.py
against predict_grad_ref with (t, M) formed in 80 bits from the fetched factors, TOL_FACTOR of tests/test_gpu_factors.py for r_mat."""
import collections
import functools
import math

import numpy as np

from tests import observe_ref as O
from tests import posterior_ref as R
from tests import sample_paths_pin_ref as S
from tests.predict_grad_ref import predict_grad_from_state
from tests.test_gpu_factors import TOL_FACTOR
from tests.test_gpu_input_grad import _case
from tests.test_gpu_input_grads import Case, case_id, data, hypers_of
from tests.test_gpu_observe import N, SIGMA2, _variants, split
from tests.test_gpu_parity import TOL_GRAD, TOL_POST
from tests.test_gpu_posterior import points_of
from tests.util import _ld_matmul

LD = np.longdouble
NT = 65
NT_COV = (65, 129)
NS = 5
SIGMA2_F = 0.25            # route F's second evaluation
PGRAD_TOL = dict(means=TOL_POST, variances=TOL_POST, dmeans=TOL_GRAD, dvariances=TOL_GRAD)

State = collections.namedtuple("State", "route variant c k path")


def _iso(m, d=3, forced=False):
    return Case("iso", N + 64, m, d, forced=forced)


# (case, the row path its evaluation takes)
SHAPES = [(_iso(17), "small"), (_iso(64), "small"), (_iso(65), "mid"), (_iso(129), "mid"), (_iso(300), "engine"),
          (_iso(17, forced=True), "engine"), (_iso(17, 16), "small")]
VARIANTS = [(v, c) for v, c in _variants(129) if v in ("fat-proj-het", "loaded", "model-only")]
STATES = [State(r, "base", c, k, path) for r in "AB" for c, path in SHAPES for k in (1, 64)] + \
    [State("A", v, c, 3, "mid") for v, c in VARIANTS] + \
    [State(r, "base", c, 3, path) for r in "CDEF" for c, path in SHAPES]
REFIT_MS = (17, 129, 300)
K1_C = 64                  # route C: observe(64), then observe(k = 3)


def state_id(s):
    return "%s-%s-%s-k%d" % (s.route, s.variant, case_id(s.c), s.k) if isinstance(s, State) else str(s)


def kernel_of(c):
    return hypers_of(c, data(c)[3])


def oracle_kernel(c):
    return _case(c.kind, c.n, c.m, c.d, c.D, c.het, c.offset)[4]


def _lift(args):
    tp = args.get("tproj")
    return (lambda p: p) if tp is None else (lambda p: tp @ np.linalg.solve(tp.T @ tp, p))


@functools.lru_cache(maxsize=None)
def new_rows(c, k, skip=0):
    """(inputs D x k, targets k) of the rows [skip, skip + k) of the 64 new ones; row i = 0 mod 3 lies a quarter of a length
    scale from one of the 13 inducing points 3 j mod m, j = 1 mod 5, that the NT test points sit on"""
    X, y, Xn, yn, Z, args = split(c, 64)
    Xn = np.array(Xn, order="F")
    ell = math.exp(args.get("log_ell", 0.0))
    lift = _lift(args)
    rng = np.random.default_rng(4100 + c.m)
    for i in range(0, 64, 3):
        e = rng.normal(size=c.d)
        Xn[:, i] = lift(Z[:, (3 * (1 + 5 * ((i // 3) % (NT // 5)))) % c.m] + 0.25 * ell * e / np.linalg.norm(e))
    Xn, yn = np.asfortranarray(Xn[:, skip:skip + k]), yn[skip:skip + k].copy()
    Xn.setflags(write=False)
    yn.setflags(write=False)
    return Xn, yn


def rows_of(s):
    """the observe calls of a state's route, in order: [(inputs, targets)]"""
    if s.route == "C":
        return [new_rows(s.c, K1_C), new_rows(s.c, s.k, skip=61)]     # (row 63 of the second call sits by an inducing point)
    return [new_rows(s.c, s.k)]


def near_share(c, Xn):
    """share of the new rows within half a length scale of an inducing point that a test point of the NT mix sits on"""
    X, y, _, _, Z, args = split(c, 1)
    tp = args.get("tproj")
    P = Xn if tp is None else tp.T @ Xn
    seen = Z[:, [(3 * i) % c.m for i in range(1, NT, 5)]]
    dist = np.sqrt(((P[:, :, None] - seen[:, None, :]) ** 2).sum(0)).min(1)
    return float(np.mean(dist <= 0.5 * math.exp(args.get("log_ell", 0.0))))


@functools.lru_cache(maxsize=None)
def points_at(c, nt):
    X, y, _, _, Z, args = split(c, 1)
    return points_of(X, Z, args, nt)


@functools.lru_cache(maxsize=16)
def geometry(c, nt):
    """posterior_ref's 80-bit K, weights and K_tt at the test points"""
    Z = split(c, 1)[4]
    return R.geometry(points_at(c, nt)[0], Z, **kernel_of(c))


@functools.lru_cache(maxsize=8)
def shifted_geometry(c, nt):
    """sample_paths_pin_ref's geometry (the shifted coordinates of the expansion kernels) at the test points"""
    Z = split(c, 1)[4]
    return S.geometry(points_at(c, nt)[0], Z, **kernel_of(c))


@functools.lru_cache(maxsize=8)
def train_geometry(c):
    X, y, _, _, Z, args = split(c, 1)
    return R.geometry(X, Z, **kernel_of(c))


def draws(c):
    return np.asfortranarray(np.random.default_rng(5100 + c.m).normal(size=(c.m, NS)))


def live(c, nt=NT):
    """the test points within reach of the inducing points"""
    Xt, far = points_at(c, nt)
    return np.asfortranarray(Xt[:, ~far])


# ---- the checks: worst error / bound of every output of a device-like object -----------------------------------------------------
# A device-like object has: fetch() -> dict(t, uinv, rinv, rtil, bvec) (t and bvec absent without targets); predict(Xt, predictive) ->
# (means or None, variances); predict_input_grad(Xt) -> the four outputs (predictive); weights(Xt, z) -> the m x ns weights of a
# sample_paths call and its nt x ns samples; covariances(Xt, kind, predictive); factors() -> (chol_km, r_mat); train_means().
def grad_state(ops):
    """(t, M) of tests/predict_grad_ref.py in 80 bits from fetched operands: M = U^-1 (I - R~^-1 R~^-T) U^-T"""
    Ui, Ri = np.triu(np.asarray(ops["uinv"], LD)), np.triu(np.asarray(ops["rinv"], LD))
    m = Ui.shape[0]
    t = np.asarray(ops["t"], LD) if "t" in ops else np.zeros(m, LD)
    return t, _ld_matmul(_ld_matmul(Ui, np.eye(m, dtype=LD) - _ld_matmul(Ri, Ri.T)), Ui.T)


OUTPUTS_MODEL_ONLY = ("state.rinv", "predict.variance", "pgrad.variances", "pgrad.dvariances", "cov.FITC", "cov.FITC.predictive", "cov.FIC",
                      "cov.FIC.predictive", "r_mat")
OUTPUTS = OUTPUTS_MODEL_ONLY + ("state.t", "predict.mean", "pgrad.means", "pgrad.dmeans", "paths.weights", "paths.samples", "train_means")


def relinf(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))


def ratios(dev, c, ops, only=None):
    """{output: worst error / bound} of the calls of `dev` against the 80-bit contraction of `ops`, the operands fetched from
    the same state.  only: the outputs wanted (all of them by default)."""
    want = lambda name: only is None or name in only
    targets = "t" in ops
    Z = split(c, 1)[4]
    Xt, far = points_at(c, NT)
    out = {}
    if want("state.rinv"):
        Rl = np.asarray(ops["rtil"], LD)
        Xl = O.inv_upper(Rl)
        out["state.rinv"] = R.ratio(ops["rinv"], Xl, O.inverse_bound(Rl, Xl))[0]
    if want("state.t") and targets:
        tref = np.triu(np.asarray(ops["uinv"], LD)) @ (np.triu(np.asarray(ops["rinv"], LD)) @ np.asarray(ops["bvec"], LD))
        out["state.t"] = R.ratio(ops["t"], tref, O.coeff_bound(ops["rinv"], ops["uinv"], ops["bvec"]))[0]
    if want("predict.mean") or want("predict.variance"):
        g = geometry(c, NT)
        ch = R.chain(g, ops["uinv"], ops["rinv"])
        for predictive in (False, True):
            mu, var = dev.predict(Xt, predictive)
            ref, b = R.variance(g, ch, SIGMA2 if predictive else 0.0)
            out["predict.variance"] = max(out.get("predict.variance", 0.0), R.ratio(var, ref, b)[0])
            if targets:
                ref, b = R.mean(g, ops["t"])
                out["predict.mean"] = max(out.get("predict.mean", 0.0), R.ratio(mu, ref, b)[0])
    if any(want("pgrad." + nm) for nm in PGRAD_TOL):
        got = dev.predict_input_grad(Xt)
        ref = predict_grad_from_state(oracle_kernel(c), Z, grad_state(ops), Xt, SIGMA2, True)
        for nm in PGRAD_TOL if targets else ("variances", "dvariances"):
            out["pgrad." + nm] = relinf(got[nm], ref[nm]) / PGRAD_TOL[nm]
    if (want("paths.weights") or want("paths.samples")) and targets:
        z = draws(c)
        A, F = dev.weights(Xt, z)
        ref, b = S.weights(ops["t"], ops["uinv"], ops["rinv"], z)
        out["paths.weights"] = S.ratio(A, ref, b)[0]
        ref, b = S.paths(shifted_geometry(c, NT), A)
        out["paths.samples"] = S.ratio(F, ref, b)[0]
    for nt in NT_COV:
        if not any(want("cov.%s%s" % (kind, pr)) for kind in ("FITC", "FIC") for pr in ("", ".predictive")):
            break
        g = geometry(c, nt)
        ch = R.chain(g, ops["uinv"], ops["rinv"])
        for kind in ("FITC", "FIC"):
            for predictive in (False, True):
                name = "cov.%s%s" % (kind, ".predictive" if predictive else "")
                ref, b = R.covariances(g, ch, kind, SIGMA2 if predictive else 0.0)
                out[name] = max(out.get(name, 0.0), R.ratio(dev.covariances(points_at(c, nt)[0], kind, predictive), ref, b)[0])
    if want("r_mat"):
        U, Rm = dev.factors()
        ref = np.asarray(np.triu(np.asarray(ops["rtil"], LD)) @ np.triu(np.asarray(U, LD)), np.float64)
        out["r_mat"] = relinf(np.triu(Rm), ref) / TOL_FACTOR
    if want("train_means") and targets:
        ref, b = R.mean(train_geometry(c), ops["t"])
        out["train_means"] = R.ratio(dev.train_means(), ref, b)[0]
    return out


# ---- the device in float64 ----------------------------------------------------------------------------------------------------
FAULTS = ("m_from_old_rinv", "weights_from_old_rinv", "t_not_reformed", "r_mat_from_old_rtil", "restore_keeps_m")
# the outputs each fault can reach (the paths themselves are held against the weights the call formed: a stale weight shows in
# "paths.weights"; a t that was not re-formed is what the fetch returns, so it shows against b', not in the means)
REACH = {"m_from_old_rinv": ("pgrad.variances", "pgrad.dvariances"), "weights_from_old_rinv": ("paths.weights",),
         "t_not_reformed": ("state.t",), "r_mat_from_old_rtil": ("r_mat",), "restore_keeps_m": ("pgrad.variances", "pgrad.dvariances")}

f64 = lambda a: np.asarray(a, np.float64)


@functools.lru_cache(maxsize=None)
def host_pre_state(c):
    """the factors of the n = 300 rows in 80 bits, rounded to double as the device holds them"""
    X, y, _, _, Z, args = split(c, 1)
    pre = O.posterior_from_scratch(X, y, Z, np.asfortranarray(X[:, :1]), SIGMA2, log_het=args.get("log_hetero_skedasticity"),
                                   **kernel_of(c))
    st = dict(rtil=f64(pre["R"]), bvec=f64(pre["b"]), uinv=f64(pre["uinv"]), umat=f64(O.inv_upper(pre["uinv"])))
    st["rinv"] = f64(O.inv_upper(np.asarray(st["rtil"], LD)))
    st["t"] = np.triu(st["uinv"]) @ (np.triu(st["rinv"]) @ st["bvec"])
    return st


def host_observe(c, st, Xn, yn):
    """the update of tests/observe_ref.py in float64 and the vectors do_observe re-forms"""
    Z = split(c, 1)[4]
    rw = O.rows(Xn, Z, st["uinv"], SIGMA2, yn, **kernel_of(c))
    up = O.update_reflectors(st["rtil"], st["bvec"], f64(rw["W"]), f64(rw["eta"]), dtype=np.float64)
    new = dict(st, rtil=up["R"], bvec=up["b"])
    new["rinv"] = f64(O.inv_upper(np.asarray(up["R"], LD)))      # (rounded from 80 bits: within u of any double inverse's bound)
    new["t"] = np.triu(st["uinv"]) @ (np.triu(new["rinv"]) @ up["b"])
    return new


class HostDevice:
    """The calls of ratios() in plain float64 from a state's factors; `stale`: the state before the route's observations
    (or, for restore_keeps_m, the observed state a restore left behind), read where `fault` says so."""

    def __init__(self, c, st, fault=None, stale=None):
        self.c, self.st, self.fault, self.stale = c, st, fault, stale
        self.sf2 = math.exp(data(c)[3]["log_sf2"])

    def fetch(self):
        st = dict(self.st)
        if self.fault == "t_not_reformed":
            st["t"] = self.stale["t"]
        return {k: st[k] for k in ("t", "uinv", "rinv", "rtil", "bvec")}

    def _k(self, nt):
        return f64(geometry(self.c, nt)["K"])

    def _chain(self, K):
        V = K @ np.triu(self.st["uinv"])
        return V, V @ np.triu(self.st["rinv"])

    def predict(self, Xt, predictive):
        K = self._k(Xt.shape[1])
        V, Q = self._chain(K)
        return K @ self.fetch()["t"], (self.sf2 - ((V * V).sum(1) - (Q * Q).sum(1))) + (SIGMA2 if predictive else 0.0)

    def predict_input_grad(self, Xt):
        src = self.stale if self.fault in ("m_from_old_rinv", "restore_keeps_m") else self.st
        Ui, Ri = np.triu(self.st["uinv"]), np.triu(src["rinv"])
        Mm = Ui @ (np.eye(Ui.shape[0]) - Ri @ Ri.T) @ Ui.T
        ref = predict_grad_from_state(oracle_kernel(self.c), split(self.c, 1)[4], (f64(self.fetch()["t"]), Mm), Xt, SIGMA2, True)
        return ref       # (the formulas of the reference over double operands: what a correct device returns up to its sums' order)

    def weights(self, Xt, z):
        Ri = np.triu((self.stale if self.fault == "weights_from_old_rinv" else self.st)["rinv"])
        A = self.fetch()["t"][:, None] + np.triu(self.st["uinv"]) @ (Ri @ z)
        return A, self._k(Xt.shape[1]) @ A

    def covariances(self, Xt, kind, predictive):
        g = geometry(self.c, Xt.shape[1])
        K = f64(g["K"])
        V, Q = self._chain(K)
        add = (SIGMA2 if predictive else 0.0) * np.eye(K.shape[0])
        if kind == "FITC":
            return f64(g["Ktt"]) - V @ V.T + Q @ Q.T + add
        return Q @ Q.T + np.diag(self.sf2 - (K * K).sum(1)) + add

    def factors(self):
        src = self.stale if self.fault == "r_mat_from_old_rtil" else self.st
        return self.st["umat"], np.triu(src["rtil"]) @ np.triu(self.st["umat"])

    def train_means(self):
        return f64(train_geometry(self.c)["K"]) @ self.fetch()["t"]
