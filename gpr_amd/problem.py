"""Device-resident FITC problem: thin object wrapper over the gprhip C ABI.

Holds the training inputs/targets of one shard in HBM and runs evaluations of the FITC log
evidence + gradient for changing hyper-parameters (what the reference's optimiser callback
multim_dcommon does per call, lib/fitc_gp.ml:1612-1636).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import COV_SE_FAT, COV_SE_ISO, F32_BULK, F64, Hypers, Result, TargetsResult

CHOLESKY_JITTER = 1e-6  # Utils.cholesky_jitter, lib/utils.ml:35


@dataclass
class Evaluation:
    l1: float                 # Model.calc_log_evidence
    l2: float
    l: float                  # Trained.calc_log_evidence
    dl_dsigma2: Optional[float]
    grad: Optional[np.ndarray]    # reference Hyper.get_all order
    coeffs: np.ndarray        # Trained.calc_mean_coeffs


@dataclass
class TargetsEvaluation:
    """One evaluation of k target vectors on one model (Problem.eval_targets)."""
    l1: float                 # Model.calc_log_evidence (the same for every target)
    l2: np.ndarray            # [k]
    l: np.ndarray             # [k] Trained.calc_log_evidence per target
    l_sum: float              # sum of l
    dl_dsigma2_sum: Optional[float]
    grad_sum: Optional[np.ndarray]  # gradient of l_sum, reference Hyper.get_all order
    coeffs: np.ndarray        # m x k, column j = Trained.calc_mean_coeffs of target j


def _f64_ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Problem:
    def __init__(self, cov_kind, n, D, d, m, device=0, chunk_rows=0, precision=F64):
        """precision: F64 (reference parity) or F32_BULK (n x m contractions in fp32, m x m work in fp64)."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.cov_kind, self.n, self.D, self.d, self.m = cov_kind, int(n), int(D), int(d), int(m)
        self.device, self.precision = device, precision
        _lib.check(self._lib.gprhip_problem_create_ex(device, cov_kind, int(precision), self.n, self.D, self.d,
                                                      self.m, int(chunk_rows), C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gprhip_problem_destroy(self._h)
            self._h = C.c_void_p()

    def is_open(self):
        return bool(self._h)

    def _handle(self):
        if not self._h:
            raise _lib.GprHipError(_lib.ESTATE, "gpr_amd.Problem: the problem has been closed")
        return self._h

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data
    def set_inputs(self, inputs):
        """inputs: D x n (reference layout, one point per column); numpy, any order."""
        x = np.asfortranarray(inputs, dtype=np.float64)
        if x.shape != (self.D, self.n):
            raise ValueError("set_inputs: expected shape (%d, %d), got %s" % (self.D, self.n, x.shape))
        _lib.check(self._lib.gprhip_set_inputs(self._handle(), _f64_ptr(x), self.D))

    def set_targets(self, targets):
        y = np.ascontiguousarray(targets, dtype=np.float64)
        if y.shape != (self.n,):
            # Trained.calc: Vec.dim targets <> n  (lib/fitc_gp.ml:283-284)
            raise ValueError("Trained.calc: Vec.dim targets (%d) <> n (%d)" % (y.shape[0], self.n))
        _lib.check(self._lib.gprhip_set_targets(self._handle(), _f64_ptr(y)))

    def set_targets_many(self, targets):
        """targets: n x k (one target vector per column), 1 <= k <= 16; replaces any earlier target matrix.  The target
        vector of `set_targets` is kept beside it."""
        y = np.asfortranarray(targets, dtype=np.float64)
        if y.ndim != 2 or y.shape[0] != self.n:
            raise ValueError("Trained.calc_many: expected targets of shape (%d, k), got %s" % (self.n, y.shape))
        _lib.check(self._lib.gprhip_set_targets_many(self._handle(), _f64_ptr(y), self.n, int(y.shape[1])))
        self._k = int(y.shape[1])

    def set_inputs_device(self, ptr):
        """ptr: device address of a contiguous point-major [n][D] fp64 array (e.g. tensor.data_ptr())."""
        _lib.check(self._lib.gprhip_set_inputs_device(self._handle(), C.c_void_p(ptr)))

    def set_targets_device(self, ptr):
        _lib.check(self._lib.gprhip_set_targets_device(self._handle(), C.c_void_p(ptr)))

    # ---- evaluation
    def n_hypers(self, has_tproj=False, has_hetero=False, has_multiscale=False):
        flags = int(has_tproj) | (int(has_hetero) << 1) | (int(has_multiscale) << 2)
        return int(self._lib.gprhip_n_hypers(self._handle(), flags))

    def _hypers(self, log_ell, log_sf2, sigma2, inducing, tproj, variational, model_only, jitter,
                log_hetero_skedasticity=None, log_multiscales_m05=None, reuse_v=False):
        z = np.asfortranarray(inducing, dtype=np.float64)
        if z.shape != (self.d, self.m):
            raise ValueError("inducing: expected shape (%d, %d), got %s" % (self.d, self.m, z.shape))
        h = Hypers()
        h.log_ell, h.log_sf2, h.sigma2 = float(log_ell), float(log_sf2), float(sigma2)
        h.inducing = _f64_ptr(z)
        keep = [z]
        if tproj is not None:
            tp = np.asfortranarray(tproj, dtype=np.float64)
            if tp.shape != (self.D, self.d):
                raise ValueError("tproj: expected shape (%d, %d), got %s" % (self.D, self.d, tp.shape))
            h.tproj = _f64_ptr(tp)
            keep.append(tp)
        h.variational, h.model_only, h.jitter = int(variational), int(model_only), float(jitter)
        h.reuse_v = int(reuse_v)
        if log_hetero_skedasticity is not None:
            lh = np.ascontiguousarray(log_hetero_skedasticity, dtype=np.float64)
            if lh.shape != (self.m,):
                raise ValueError("log_hetero_skedasticity: expected %d entries" % self.m)
            h.log_hetero_skedasticity = _f64_ptr(lh)
            keep.append(lh)
        if log_multiscales_m05 is not None:
            lm = np.asfortranarray(log_multiscales_m05, dtype=np.float64)
            if lm.shape != (self.d, self.m):
                raise ValueError("log_multiscales_m05: expected shape (%d, %d)" % (self.d, self.m))
            h.log_multiscales_m05 = _f64_ptr(lm)
            keep.append(lm)
        return h, keep

    def eval(self, *, log_sf2, sigma2, inducing, log_ell=0.0, tproj=None, variational=False,
             model_only=False, want_grad=True, jitter=CHOLESKY_JITTER, log_hetero_skedasticity=None,
             log_multiscales_m05=None, reuse_v=False):
        """reuse_v=True: only sigma2/targets changed since the previous eval on this problem
        (Model.update_sigma2, lib/fitc_gp.ml:234-236): K_nm, V and r are reused."""
        self._log_sf2 = float(log_sf2)  # (Problem.acquire's default var_floor)
        h, keep = self._hypers(log_ell, log_sf2, sigma2, inducing, tproj, variational, model_only, jitter,
                               log_hetero_skedasticity, log_multiscales_m05, reuse_v)
        res = Result()
        nh = self.n_hypers(tproj is not None, log_hetero_skedasticity is not None, log_multiscales_m05 is not None)
        grad = np.empty(nh if want_grad else 1, dtype=np.float64)
        coeffs = np.empty(self.m, dtype=np.float64)
        _lib.check(self._lib.gprhip_eval(self._handle(), C.byref(h), int(want_grad), C.byref(res),
                                         _f64_ptr(grad), _f64_ptr(coeffs)))
        del keep
        return Evaluation(res.l1, res.l2, res.l, res.dl_dsigma2 if want_grad else None,
                          grad[:res.n_hypers] if want_grad else None, coeffs)

    def eval_input_grad(self, *, log_sf2, sigma2, inducing, log_ell=0.0, tproj=None, variational=False,
                        model_only=False, jitter=CHOLESKY_JITTER, log_hetero_skedasticity=None,
                        log_multiscales_m05=None, reuse_v=False, out_device_ptr=None, ld=None):
        """A gradient evaluation (keyword arguments as `eval`) that also returns dl/d(training inputs): (Evaluation,
        D x n array in the layout of `set_inputs`).  out_device_ptr: device address of a contiguous point-major [n][D] fp64
        array (the layout of `set_inputs_device`, e.g. tensor.data_ptr()) that receives it instead -- the second value is
        then None.  ld (host output only): leading dimension >= D of the returned array's buffer; rows D.. of it are not
        written (they hold NaN).  fp64 problems, no multiscales (the library refuses otherwise)."""
        self._log_sf2 = float(log_sf2)  # (Problem.acquire's default var_floor)
        h, keep = self._hypers(log_ell, log_sf2, sigma2, inducing, tproj, variational, model_only, jitter,
                               log_hetero_skedasticity, log_multiscales_m05, reuse_v)
        res = Result()
        nh = self.n_hypers(tproj is not None, log_hetero_skedasticity is not None, log_multiscales_m05 is not None)
        grad = np.empty(nh, dtype=np.float64)
        coeffs = np.empty(self.m, dtype=np.float64)
        if out_device_ptr is not None:
            out, ptr, ldv, dev = None, C.c_void_p(int(out_device_ptr)), self.D, 1
        else:
            ldv = self.D if ld is None else int(ld)
            out = np.full((max(ldv, 1), self.n), np.nan, dtype=np.float64, order="F")
            ptr, dev = C.c_void_p(out.ctypes.data), 0
        _lib.check(self._lib.gprhip_eval_input_grad(self._handle(), C.byref(h), C.byref(res), _f64_ptr(grad), _f64_ptr(coeffs),
                                                    ptr, ldv, dev))
        del keep
        ev = Evaluation(res.l1, res.l2, res.l, res.dl_dsigma2, grad[:res.n_hypers], coeffs)
        if out is None:
            return ev, None
        return ev, (out if ld is not None else out[:self.D])

    def eval_targets(self, *, log_sf2, sigma2, inducing, log_ell=0.0, tproj=None, variational=False,
                     model_only=False, want_grad=True, jitter=CHOLESKY_JITTER, log_hetero_skedasticity=None,
                     log_multiscales_m05=None, reuse_v=False):
        """All target vectors of `set_targets_many` against one model in one evaluation: per-target evidence and mean
        coefficients, the gradient of the summed log evidence.  Keyword arguments as `eval` (model_only is refused)."""
        self._log_sf2 = float(log_sf2)  # (Problem.acquire's default var_floor)
        h, keep = self._hypers(log_ell, log_sf2, sigma2, inducing, tproj, variational, model_only, jitter,
                               log_hetero_skedasticity, log_multiscales_m05, reuse_v)
        res = TargetsResult()
        nh = self.n_hypers(tproj is not None, log_hetero_skedasticity is not None, log_multiscales_m05 is not None)
        grad = np.empty(nh if want_grad else 1, dtype=np.float64)
        l2 = np.zeros(_lib.MAX_TARGETS, dtype=np.float64)
        coeffs = np.zeros((self.m, _lib.MAX_TARGETS), dtype=np.float64, order="F")
        _lib.check(self._lib.gprhip_eval_targets(self._handle(), C.byref(h), int(want_grad), C.byref(res), _f64_ptr(l2),
                                                 _f64_ptr(grad), _f64_ptr(coeffs)))
        del keep
        k = int(res.k)
        l2 = l2[:k].copy()
        return TargetsEvaluation(res.l1, l2, res.l1 + l2, res.l_sum, res.dl_dsigma2_sum if want_grad else None,
                                 grad[:res.n_hypers] if want_grad else None, np.asfortranarray(coeffs[:, :k]))

    def predict_targets(self, test_inputs):
        """Means.calc per target column (lib/fitc_gp.ml:418-425) at test points (D x nt) with the coefficients of the last
        `eval_targets`: nt x k."""
        xt = np.asfortranarray(test_inputs, dtype=np.float64)
        if xt.ndim != 2 or xt.shape[0] != self.D:
            raise ValueError("predict_targets: expected test inputs of shape (%d, nt)" % self.D)
        nt = xt.shape[1]
        k = getattr(self, "_k", 0)
        means = np.empty((nt, max(k, 1)), dtype=np.float64, order="F")
        _lib.check(self._lib.gprhip_predict_targets(self._handle(), _f64_ptr(xt), self.D, nt, _f64_ptr(means)))
        return means

    # ---- prediction
    def predict(self, test_inputs, predictive=True, want_variances=True):
        """Means.calc / Variances.calc (lib/fitc_gp.ml:418-425, :498-518) at test points (D x nt), using
        the model state of the last evaluation.  Returns (means, variances or None)."""
        xt = np.asfortranarray(test_inputs, dtype=np.float64)
        if xt.ndim != 2 or xt.shape[0] != self.D:
            raise ValueError("predict: expected test inputs of shape (%d, nt)" % self.D)
        nt = xt.shape[1]
        means = np.empty(nt, dtype=np.float64)
        var = np.empty(nt, dtype=np.float64) if want_variances else None
        _lib.check(self._lib.gprhip_predict(self._handle(), _f64_ptr(xt), self.D, nt, int(predictive), _f64_ptr(means),
                                            _f64_ptr(var) if want_variances else None))
        return means, var

    PREDICT_OUTPUTS = ("means", "variances", "dmeans", "dvariances")

    def predict_input_grad(self, test_inputs, predictive=True, want=PREDICT_OUTPUTS, out_device_ptrs=None, nt=None, ldg=None):
        """Means and variances as `predict`, and their gradients with respect to the test inputs (gprhip_predict_input_grad):
        a dict with the names in `want` -- means / variances [nt], dmeans / dvariances D x nt in the layout of the test
        inputs.  A request without variances and dvariances runs the mean part alone.
        out_device_ptrs: {name: device address} for the names in `want` (means / variances: nt doubles, the gradients
        point-major [nt][D]); `test_inputs` is then the device address of a contiguous point-major [nt][D] fp64 array of
        `nt` points, the outputs are written in place and None is returned.
        ldg (host output only): leading dimension >= D of the gradient buffers; rows D.. are not written (they hold NaN).
        fp64 problems, no multiscales, at most 64 point dimensions on the kernel side (the library refuses otherwise)."""
        want = tuple(want)
        unknown = [w for w in want if w not in self.PREDICT_OUTPUTS]
        if unknown:
            raise ValueError("predict_input_grad: unknown outputs %s" % unknown)
        null = C.c_void_p(None)
        if out_device_ptrs is not None:
            if nt is None:
                raise ValueError("predict_input_grad: device buffers need nt")
            ptrs = [C.c_void_p(int(out_device_ptrs[w])) if w in want else null for w in self.PREDICT_OUTPUTS]
            _lib.check(self._lib.gprhip_predict_input_grad(self._handle(), C.c_void_p(int(test_inputs)), self.D, int(nt),
                                                           int(predictive), *ptrs, self.D, 1))
            return None
        xt = np.asfortranarray(test_inputs, dtype=np.float64)
        if xt.ndim != 2 or xt.shape[0] != self.D:
            raise ValueError("predict_input_grad: expected test inputs of shape (%d, nt)" % self.D)
        nt = xt.shape[1]
        ldv = self.D if ldg is None else int(ldg)
        out = {}
        for w in want:
            out[w] = (np.empty(nt, dtype=np.float64) if w in ("means", "variances")
                      else np.full((max(ldv, 1), nt), np.nan, dtype=np.float64, order="F"))
        ptrs = [C.c_void_p(out[w].ctypes.data) if w in out else null for w in self.PREDICT_OUTPUTS]
        _lib.check(self._lib.gprhip_predict_input_grad(self._handle(), C.c_void_p(xt.ctypes.data), self.D, nt, int(predictive),
                                                       *ptrs, ldv, 0))
        if ldg is None:
            for w in ("dmeans", "dvariances"):
                if w in out:
                    out[w] = out[w][:self.D]
        return out

    ACQUIRE_KINDS = {"ei": _lib.ACQ_EI, "log_ei": _lib.ACQ_LOG_EI, "pi": _lib.ACQ_PI, "bound": _lib.ACQ_BOUND}
    ACQUIRE_OUTPUTS = ("values", "dvalues", "means", "variances")

    def acquire(self, test_inputs, kind, *, maximise, best=0.0, xi=0.0, kappa=0.0, var_floor=None, predictive=False,
                want=("values", "dvalues"), top_k=0, out_device_ptrs=None, nt=None):
        """An acquisition criterion over candidate points (gprhip_acquire): kind "ei" | "log_ei" | "pi" | "bound" (or a
        GPRHIP_ACQ_* number), every one "larger is better"; maximise: larger targets are better.  best / xi: incumbent and
        margin of ei, log_ei, pi; kappa: weight of the standard deviation in bound.  The criterion sees the variance
        max(variance, var_floor) -- default 1e-10 sf2, the level of the variance's own error -- with sigma2 added when
        `predictive`.  Returns a dict with the names in `want` -- values / means / variances [nt], dvalues D x nt in the layout
        of the test inputs -- and, with top_k > 0 (at most 64), top_index [top_k] (the best candidates, value descending, the
        lower index first among equal values, -1 where fewer qualify), top_values [top_k] and top_dvalues D x top_k (NaN
        where top_index is -1).  want=() with top_k > 0 moves nothing of size nt off the device.
        out_device_ptrs: {name: device address} for the names in `want` (vectors: nt doubles, dvalues point-major [nt][D]);
        `test_inputs` is then the device address of a contiguous point-major [nt][D] fp64 array of `nt` points; only the
        top_* entries are returned."""
        want = tuple(want)
        unknown = [w for w in want if w not in self.ACQUIRE_OUTPUTS]
        if unknown:
            raise ValueError("acquire: unknown outputs %s" % unknown)
        if isinstance(kind, str):
            if kind not in self.ACQUIRE_KINDS:
                raise ValueError("acquire: unknown kind %r (one of %s)" % (kind, sorted(self.ACQUIRE_KINDS)))
            kind = self.ACQUIRE_KINDS[kind]
        if var_floor is None:
            if getattr(self, "_log_sf2", None) is None:
                raise ValueError("acquire: var_floor is needed (this object has not seen the model state's log_sf2)")
            var_floor = 1e-10 * float(np.exp(self._log_sf2))
        acq = _lib.Acquisition(int(kind), int(bool(maximise)), int(bool(predictive)), float(best), float(xi), float(kappa),
                               float(var_floor))
        top_k = int(top_k)
        out = {}
        kk = max(top_k, 1)
        top_index = np.full(kk, -1, dtype=np.int64)
        top_values = np.full(kk, np.nan, dtype=np.float64)
        top_dvalues = np.full((self.D, kk), np.nan, dtype=np.float64, order="F")
        tops = ((top_index.ctypes.data_as(C.POINTER(C.c_int64)), _f64_ptr(top_values), _f64_ptr(top_dvalues)) if top_k > 0
                else (None, None, None))
        null = C.c_void_p(None)
        if out_device_ptrs is not None:
            if nt is None:
                raise ValueError("acquire: device buffers need nt")
            ptrs = {w: (C.c_void_p(int(out_device_ptrs[w])) if w in want else null) for w in self.ACQUIRE_OUTPUTS}
            xt_ptr, on_device = C.c_void_p(int(test_inputs)), 1
            nt = int(nt)
        else:
            xt = np.asfortranarray(test_inputs, dtype=np.float64)
            if xt.ndim != 2 or xt.shape[0] != self.D:
                raise ValueError("acquire: expected test inputs of shape (%d, nt)" % self.D)
            nt = xt.shape[1]
            for w in want:
                out[w] = (np.full((self.D, nt), np.nan, dtype=np.float64, order="F") if w == "dvalues"
                          else np.empty(nt, dtype=np.float64))
            ptrs = {w: (C.c_void_p(out[w].ctypes.data) if w in out else null) for w in self.ACQUIRE_OUTPUTS}
            xt_ptr, on_device = C.c_void_p(xt.ctypes.data), 0
        _lib.check(self._lib.gprhip_acquire(self._handle(), C.byref(acq), xt_ptr, self.D, nt, ptrs["values"], ptrs["dvalues"],
                                            self.D, ptrs["means"], ptrs["variances"], top_k, *tops, on_device))
        if top_k > 0:
            out.update(top_index=top_index, top_values=top_values, top_dvalues=top_dvalues)
        return out

    def acquire_max_value(self, test_inputs, extremes, *, maximise, var_floor=None, want=("values", "dvalues"), top_k=0,
                          out_device_ptrs=None, nt=None):
        """Max-value entropy search over candidate points (gprhip_acquire_max_value): how much observing a candidate tells
        about the value of the optimum, "larger is better".  extremes: the extreme values e_j of f on 1 .. 64 drawn paths
        (host numbers) -- maxima when `maximise`, else minima; `sample_paths_refine` reports the objective s f, so e_j is s
        times its best value of draw j (`max_value_search` does all of it).  The criterion sees the latent variance
        max(variance, var_floor), default 1e-10 sf2.  `want`, top_k, the returned dict and out_device_ptrs / nt as `acquire`.
        `acquire_max_value_refine` refines candidates of this criterion."""
        want = tuple(want)
        unknown = [w for w in want if w not in self.ACQUIRE_OUTPUTS]
        if unknown:
            raise ValueError("acquire_max_value: unknown outputs %s" % unknown)
        ext = np.ascontiguousarray(extremes, dtype=np.float64)
        if ext.ndim != 1:
            raise ValueError("acquire_max_value: extremes is a vector")
        if var_floor is None:
            if getattr(self, "_log_sf2", None) is None:
                raise ValueError("acquire_max_value: var_floor is needed (this object has not seen the model state's log_sf2)")
            var_floor = 1e-10 * float(np.exp(self._log_sf2))
        top_k = int(top_k)
        out = {}
        kk = max(top_k, 1)
        top_index = np.full(kk, -1, dtype=np.int64)
        top_values = np.full(kk, np.nan, dtype=np.float64)
        top_dvalues = np.full((self.D, kk), np.nan, dtype=np.float64, order="F")
        tops = ((top_index.ctypes.data_as(C.POINTER(C.c_int64)), _f64_ptr(top_values), _f64_ptr(top_dvalues)) if top_k > 0
                else (None, None, None))
        null = C.c_void_p(None)
        if out_device_ptrs is not None:
            if nt is None:
                raise ValueError("acquire_max_value: device buffers need nt")
            ptrs = {w: (C.c_void_p(int(out_device_ptrs[w])) if w in want else null) for w in self.ACQUIRE_OUTPUTS}
            xt_ptr, on_device = C.c_void_p(int(test_inputs)), 1
            nt = int(nt)
        else:
            xt = np.asfortranarray(test_inputs, dtype=np.float64)
            if xt.ndim != 2 or xt.shape[0] != self.D:
                raise ValueError("acquire_max_value: expected test inputs of shape (%d, nt)" % self.D)
            nt = xt.shape[1]
            for w in want:
                out[w] = (np.full((self.D, nt), np.nan, dtype=np.float64, order="F") if w == "dvalues"
                          else np.empty(nt, dtype=np.float64))
            ptrs = {w: (C.c_void_p(out[w].ctypes.data) if w in out else null) for w in self.ACQUIRE_OUTPUTS}
            xt_ptr, on_device = C.c_void_p(xt.ctypes.data), 0
        _lib.check(self._lib.gprhip_acquire_max_value(self._handle(), _f64_ptr(ext) if ext.size else None, int(ext.size),
                                                      int(bool(maximise)), float(var_floor), xt_ptr, self.D, nt, ptrs["values"],
                                                      ptrs["dvalues"], self.D, ptrs["means"], ptrs["variances"], top_k, *tops,
                                                      on_device))
        if top_k > 0:
            out.update(top_index=top_index, top_values=top_values, top_dvalues=top_dvalues)
        return out

    def max_value_search(self, z, lower, upper, grid, top_k=4, refine_options=None, *, maximise=True, var_floor=None,
                         want=("values", "dvalues"), acquire_top_k=0, refine_top_k=0, candidate_refine_options=None):
        """Max-value entropy search end to end, host level.  z: m x nd standard normal draws (1 <= nd <= 64); grid: D x nt
        candidates inside the box [lower, upper].  In this order: `sample_paths` on the grid with the best top_k points per
        draw; `sample_paths_refine` from those winners (refine_options: its keyword arguments max_evals, step0, ...); per
        draw the best refined objective o_j; the extremes e_j = s o_j (the refinement reports the objective s f, s = +1 if
        maximise else -1); `acquire_max_value` over the grid (want, acquire_top_k: its want and top_k).  Returns its dict
        plus extremes [nd] and extreme_x (D x nd, where each was found).
        refine_top_k = k > 0: `acquire_max_value` runs with top_k = max(acquire_top_k, k), and its best k grid candidates are
        refined inside the box by `acquire_max_value_refine` (candidate_refine_options: its keyword arguments max_evals,
        step0, ...); the dict gains refined_x (D x k'), refined_values [k'], refined_dvalues (D x k') and refined_status
        [k'], k' <= k the candidates that qualified, best grid candidate first."""
        z = np.asfortranarray(z, dtype=np.float64)
        if z.ndim != 2:
            raise ValueError("max_value_search: expected z of shape (%d, nd)" % self.m)
        nd = z.shape[1]
        top_k = int(top_k)
        if top_k < 1:
            raise ValueError("max_value_search: top_k starts per draw, at least 1")
        grid = np.asfortranarray(grid, dtype=np.float64)
        tops = self.sample_paths(grid, z, maximise=maximise, top_k=top_k, want_samples=False)
        idx = tops["top_index"]                       # top_k x nd
        draw_of, cols = [], []
        for j in range(nd):
            for i in idx[:, j]:
                if i >= 0:
                    draw_of.append(j)
                    cols.append(int(i))
        if sorted(set(draw_of)) != list(range(nd)):
            raise ValueError("max_value_search: a draw has no finite sample on the grid")
        draw_of = np.asarray(draw_of, dtype=np.int32)
        ref = self.sample_paths_refine(grid[:, cols], z, draw_of, lower=lower, upper=upper, maximise=maximise,
                                       want=("x", "values"), **(refine_options or {}))
        extremes, where = self._extremes_of_refined(ref["values"], draw_of, nd, maximise)
        refine_top_k = int(refine_top_k)
        if refine_top_k < 0:
            raise ValueError("max_value_search: refine_top_k is a count, at least 0")
        out = self.acquire_max_value(grid, extremes, maximise=maximise, var_floor=var_floor, want=want,
                                     top_k=max(acquire_top_k, refine_top_k))
        out.update(extremes=extremes, extreme_x=np.asfortranarray(ref["x"][:, where]))
        if refine_top_k > 0:
            best = [int(i) for i in out["top_index"][:refine_top_k] if i >= 0]
            if not best:
                raise ValueError("max_value_search: no grid candidate has a finite criterion")
            fine = self.acquire_max_value_refine(grid[:, best], extremes, lower=lower, upper=upper, maximise=maximise,
                                                 var_floor=var_floor, want=("x", "values", "dvalues", "status"),
                                                 **(candidate_refine_options or {}))
            out.update(refined_x=fine["x"], refined_values=fine["values"], refined_dvalues=fine["dvalues"],
                       refined_status=fine["status"])
        return out

    @staticmethod
    def _extremes_of_refined(objective, draw_of, nd, maximise):
        """Per draw the best (largest) refined objective o_j -- the first among equal ones -- as the extreme e_j = s o_j of f,
        and the start that reached it."""
        objective = np.asarray(objective, dtype=np.float64)
        s = 1.0 if maximise else -1.0
        where = np.empty(nd, dtype=np.int64)
        for j in range(nd):
            mine = np.flatnonzero(np.asarray(draw_of) == j)
            where[j] = mine[np.argmax(objective[mine])]
        return s * objective[where], where

    REFINE_OUTPUTS = ("x", "values", "dvalues", "evals", "accepted", "status", "trace")

    def acquire_refine(self, starts, kind, *, lower, upper, maximise, scale=None, best=0.0, xi=0.0, kappa=0.0, var_floor=None,
                       predictive=False, max_evals=50, step0=0.1, c1=1e-4, shrink=0.5, grow=2.0, xtol=1e-8,
                       want=("x", "values", "dvalues", "evals", "accepted", "status"), out_device_ptrs=None, ns=None):
        """Refines candidates of an acquisition criterion on the device (gprhip_acquire_refine): projected gradient ascent with
        Armijo backtracking from the columns of `starts` (D x ns) inside the box [lower, upper] (D each), every start on its
        own.  kind and the criterion's keywords as `acquire`; scale (D, default ones) weights the gradient's components;
        max_evals / step0 / c1 / shrink / grow / xtol are the rule's constants (include/gprhip.h).  Returns a dict with the
        names in `want`: x (D x ns), values [ns] and dvalues (D x ns) -- value and gradient at x --, evals / accepted / status
        [ns] (int32; status one of _lib.REFINE_ST_*), trace [ns, max_evals, 2 D + 3] with one record (y, g_y, a_y, alpha,
        accepted) per evaluation and NaN where none was made.
        out_device_ptrs: {name: device address} for the names in `want` (x / dvalues point-major [ns][D], the integers int32,
        trace as above); `starts` is then the device address of a contiguous point-major [ns][D] fp64 array of `ns` points,
        the outputs are written in place and {} is returned."""
        want = tuple(want)
        unknown = [w for w in want if w not in self.REFINE_OUTPUTS]
        if unknown:
            raise ValueError("acquire_refine: unknown outputs %s" % unknown)
        if isinstance(kind, str):
            if kind not in self.ACQUIRE_KINDS:
                raise ValueError("acquire_refine: unknown kind %r (one of %s)" % (kind, sorted(self.ACQUIRE_KINDS)))
            kind = self.ACQUIRE_KINDS[kind]
        if var_floor is None:
            if getattr(self, "_log_sf2", None) is None:
                raise ValueError("acquire_refine: var_floor is needed (this object has not seen the model state's log_sf2)")
            var_floor = 1e-10 * float(np.exp(self._log_sf2))
        acq = _lib.Acquisition(int(kind), int(bool(maximise)), int(bool(predictive)), float(best), float(xi), float(kappa),
                               float(var_floor))
        opt = _lib.RefineOptions(int(max_evals), float(step0), float(c1), float(shrink), float(grow), float(xtol))
        box = [np.ascontiguousarray(b, dtype=np.float64) for b in (lower, upper)]
        if scale is not None:
            box.append(np.ascontiguousarray(scale, dtype=np.float64))
        if any(b.shape != (self.D,) for b in box):
            raise ValueError("acquire_refine: lower, upper and scale take %d entries each" % self.D)
        bptr = [_f64_ptr(b) for b in box] + ([None] if scale is None else [])
        null = C.c_void_p(None)
        out = {}
        if out_device_ptrs is not None:
            if ns is None:
                raise ValueError("acquire_refine: device buffers need ns")
            ptrs = {w: (C.c_void_p(int(out_device_ptrs[w])) if w in want else null) for w in self.REFINE_OUTPUTS}
            st_ptr, on_device, ns = C.c_void_p(int(starts)), 1, int(ns)
        else:
            xs = np.asfortranarray(starts, dtype=np.float64)
            if xs.ndim != 2 or xs.shape[0] != self.D:
                raise ValueError("acquire_refine: expected starts of shape (%d, ns)" % self.D)
            ns = xs.shape[1]
            for w in want:
                if w in ("x", "dvalues"):
                    out[w] = np.full((self.D, ns), np.nan, dtype=np.float64, order="F")
                elif w == "values":
                    out[w] = np.full(ns, np.nan, dtype=np.float64)
                elif w == "trace":
                    out[w] = np.full((ns, int(max_evals), 2 * self.D + 3), np.nan, dtype=np.float64)
                else:
                    out[w] = np.full(ns, -1, dtype=np.int32)
            ptrs = {w: (C.c_void_p(out[w].ctypes.data) if w in out else null) for w in self.REFINE_OUTPUTS}
            st_ptr, on_device = C.c_void_p(xs.ctypes.data), 0
        _lib.check(self._lib.gprhip_acquire_refine(self._handle(), C.byref(acq), C.byref(opt), *bptr, st_ptr, self.D, ns,
                                                   ptrs["x"], self.D, ptrs["values"], ptrs["dvalues"], self.D, ptrs["evals"],
                                                   ptrs["accepted"], ptrs["status"], ptrs["trace"], on_device))
        return out

    def acquire_max_value_refine(self, starts, extremes, *, lower, upper, maximise, scale=None, var_floor=None, max_evals=50,
                                 step0=0.1, c1=1e-4, shrink=0.5, grow=2.0, xtol=1e-8,
                                 want=("x", "values", "dvalues", "evals", "accepted", "status"), out_device_ptrs=None, ns=None):
        """Refines candidates of max-value entropy search on the device (gprhip_acquire_max_value_refine): the rule of
        `acquire_refine` on the criterion of `acquire_max_value` -- extremes, maximise and var_floor as there (host numbers,
        the latent variance).  Box, scale, the rule's constants, `want`, the outputs and out_device_ptrs / ns as
        `acquire_refine`."""
        want = tuple(want)
        unknown = [w for w in want if w not in self.REFINE_OUTPUTS]
        if unknown:
            raise ValueError("acquire_max_value_refine: unknown outputs %s" % unknown)
        ext = np.ascontiguousarray(extremes, dtype=np.float64)
        if ext.ndim != 1:
            raise ValueError("acquire_max_value_refine: extremes is a vector")
        if var_floor is None:
            if getattr(self, "_log_sf2", None) is None:
                raise ValueError("acquire_max_value_refine: var_floor is needed (this object has not seen the model state's "
                                 "log_sf2)")
            var_floor = 1e-10 * float(np.exp(self._log_sf2))
        opt = _lib.RefineOptions(int(max_evals), float(step0), float(c1), float(shrink), float(grow), float(xtol))
        box = [np.ascontiguousarray(b, dtype=np.float64) for b in (lower, upper)]
        if scale is not None:
            box.append(np.ascontiguousarray(scale, dtype=np.float64))
        if any(b.shape != (self.D,) for b in box):
            raise ValueError("acquire_max_value_refine: lower, upper and scale take %d entries each" % self.D)
        bptr = [_f64_ptr(b) for b in box] + ([None] if scale is None else [])
        null = C.c_void_p(None)
        out = {}
        if out_device_ptrs is not None:
            if ns is None:
                raise ValueError("acquire_max_value_refine: device buffers need ns")
            ptrs = {w: (C.c_void_p(int(out_device_ptrs[w])) if w in want else null) for w in self.REFINE_OUTPUTS}
            st_ptr, on_device, ns = C.c_void_p(int(starts)), 1, int(ns)
        else:
            xs = np.asfortranarray(starts, dtype=np.float64)
            if xs.ndim != 2 or xs.shape[0] != self.D:
                raise ValueError("acquire_max_value_refine: expected starts of shape (%d, ns)" % self.D)
            ns = xs.shape[1]
            for w in want:
                if w in ("x", "dvalues"):
                    out[w] = np.full((self.D, ns), np.nan, dtype=np.float64, order="F")
                elif w == "values":
                    out[w] = np.full(ns, np.nan, dtype=np.float64)
                elif w == "trace":
                    out[w] = np.full((ns, int(max_evals), 2 * self.D + 3), np.nan, dtype=np.float64)
                else:
                    out[w] = np.full(ns, -1, dtype=np.int32)
            ptrs = {w: (C.c_void_p(out[w].ctypes.data) if w in out else null) for w in self.REFINE_OUTPUTS}
            st_ptr, on_device = C.c_void_p(xs.ctypes.data), 0
        _lib.check(self._lib.gprhip_acquire_max_value_refine(
            self._handle(), _f64_ptr(ext) if ext.size else None, int(ext.size), int(bool(maximise)), float(var_floor),
            C.byref(opt), *bptr, st_ptr, self.D, ns, ptrs["x"], self.D, ptrs["values"], ptrs["dvalues"], self.D, ptrs["evals"],
            ptrs["accepted"], ptrs["status"], ptrs["trace"], on_device))
        return out

    def sample_paths_refine(self, starts, z, draw_of, *, lower, upper, maximise=True, scale=None, max_evals=50, step0=0.1,
                            c1=1e-4, shrink=0.5, grow=2.0, xtol=1e-8,
                            want=("x", "values", "dvalues", "evals", "accepted", "status"), out_device_ptrs=None, ns=None):
        """Refines drawn sample paths on the device (gprhip_sample_paths_refine): the rule of `acquire_refine` on the draws of
        `sample_paths`.  z: m x nd standard normal draws (host, 1 <= nd <= 64), the same z as in `sample_paths` gives the same
        functions; draw_of: ns integers in 0 .. nd - 1, the draw that each column of `starts` (D x ns) climbs.  The objective
        is s f_j with s = +1 if maximise else -1: values, dvalues and the trace hold the objective and its gradient, not the
        unsigned path.  Box, scale, the rule's constants, `want`, the outputs and out_device_ptrs / ns as `acquire_refine`
        (z and draw_of stay host arrays)."""
        want = tuple(want)
        unknown = [w for w in want if w not in self.REFINE_OUTPUTS]
        if unknown:
            raise ValueError("sample_paths_refine: unknown outputs %s" % unknown)
        z = np.asfortranarray(z, dtype=np.float64)
        if z.ndim != 2 or z.shape[0] != self.m:
            raise ValueError("sample_paths_refine: expected z of shape (%d, nd)" % self.m)
        nd = z.shape[1]
        opt = _lib.RefineOptions(int(max_evals), float(step0), float(c1), float(shrink), float(grow), float(xtol))
        box = [np.ascontiguousarray(b, dtype=np.float64) for b in (lower, upper)]
        if scale is not None:
            box.append(np.ascontiguousarray(scale, dtype=np.float64))
        if any(b.shape != (self.D,) for b in box):
            raise ValueError("sample_paths_refine: lower, upper and scale take %d entries each" % self.D)
        bptr = [_f64_ptr(b) for b in box] + ([None] if scale is None else [])
        null = C.c_void_p(None)
        out = {}
        if out_device_ptrs is not None:
            if ns is None:
                raise ValueError("sample_paths_refine: device buffers need ns")
            ptrs = {w: (C.c_void_p(int(out_device_ptrs[w])) if w in want else null) for w in self.REFINE_OUTPUTS}
            st_ptr, on_device, ns = C.c_void_p(int(starts)), 1, int(ns)
        else:
            xs = np.asfortranarray(starts, dtype=np.float64)
            if xs.ndim != 2 or xs.shape[0] != self.D:
                raise ValueError("sample_paths_refine: expected starts of shape (%d, ns)" % self.D)
            ns = xs.shape[1]
            for w in want:
                if w in ("x", "dvalues"):
                    out[w] = np.full((self.D, ns), np.nan, dtype=np.float64, order="F")
                elif w == "values":
                    out[w] = np.full(ns, np.nan, dtype=np.float64)
                elif w == "trace":
                    out[w] = np.full((ns, int(max_evals), 2 * self.D + 3), np.nan, dtype=np.float64)
                else:
                    out[w] = np.full(ns, -1, dtype=np.int32)
            ptrs = {w: (C.c_void_p(out[w].ctypes.data) if w in out else null) for w in self.REFINE_OUTPUTS}
            st_ptr, on_device = C.c_void_p(xs.ctypes.data), 0
        dr = np.ascontiguousarray(draw_of, dtype=np.int32)
        if dr.shape != (ns,):
            raise ValueError("sample_paths_refine: draw_of takes %d entries" % ns)
        self._sp_ns_last = 0  # (until the call returns: a call that raises may or may not have formed its weights)
        _lib.check(self._lib.gprhip_sample_paths_refine(self._handle(), _f64_ptr(z), self.m, nd, int(bool(maximise)), C.byref(opt),
                                                        *bptr, st_ptr, self.D, ns, dr.ctypes.data_as(C.POINTER(C.c_int)),
                                                        ptrs["x"], self.D, ptrs["values"], ptrs["dvalues"], self.D,
                                                        ptrs["evals"], ptrs["accepted"], ptrs["status"], ptrs["trace"], on_device))
        self._sp_ns_last = nd  # (debug_fetch_matrix("sp_a"))
        return out

    def sample_paths(self, test_inputs, z, eps=None, predictive=False, maximise=True, top_k=0, want_samples=True,
                     out_device_ptrs=None, nt=None):
        """Posterior sample paths at test points (gprhip_sample_paths).  z: m x ns standard normal draws (host, 1 <= ns <= 64);
        column j fixes the draw f_j(x) = sum_c k(x, z_c) a_cj, a_j = t + R^-1 z_j, a function that the same z evaluates again
        at any other points.  eps: nt x ns standard normal draws, or None for the path part alone; with eps the sample adds
        sqrt(max(0, sf2 - |K_r U^-1|^2 (+ sigma2 if predictive))) eps, so that mean and variance are those of `predict`.
        Returns a dict: samples (nt x ns, unless want_samples is False) and, with top_k > 0 (at most 64), per draw top_index
        (top_k x ns; the largest -- maximise=False: the smallest -- samples first, the lower index first among equal values,
        -1 where fewer qualify), top_values (top_k x ns) and top_dvalues (D x top_k x ns: the gradient of the PATH part at each
        winner; NaN where top_index is -1).  want_samples=False with top_k > 0 moves nothing of size nt off the device.
        out_device_ptrs: {"samples": device address of [ns][nt] doubles} (or {} for the top_* entries alone); `test_inputs`
        is then the device address of a contiguous point-major [nt][D] fp64 array, `nt` (required then, else not used) the
        number of points, `eps` None or the device address (an int) of [ns][nt] doubles -- an array is refused --, and only
        the top_* entries are returned.
        fp64 problems, no multiscales, at most 64 point dimensions on the kernel side (the library refuses otherwise)."""
        z = np.asfortranarray(z, dtype=np.float64)
        if z.ndim == 1:
            z = np.asfortranarray(z.reshape(-1, 1))
        if z.ndim != 2 or z.shape[0] != self.m:
            raise ValueError("sample_paths: expected z of shape (%d, ns)" % self.m)
        ns = z.shape[1]
        top_k = int(top_k)
        kk = max(top_k, 1)
        top_index = np.full((kk, max(ns, 1)), -1, dtype=np.int64, order="F")
        top_values = np.full((kk, max(ns, 1)), np.nan, dtype=np.float64, order="F")
        top_dvalues = np.full((self.D, kk, max(ns, 1)), np.nan, dtype=np.float64, order="F")
        tops = ((top_index.ctypes.data_as(C.POINTER(C.c_int64)), _f64_ptr(top_values), _f64_ptr(top_dvalues)) if top_k > 0
                else (None, None, None))
        null = C.c_void_p(None)
        out = {}
        if out_device_ptrs is not None:
            if nt is None:
                raise ValueError("sample_paths: device buffers need nt")
            nt = int(nt)
            unknown = [w for w in out_device_ptrs if w != "samples"]
            if unknown:
                raise ValueError("sample_paths: unknown device outputs %s" % unknown)
            if eps is not None and not isinstance(eps, (int, np.integer)):
                raise TypeError("sample_paths: with device buffers eps is a device address (an int), not an array")
            sp = C.c_void_p(int(out_device_ptrs["samples"])) if out_device_ptrs.get("samples") else null
            ep = C.c_void_p(int(eps)) if eps is not None else null
            xt_ptr, on_device = C.c_void_p(int(test_inputs)), 1
        else:
            xt = np.asfortranarray(test_inputs, dtype=np.float64)
            if xt.ndim != 2 or xt.shape[0] != self.D:
                raise ValueError("sample_paths: expected test inputs of shape (%d, nt)" % self.D)
            nt = xt.shape[1]
            if eps is not None:
                eps = np.asfortranarray(eps, dtype=np.float64)
                if eps.ndim == 1:
                    eps = np.asfortranarray(eps.reshape(-1, 1))
                if eps.shape != (nt, ns):
                    raise ValueError("sample_paths: expected eps of shape (%d, %d)" % (nt, ns))
            if want_samples:
                out["samples"] = np.empty((nt, ns), dtype=np.float64, order="F")
            sp = C.c_void_p(out["samples"].ctypes.data) if want_samples else null
            ep = C.c_void_p(eps.ctypes.data) if eps is not None else null
            xt_ptr, on_device = C.c_void_p(xt.ctypes.data), 0
        self._sp_ns_last = 0  # (until the call returns: a call that raises may or may not have formed its weights)
        _lib.check(self._lib.gprhip_sample_paths(self._handle(), _f64_ptr(z), self.m, ns, xt_ptr, self.D, nt, ep, nt,
                                                 int(bool(predictive)), sp, nt, int(bool(maximise)), top_k, *tops, on_device))
        self._sp_ns_last = ns  # (debug_fetch_matrix("sp_a"))
        if top_k > 0:
            out.update(top_index=top_index, top_values=top_values, top_dvalues=top_dvalues)
        return out

    def train_stats(self, want_means=False):
        """Residual sums of the training set under the last evaluation's mean coefficients
        (Trained.calc_means + the loops of Stats.calc, lib/fitc_gp.ml:296-297, :353-373).
        Returns (sums = [sse, sum|y-mean|, max|y-mean|, sum y^2], means or None)."""
        sums = np.empty(4, dtype=np.float64)
        means = np.empty(self.n, dtype=np.float64) if want_means else None
        _lib.check(self._lib.gprhip_train_stats(self._handle(), _f64_ptr(means) if want_means else None,
                                                _f64_ptr(sums)))
        return sums, means

    def covariances(self, test_inputs, kind="FITC", predictive=True):
        """FITC_covariances.calc / FIC_covariances.calc (lib/fitc_gp.ml:585-599, :617-627): nt x nt posterior
        covariance between the test points (full symmetric matrix)."""
        xt = np.asfortranarray(test_inputs, dtype=np.float64)
        if xt.ndim != 2 or xt.shape[0] != self.D:
            raise ValueError("covariances: expected test inputs of shape (%d, nt)" % self.D)
        nt = xt.shape[1]
        cov = np.empty((nt, nt), dtype=np.float64, order="F")
        _lib.check(self._lib.gprhip_covariances(self._handle(), _f64_ptr(xt), self.D, nt, {"FITC": 0, "FIC": 1}[kind],
                                                int(predictive), _f64_ptr(cov)))
        return cov

    def cov_samples(self, covariances, means, z, add_diag=0.0, jitter=CHOLESKY_JITTER):
        """Common_cov_sampler.calc + samples (lib/fitc_gp.ml:656-697): means + chol(cov + (add_diag+jitter) I)^T z
        for every column of z (nt x ns standard normal draws)."""
        cov = np.asfortranarray(covariances, dtype=np.float64)
        nt = cov.shape[0]
        means = np.ascontiguousarray(means, dtype=np.float64)
        z = np.asfortranarray(z, dtype=np.float64)
        if z.ndim == 1:
            z = np.asfortranarray(z.reshape(nt, 1))
        if cov.shape != (nt, nt) or means.shape != (nt,) or z.shape[0] != nt:
            raise ValueError("cov_samples: shapes of covariances/means/z disagree")
        ns = z.shape[1]
        out = np.empty((nt, ns), dtype=np.float64, order="F")
        _lib.check(self._lib.gprhip_cov_samples(self._handle(), _f64_ptr(cov), nt, nt, float(add_diag), float(jitter),
                                                _f64_ptr(means), _f64_ptr(z), ns, _f64_ptr(out)))
        return out

    # ---- model export / import (bin/ocaml_gpr.ml:207-232, :373-413)
    def co_variance_coeffs(self):
        """Model.calc_co_variance_coeffs (lib/fitc_gp.ml:240): (chol_km, r_mat) of the last evaluation, each an
        m x m upper-triangular Fortran matrix."""
        u = np.empty((self.m, self.m), dtype=np.float64, order="F")
        r = np.empty((self.m, self.m), dtype=np.float64, order="F")
        _lib.check(self._lib.gprhip_co_variance_coeffs(self._handle(), _f64_ptr(u), _f64_ptr(r)))
        return u, r

    def load_predictor(self, *, log_sf2, sigma2, inducing, coeffs=None, co_variance_coeffs=None, log_ell=0.0,
                       tproj=None, jitter=CHOLESKY_JITTER, log_hetero_skedasticity=None,
                       log_multiscales_m05=None):
        """Mean_predictor.calc / Co_variance_predictor.calc (lib/fitc_gp.ml:386-391, :446-447): install a saved
        model's predictor state; `predict` / `covariances` then work without any evaluation."""
        self._log_sf2 = float(log_sf2)  # (Problem.acquire's default var_floor)
        h, keep = self._hypers(log_ell, log_sf2, sigma2, inducing, tproj, False, False, jitter,
                               log_hetero_skedasticity, log_multiscales_m05)
        c = u = r = None
        if coeffs is not None:
            c = np.ascontiguousarray(coeffs, dtype=np.float64)
            if c.shape != (self.m,):  # lib/fitc_gp.ml:387-390
                raise ValueError("Mean_predictor.calc: number of inducing points disagrees with dimension of "
                                 "coefficients")
        if co_variance_coeffs is not None:
            u = np.asfortranarray(co_variance_coeffs[0], dtype=np.float64)
            r = np.asfortranarray(co_variance_coeffs[1], dtype=np.float64)
            if u.shape != (self.m, self.m) or r.shape != (self.m, self.m):
                raise ValueError("Co_variance_predictor.calc: expected two %d x %d factors" % (self.m, self.m))
        _lib.check(self._lib.gprhip_load_predictor(self._handle(), C.byref(h), _f64_ptr(c) if c is not None else None,
                                                   _f64_ptr(u) if u is not None else None,
                                                   _f64_ptr(r) if r is not None else None))
        del keep

    # ---- observations folded into the posterior without a refit (an extension beyond the reference's surface)
    def observe(self, inputs, targets=None, want_dlog_evidence=False, device_ptrs=None):
        """gprhip_observe: folds k <= 64 new observations into the predictor state of the last evaluation or load_predictor --
        a QR update of the whitened factors, O(k m^2); every posterior call then reads the conditioned model.  inputs: D x k
        (one point per column), targets: k values, or None for a state without targets (model_only, or a predictor loaded
        without coefficients).  The resident training set is not touched: the next eval forgets the observations.
        device_ptrs: (inputs address, targets address or None, k) of point-major [k][D] / [k] fp64 device arrays, used
        instead of `inputs` / `targets`.
        Returns the joint log density of the new targets given everything before them (the evidence of the enlarged data set
        minus the evidence before, at fixed hyper-parameters) when want_dlog_evidence, else None."""
        dl = C.c_double(0.0)
        dlp = C.byref(dl) if want_dlog_evidence else None
        if device_ptrs is not None:
            xp, yp, k = device_ptrs
            _lib.check(self._lib.gprhip_observe(self._handle(), C.c_void_p(int(xp)), self.D,
                                                C.c_void_p(int(yp)) if yp is not None else None, int(k), dlp, 1))
        else:
            x = np.asfortranarray(inputs, dtype=np.float64)
            if x.ndim == 1:
                if x.shape[0] != self.D:  # (a flat list of several points has no one reading)
                    raise ValueError("observe: a 1-D input is ONE point of %d coordinates; pass several as (%d, k)" % (self.D, self.D))
                x = np.asfortranarray(x.reshape(self.D, 1))
            if x.ndim != 2 or x.shape[0] != self.D:
                raise ValueError("observe: expected inputs of shape (%d, k)" % self.D)
            k = x.shape[1]
            y = None
            if targets is not None:
                y = np.ascontiguousarray(np.atleast_1d(targets), dtype=np.float64)
                if y.shape != (k,):
                    raise ValueError("observe: expected %d targets" % k)
            _lib.check(self._lib.gprhip_observe(self._handle(), C.c_void_p(x.ctypes.data), self.D,
                                                C.c_void_p(y.ctypes.data) if y is not None else None, k, dlp, 0))
        self._sp_ns_last = 0  # (the weights of the last sample_paths call belong to the state before)
        return dl.value if want_dlog_evidence else None

    def posterior_save(self):
        """gprhip_posterior_save: copies R~, R~^-1, b, t~, t and the observed count into the problem's one slot."""
        _lib.check(self._lib.gprhip_posterior_save(self._handle()))

    def posterior_restore(self):
        """gprhip_posterior_restore: the saved posterior back (the slot is kept); a state error without a slot of this model
        state -- an evaluation and load_predictor drop it."""
        _lib.check(self._lib.gprhip_posterior_restore(self._handle()))
        self._sp_ns_last = 0

    @property
    def observed_count(self):
        """Observations folded in since the last evaluation or load_predictor."""
        return int(self._lib.gprhip_observed_count(self._handle()))

    # ---- staged evaluation (row-sharded across devices; see gpr_amd/dist.py)
    def ar1_len(self):
        return int(self._lib.gprhip_ar1_len(self._handle()))

    def ar2_len(self):
        return int(self._lib.gprhip_ar2_len(self._handle()))

    def eval_pass1(self, ar1_ptr, n_total, *, log_sf2, sigma2, inducing, log_ell=0.0, tproj=None,
                   variational=False, model_only=False, want_grad=True, jitter=CHOLESKY_JITTER,
                   log_hetero_skedasticity=None, log_multiscales_m05=None, reuse_v=False):
        self._log_sf2 = float(log_sf2)  # (Problem.acquire's default var_floor)
        h, keep = self._hypers(log_ell, log_sf2, sigma2, inducing, tproj, variational, model_only, jitter,
                               log_hetero_skedasticity, log_multiscales_m05, reuse_v)
        self._has_ms = log_multiscales_m05 is not None
        self._want_grad = bool(want_grad)
        self._has_tproj = tproj is not None
        self._has_het = log_hetero_skedasticity is not None
        _lib.check(self._lib.gprhip_eval_pass1(self._handle(), C.byref(h), int(want_grad), int(n_total),
                                               C.c_void_p(ar1_ptr)))
        del keep  # the library copies borrowed host buffers before returning

    def eval_pass2(self, ar1_ptr, ar2_ptr):
        _lib.check(self._lib.gprhip_eval_pass2(self._handle(), C.c_void_p(ar1_ptr), C.c_void_p(ar2_ptr)))

    def eval_finish(self, ar2_ptr):
        res = Result()
        nh = self.n_hypers(self._has_tproj, self._has_het, self._has_ms)
        grad = np.empty(nh if self._want_grad else 1, dtype=np.float64)
        coeffs = np.empty(self.m, dtype=np.float64)
        _lib.check(self._lib.gprhip_eval_finish(self._handle(), C.c_void_p(ar2_ptr), C.byref(res),
                                                _f64_ptr(grad), _f64_ptr(coeffs)))
        return Evaluation(res.l1, res.l2, res.l, res.dl_dsigma2 if self._want_grad else None,
                          grad[:res.n_hypers] if self._want_grad else None, coeffs)

    def sync(self):
        _lib.check(self._lib.gprhip_sync(self._handle()))

    def stream(self):
        return self._lib.gprhip_stream(self._handle())

    # ---- diagnostics
    def set_timing(self, level):
        """0: none; 1: HIP events around the dominant kernel (pass-1 SYRK); 2: around every stage."""
        _lib.check(self._lib.gprhip_set_timing(self._handle(), int(level)))

    def condition(self):
        """(cond estimate of K_m + jitter, relative error bound of the mean coefficients) of the current model state."""
        c, b = C.c_double(), C.c_double()
        _lib.check(self._lib.gprhip_condition(self._handle(), C.byref(c), C.byref(b)))
        return c.value, b.value

    def debug_fetch(self, name):
        length = self.m if name in ("t", "bvec") else self.n
        out = np.empty(length, dtype=np.float64)
        _lib.check(self._lib.gprhip_debug_fetch(self._handle(), name.encode(), _f64_ptr(out), length))
        return out

    def debug_fetch_matrix(self, name, rows=None):
        """"km": K_m of the last evaluation (m x m, upper triangle valid, zeros below); "knm_rows": the first `rows`
        rows of K_nm rebuilt with the last evaluation's kernel (rows x m); "uinv", "rinv": U^-1 and R~^-1 as the posterior
        calls read them (m x m, upper triangle, zeros below; they need the factors of an evaluation or of a predictor loaded
        with co-variance coefficients); "rtil": R~ as stored, what `observe` updates (the same layout and conditions;
        `debug_fetch("bvec")` gives b); "pg_m": M = U^-1 (I - R~^-1 R~^-T) U^-T as the product G = K M of predict_input_grad
        and acquire reads it (m x m, full; available once such a call has formed it -- stage "pg_m" --, until the next
        evaluation or load_predictor; `rows` = m rounded up to a multiple of 128 returns the padded matrix as it is stored);
        "sp_a": the weights A = t 1^T + U^-1 (R~^-1 Z) of the last sample_paths / sample_paths_refine call of this object, as
        its kernels read them (m x ns of that call; a state error before any such call and after the next evaluation or
        load_predictor; `rows` = m rounded up to a multiple of 128 returns the padded rows x 64 block as it is stored).  For "pg_m" and "sp_a" any other `rows` than m or that
        padded count is a ValueError: the library tells the two layouts apart by the length alone."""
        if name in ("pg_m", "sp_a"):
            # the library picks the padded or the plain layout from the length alone: only the two row counts it knows pass
            mp = -(-self.m // 128) * 128
            if rows is not None and int(rows) not in (self.m, mp):
                raise ValueError("debug_fetch_matrix: %r takes rows = %d (the default) or %d (padded)" % (name, self.m, mp))
            padded = rows is not None and int(rows) == mp
        if name == "pg_m":
            w = mp if padded else self.m
            out = np.empty((w, w), dtype=np.float64, order="F")
        elif name == "sp_a":
            # the draw count of the last call that returned; 0 while a call is under way or after one that raised -- one column
            # is asked for then, and the library, which holds the count too, refuses where that is not what it has
            ns = getattr(self, "_sp_ns_last", 0) or 1
            out = np.empty((mp, 64) if padded else (self.m, ns), dtype=np.float64, order="F")
        elif name in ("km", "w_mat", "uinv", "rinv", "rtil"):
            out = np.empty((self.m, self.m), dtype=np.float64, order="F")
        elif name in ("knm_rows", "x_rows"):
            out = np.empty((int(rows), self.m), dtype=np.float64, order="F")
        else:
            raise ValueError("debug_fetch_matrix: unknown name %r" % name)
        _lib.check(self._lib.gprhip_debug_fetch(self._handle(), name.encode(), _f64_ptr(out), out.size))
        return out

    def batch(self, lanes):
        """A `Batch` of `lanes` lanes on this problem: up to 64 hyper-parameter sets against its resident data in one
        chain of launches (gprhip_batch_*; small path only: fp64, m <= 64, d <= 16)."""
        return Batch(self, lanes)

    def last_timings(self):
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        k = self._lib.gprhip_last_timings(self._handle(), names, ms, 32)
        return {names[i].decode(): float(ms[i]) for i in range(k)}


class _LaneProblem(Problem):
    """A lane's problem of a `Batch`, owned by the batch: predictions and diagnostics after a batch evaluation."""

    def __init__(self, batch, handle):
        parent = batch.problem
        self._lib = parent._lib
        self._h = C.c_void_p(handle)
        self._batch = batch  # (keeps the owner alive)
        self.cov_kind, self.n, self.D, self.d, self.m = parent.cov_kind, parent.n, parent.D, parent.d, parent.m
        self.device, self.precision = parent.device, parent.precision

    def _handle(self):
        if not self._batch.is_open():
            raise _lib.GprHipError(_lib.ESTATE, "gpr_amd.Batch: the batch has been closed")
        return self._h

    def close(self):
        self._h = C.c_void_p()  # owned by the batch


class Batch:
    """Several hyper-parameter sets against one resident data set in one pass (gprhip_batch_create / _eval).

    `eval(hypers_list, want_grad)` takes one dict of `Problem.eval`'s keyword arguments per lane and returns
    (evaluations, statuses): evaluations[j] is an `Evaluation`, or None where statuses[j] is not OK (a refused
    factorisation; `last_error` holds the first such message).  `lane(j)` serves predictions from lane j's state."""

    def __init__(self, problem, lanes):
        self._lib = _lib.load()
        self.problem = problem
        self._h = C.c_void_p()
        _lib.check(self._lib.gprhip_batch_create(problem._handle(), int(lanes), C.byref(self._h)))
        self.lanes = int(self._lib.gprhip_batch_lanes(self._h))
        self.last_error = ""

    def is_open(self):
        return bool(self._h)

    def close(self):
        if self._h:
            self._lib.gprhip_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lane(self, j):
        if not self._h:
            raise _lib.GprHipError(_lib.ESTATE, "gpr_amd.Batch: the batch has been closed")
        h = self._lib.gprhip_batch_lane(self._h, int(j))
        if not h:
            raise IndexError("Batch.lane: lane %d of %d" % (j, self.lanes))
        return _LaneProblem(self, h)

    def eval(self, hypers_list, want_grad=True):
        if not self._h:
            raise _lib.GprHipError(_lib.ESTATE, "gpr_amd.Batch: the batch has been closed")
        p = self.problem
        count = len(hypers_list)
        hs = (Hypers * max(count, 1))()
        keep = []
        nh = 1
        for j, kw in enumerate(hypers_list):
            kw = dict(kw)
            h, k = p._hypers(kw.pop("log_ell", 0.0), kw.pop("log_sf2"), kw.pop("sigma2"), kw.pop("inducing"),
                             kw.pop("tproj", None), kw.pop("variational", False), kw.pop("model_only", False),
                             kw.pop("jitter", CHOLESKY_JITTER), kw.pop("log_hetero_skedasticity", None),
                             kw.pop("log_multiscales_m05", None), kw.pop("reuse_v", False))
            if kw:
                raise TypeError("Batch.eval: unknown hyper-parameter names %s" % sorted(kw))
            hs[j] = h
            keep.append(k)
            nh = max(nh, p.n_hypers(bool(h.tproj), bool(h.log_hetero_skedasticity), bool(h.log_multiscales_m05)))
        res = (Result * max(count, 1))()
        grad = np.empty((nh, max(count, 1)), dtype=np.float64, order="F")
        coeffs = np.empty((p.m, max(count, 1)), dtype=np.float64, order="F")
        status = (C.c_int * max(count, 1))()
        _lib.check(self._lib.gprhip_batch_eval(self._h, count, hs, int(want_grad), res, _f64_ptr(grad), nh,
                                               _f64_ptr(coeffs), status))
        del keep
        statuses = [int(status[j]) for j in range(count)]
        self.last_error = "" if all(s == _lib.OK for s in statuses) else self._lib.gprhip_last_error().decode("utf-8", "replace")
        evs = []
        for j in range(count):
            if statuses[j] != _lib.OK:
                evs.append(None)
                continue
            r = res[j]
            evs.append(Evaluation(r.l1, r.l2, r.l, r.dl_dsigma2 if want_grad else None,
                                  grad[:r.n_hypers, j].copy() if want_grad else None, coeffs[:, j].copy()))
        return evs, statuses
