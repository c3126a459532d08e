"""PyTorch front end of the input gradient: the FITC log evidence as a differentiable function of the training inputs and
the hyper-parameters, evaluated by the HIP library on the tensors' own device memory.

    l = log_evidence(problem, inputs, targets, log_sf2=..., log_sigma2=..., inducing=..., log_ell=..., tproj=...)
    l.backward()

`inputs` may be the output of anything trainable (a feature extractor in front of the GP, an input warping, latent inputs):
its gradient is written by the library straight into a fresh tensor (gprhip_eval_input_grad, on_device = 1).

`predict(problem, test_inputs)` is the posterior side: predictive mean and variance as differentiable functions of the test
inputs (gprhip_predict_input_grad, on_device = 1) -- an acquisition function over candidate points, an input uncertainty pushed
through the model, a feature extractor in front of the GP at prediction time.

`acquire(problem, test_inputs, kind, ...)` is an acquisition criterion over candidate points (expected improvement, its
logarithm, probability of improvement, a confidence bound) as a differentiable function of them (gprhip_acquire, on_device = 1);
`acquire_max_value(problem, test_inputs, extremes, ...)` is max-value entropy search in the same way (gprhip_acquire_max_value).

torch is imported when `log_evidence`, `predict` or `acquire` is first called, not with this module: `import gpr_amd` never starts importing it.
"""
from __future__ import annotations

import numpy as np

from . import _lib

_fn = None


def _function():
    """The torch.autograd.Function, made at first use."""
    global _fn
    if _fn is not None:
        return _fn
    import torch
    from torch.autograd.function import once_differentiable

    class _LogEvidence(torch.autograd.Function):
        @staticmethod
        def forward(ctx, problem, variational, inputs, targets, log_sf2, log_sigma2, inducing, log_ell, tproj):
            n, D, d, m = problem.n, problem.D, problem.d, problem.m
            if inputs.dtype != torch.float64 or tuple(inputs.shape) != (n, D) or not inputs.is_contiguous() or not inputs.is_cuda:
                raise ValueError("log_evidence: inputs must be a contiguous (%d, %d) float64 tensor on the problem's device"
                                 % (n, D))
            if inputs.device.index != problem.device:
                raise ValueError("log_evidence: inputs live on device %s, the problem on device %d"
                                 % (inputs.device.index, problem.device))
            iso = problem.cov_kind == _lib.COV_SE_ISO
            if iso and log_ell is None:
                raise ValueError("log_evidence: Cov_se_iso needs log_ell")
            y = targets.detach().to(torch.float64).contiguous() if targets.is_cuda else None
            # the library works on its own stream: what produced the tensors must be complete before it reads them
            torch.cuda.current_stream(inputs.device).synchronize()
            problem.set_inputs_device(inputs.data_ptr())
            if y is not None:
                problem.set_targets_device(y.data_ptr())
            else:
                problem.set_targets(targets.detach().numpy())
            z = np.asfortranarray(inducing.detach().cpu().numpy().astype(np.float64).T)  # (m, d) tensor -> d x m
            args = dict(log_sf2=float(log_sf2), sigma2=float(np.exp(float(log_sigma2))), inducing=z, variational=variational)
            if iso:
                args["log_ell"] = float(log_ell)
            if tproj is not None:
                args["tproj"] = np.asfortranarray(tproj.detach().cpu().numpy().astype(np.float64))
            need = ctx.needs_input_grad
            ctx.any_grad = any(need)
            if not ctx.any_grad:
                ev = problem.eval(want_grad=False, **args)
                return torch.tensor(ev.l, dtype=torch.float64, device=inputs.device)
            gx = torch.empty((n, D), dtype=torch.float64, device=inputs.device)
            ev, _ = problem.eval_input_grad(out_device_ptr=gx.data_ptr(), **args)
            g = ev.grad
            pos = 0
            g_ell = None
            if iso:
                g_ell, pos = g[0], 1
            g_sf2 = g[pos]
            g_z = g[pos + 1: pos + 1 + d * m].reshape(m, d)  # ind-major: one row per inducing point
            g_tp = g[pos + 1 + d * m: pos + 1 + d * m + D * d].reshape(D, d) if tproj is not None else None  # big-major
            sigma2 = args["sigma2"]
            dev = inputs.device

            def t(v):
                return None if v is None else torch.as_tensor(np.array(v, dtype=np.float64), device=dev)
            ctx.grads = (gx, t(g_sf2), t(ev.dl_dsigma2 * sigma2), t(g_z), t(g_ell), t(g_tp))
            ctx.like = (log_sf2, log_sigma2, inducing, log_ell, tproj)
            return torch.tensor(ev.l, dtype=torch.float64, device=dev)

        @staticmethod
        @once_differentiable  # (the stored gradients are numbers, not a graph: a second derivative raises instead of being zero)
        def backward(ctx, gl):
            gx, g_sf2, g_s2, g_z, g_ell, g_tp = ctx.grads
            need = ctx.needs_input_grad  # (problem, variational, inputs, targets, log_sf2, log_sigma2, inducing, log_ell, tproj)
            like = ctx.like

            def out(i, g, ref):
                if not need[i] or g is None:
                    return None
                return (gl * g).to(device=ref.device, dtype=ref.dtype).reshape(ref.shape)
            return (None, None, gl * gx if need[2] else None, None,  # targets: no gradient is returned
                    out(4, g_sf2, like[0]), out(5, g_s2, like[1]), out(6, g_z, like[2]), out(7, g_ell, like[3]),
                    out(8, g_tp, like[4]))

    _fn = _LogEvidence
    return _fn


def log_evidence(problem, inputs, targets, *, log_sf2, log_sigma2, inducing, log_ell=None, tproj=None, variational=False):
    """The FITC (or variational) log evidence l of `problem` (a gpr_amd.Problem, fp64) as a 0-d float64 tensor.

    inputs     (n, D) contiguous float64 tensor on the problem's device; handed to the library by address
    targets    (n,) tensor (device or host).  NO gradient flows back to the targets: backward returns None for them
    log_sf2, log_sigma2, log_ell   0-d tensors (or floats); sigma2 = exp(log_sigma2), so the gradient is dl/dsigma2 * sigma2
    inducing   (m, d) tensor, one inducing point per row;  tproj (D, d) tensor (Cov_se_fat)

    Backward gives gradients for inputs, log_sf2, log_ell, log_sigma2, inducing and tproj, the hyper-parameter ones cut from
    the library's gradient vector (the reference's Hyper.get_all order).  One gradient evaluation runs in forward when any
    argument requires grad; otherwise forward is an evidence-only evaluation."""
    import torch

    def as_t(v):
        return v if (v is None or isinstance(v, torch.Tensor)) else torch.tensor(float(v), dtype=torch.float64)
    return _function().apply(problem, bool(variational), inputs, targets, as_t(log_sf2), as_t(log_sigma2), inducing,
                             as_t(log_ell), tproj)


_predict_fn = None


def _predict_function():
    """The torch.autograd.Function of `predict`, made at first use."""
    global _predict_fn
    if _predict_fn is not None:
        return _predict_fn
    import torch
    from torch.autograd.function import once_differentiable

    class _Predict(torch.autograd.Function):
        @staticmethod
        def forward(ctx, problem, predictive, x):
            D = problem.D
            if x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D or not x.is_contiguous() or not x.is_cuda:
                raise ValueError("predict: test_inputs must be a contiguous (nt, %d) float64 tensor on the problem's device" % D)
            if x.device.index != problem.device:
                raise ValueError("predict: test_inputs live on device %s, the problem on device %d"
                                 % (x.device.index, problem.device))
            nt = int(x.shape[0])
            mean = torch.empty(nt, dtype=torch.float64, device=x.device)
            var = torch.empty(nt, dtype=torch.float64, device=x.device)
            ptrs = {"means": mean.data_ptr(), "variances": var.data_ptr()}
            need = ctx.needs_input_grad[2]
            if need:
                dm = torch.empty((nt, D), dtype=torch.float64, device=x.device)
                dv = torch.empty((nt, D), dtype=torch.float64, device=x.device)
                ptrs.update(dmeans=dm.data_ptr(), dvariances=dv.data_ptr())
                ctx.grads = (dm, dv)
            # the library works on its own stream: what produced the tensor must be complete before it reads it (its own
            # outputs are complete when the call returns)
            torch.cuda.current_stream(x.device).synchronize()
            problem.predict_input_grad(x.data_ptr(), predictive=predictive, want=tuple(ptrs), out_device_ptrs=ptrs, nt=nt)
            return mean, var

        @staticmethod
        @once_differentiable  # (the stored gradients are numbers, not a graph: a second derivative raises instead of being zero)
        def backward(ctx, g_mean, g_var):
            if not ctx.needs_input_grad[2]:
                return None, None, None
            dm, dv = ctx.grads
            return None, None, g_mean[:, None] * dm + g_var[:, None] * dv

    _predict_fn = _Predict
    return _predict_fn


def predict(problem, test_inputs, predictive=True):
    """(mean, var): the predictive means and variances of `problem`'s current model state (a gpr_amd.Problem, fp64, after an
    evaluation or `load_predictor`) at `test_inputs`, an (nt, D) contiguous float64 tensor on the problem's device, as (nt,)
    float64 tensors.  One library call runs in forward; backward returns g_mean[:, None] * dmeans + g_var[:, None] * dvariances.
    predictive=True adds sigma2 to the variances (not to the gradients)."""
    return _predict_function().apply(problem, bool(predictive), test_inputs)


_acquire_fn = None
_MAX_VALUE = object()  # the `kind` of acquire_max_value inside _Acquire: Problem.acquire_max_value instead of Problem.acquire


def _acquire_function():
    """The torch.autograd.Function of `acquire`, made at first use."""
    global _acquire_fn
    if _acquire_fn is not None:
        return _acquire_fn
    import torch
    from torch.autograd.function import once_differentiable

    class _Acquire(torch.autograd.Function):
        @staticmethod
        def forward(ctx, problem, kind, kw, x):
            D = problem.D
            if x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D or not x.is_contiguous() or not x.is_cuda:
                raise ValueError("acquire: test_inputs must be a contiguous (nt, %d) float64 tensor on the problem's device" % D)
            if x.device.index != problem.device:
                raise ValueError("acquire: test_inputs live on device %s, the problem on device %d"
                                 % (x.device.index, problem.device))
            nt = int(x.shape[0])
            values = torch.empty(nt, dtype=torch.float64, device=x.device)
            ptrs = {"values": values.data_ptr()}
            if ctx.needs_input_grad[3]:
                ctx.dvalues = torch.empty((nt, D), dtype=torch.float64, device=x.device)
                ptrs["dvalues"] = ctx.dvalues.data_ptr()
            # the library works on its own stream: what produced the tensor must be complete before it reads it (its own
            # outputs are complete when the call returns)
            torch.cuda.current_stream(x.device).synchronize()
            if kind is _MAX_VALUE:
                problem.acquire_max_value(x.data_ptr(), want=tuple(ptrs), out_device_ptrs=ptrs, nt=nt, **kw)
            else:
                problem.acquire(x.data_ptr(), kind, want=tuple(ptrs), out_device_ptrs=ptrs, nt=nt, **kw)
            return values

        @staticmethod
        @once_differentiable  # (the stored gradient is numbers, not a graph: a second derivative raises instead of being zero)
        def backward(ctx, g):
            if not ctx.needs_input_grad[3]:
                return None, None, None, None
            return None, None, None, g[:, None] * ctx.dvalues

    _acquire_fn = _Acquire
    return _acquire_fn


def acquire(problem, test_inputs, kind, **kw):
    """The acquisition criterion `kind` ("ei" | "log_ei" | "pi" | "bound") of `problem`'s current model state at `test_inputs`,
    an (nt, D) contiguous float64 tensor on the problem's device, as an (nt,) float64 tensor; every criterion is "larger is
    better".  kw: maximise (required), best, xi, kappa, var_floor, predictive -- those of Problem.acquire.  One library call
    runs in forward; backward returns g[:, None] * dvalues."""
    extra = set(kw) - {"maximise", "best", "xi", "kappa", "var_floor", "predictive"}
    if extra:
        raise TypeError("acquire: unknown arguments %s" % sorted(extra))
    return _acquire_function().apply(problem, kind, dict(kw), test_inputs)


def acquire_max_value(problem, test_inputs, extremes, **kw):
    """Max-value entropy search (Problem.acquire_max_value) of `problem`'s current model state at `test_inputs`, an (nt, D)
    contiguous float64 tensor on the problem's device, as an (nt,) float64 tensor ("larger is better").  extremes: the extreme
    values of 1 .. 64 drawn paths (host numbers: they are constants of the graph); kw: maximise (required), var_floor.  One
    library call runs in forward; backward returns g[:, None] * dvalues."""
    extra = set(kw) - {"maximise", "var_floor"}
    if extra:
        raise TypeError("acquire_max_value: unknown arguments %s" % sorted(extra))
    return _acquire_function().apply(problem, _MAX_VALUE, dict(kw, extremes=extremes), test_inputs)
