"""``torch.autograd`` bindings: ``NoiseFlow.nll_torch`` (the NLL) and ``NoiseFlow.sample_torch`` (the sampling direction).

The forward pass of a call whose inputs need gradients is ONE ``nf_nll_grad`` launch that returns the NLL together with
d nll_b / d x and d nll_b / d y (patches are independent in evaluation mode); the backward pass is one multiplication by
the incoming gradient.  Without gradients the forward pass is plain ``nf_nll``.  Everything is enqueued on the current stream.

``sample_torch``: the forward pass is plain ``nf_sample`` and saves yy, eps or the Philox key (seed, base), the temperature and
the condition; the backward pass is ONE ``nf_sample_vjp`` launch with ``x_out = NULL`` that turns the incoming d L / d x into
d L / d yy, d L / d eps and d L / d eps_std.
"""
from __future__ import annotations

import ctypes as C

from . import _lib


def _function(torch):
    class _NllFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, model, cond, x, y):
            need_x = ctx.needs_input_grad[2]
            need_y = y is not None and ctx.needs_input_grad[3]
            nll, gx, gy = model._run_nll_grad(x, y, cond, need_x, need_y)
            ctx.save_for_backward(*[g for g in (gx, gy) if g is not None])
            ctx.have = (gx is not None, gy is not None)
            return nll

        @staticmethod
        @torch.autograd.function.once_differentiable   # gx / gy enter as constants: a double backward raises instead of giving zeros
        def backward(ctx, grad_out):
            saved = list(ctx.saved_tensors)
            gx = saved.pop(0) if ctx.have[0] else None
            gy = saved.pop(0) if ctx.have[1] else None
            w = grad_out[:, None, None, None]
            return None, None, (w * gx if gx is not None else None), (w * gy if gy is not None else None)

    return _NllFunction


_FN = None


def nll_torch(model, x, y, nlf0=None, nlf1=None, iso=None, cam=None):
    """``model`` = a :class:`noise_flow_amd.NoiseFlow` in evaluation mode; ``x``, ``y`` CUDA tensors [B, H, W, 4]."""
    global _FN
    torch = model._dev.torch
    if not isinstance(x, torch.Tensor) or (y is not None and not isinstance(y, torch.Tensor)):
        raise TypeError("nll_torch takes torch tensors (use nll_and_grad for numpy arrays)")
    xt, yt, _ = model._grad_inputs(x, y)
    cond = model._cond(nlf0, nlf1, iso, cam, int(xt.shape[0]))
    if not torch.is_grad_enabled() or not (xt.requires_grad or (yt is not None and yt.requires_grad)):
        nll, _, _, _, _, _ = model._run_nll(xt, yt, cond, False)
        return nll
    if _FN is None:
        _FN = _function(torch)
    return _FN.apply(model, cond, xt, yt)


def _sample_function(torch):
    class _SampleFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, model, cond, key, temp, yy, eps, eps_std):
            seed, base, B = key
            ctx.model, ctx.cond, ctx.key, ctx.temp = model, cond, key, temp
            ctx.have = (yy is not None, eps is not None)
            ctx.save_for_backward(*[t for t in (yy, eps) if t is not None])
            dev = model._dev
            x = dev.empty((B,) + tuple(model.x_shape))
            per_patch = not isinstance(cond, _lib.nf_cond)
            rows = model._rows_to_dev(cond, 1) if per_patch else None
            args = (model._flow.ptr, yy.data_ptr() if yy is not None else None, eps.data_ptr() if eps is not None else None,
                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(base), float(temp), B, rows.data_ptr() if per_patch else C.byref(cond), x.data_ptr())
            with torch.cuda.device(dev.device):
                fn = model._flow.lib.nf_sample_percond if per_patch else model._flow.lib.nf_sample
                _lib.check(fn(*args, dev.stream_ptr()))
            return x

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients enter as constants: a double backward raises instead of giving zeros
        def backward(ctx, gx):
            saved = list(ctx.saved_tensors)
            yy = saved.pop(0) if ctx.have[0] else None
            eps = saved.pop(0) if ctx.have[1] else None
            need_y = yy is not None and ctx.needs_input_grad[4]
            need_e = eps is not None and ctx.needs_input_grad[5]
            need_t = ctx.needs_input_grad[6]
            seed, base, _ = ctx.key
            _, gy, geps, gtemp = ctx.model._run_sample_vjp(yy, eps, seed, base, ctx.temp, ctx.cond, gx.contiguous().float(), False,
                                                           need_y, need_e, need_t)
            return None, None, None, None, gy, geps, (gtemp.sum() if need_t else None)

    return _SampleFunction


_SFN = None


def sample_torch(model, yy, eps=None, seed=None, eps_std=None, nlf0=None, nlf1=None, iso=None, cam=None):
    """``model`` = a :class:`noise_flow_amd.NoiseFlow` in evaluation mode; ``yy`` a CUDA tensor [B, H, W, 4]; ``eps`` None (the
    in-kernel draw of ``model.sample`` under ``seed``) or a CUDA tensor; ``eps_std`` None (1), a number or a 0-d tensor."""
    global _SFN
    torch = model._dev.torch
    if not isinstance(yy, torch.Tensor) or (eps is not None and not isinstance(eps, torch.Tensor)):
        raise TypeError("sample_torch takes torch tensors (use sample_and_vjp for numpy arrays)")
    t_std = eps_std if isinstance(eps_std, torch.Tensor) else None
    if t_std is not None and t_std.dim() != 0:
        raise ValueError("sample_torch takes one temperature per call: eps_std must be a number or a 0-d tensor")
    temp = 1.0 if eps_std is None else float(eps_std)
    yt, epst, sd, base, B, _ = model._sample_vjp_inputs(yy, yy, eps, seed)
    cond = model._cond(nlf0, nlf1, iso, cam, B)
    if _SFN is None:
        _SFN = _sample_function(torch)
    # (apply builds no graph when grad mode is off or nothing requires grad)
    return _SFN.apply(model, cond, (sd, base, B), temp, yt, epst, t_std)
