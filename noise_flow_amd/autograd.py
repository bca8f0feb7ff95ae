"""``torch.autograd`` binding of the NLL: ``NoiseFlow.nll_torch``.

The forward pass of a call whose inputs need gradients is ONE ``nf_nll_grad`` launch that returns the NLL together with
d nll_b / d x and d nll_b / d y (patches are independent in evaluation mode); the backward pass is one multiplication by
the incoming gradient.  Without gradients the forward pass is plain ``nf_nll``.  Everything is enqueued on the current stream.
"""
from __future__ import annotations


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
