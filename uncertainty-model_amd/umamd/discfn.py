"""Autograd functions of the adversarial path over the umamd C ABI
(reference model/discriminator.py:53-86, train/loss.py:267-337).

  * ``image_to_nhwc``  NCHW f32 -> NHWC compute dtype WITH a gradient (the
                       discriminator sees the recon pyramid, whose gradient
                       flows back to the disparities through the warp)
  * ``disc_head``      sigmoid(Linear(flatten(x))) on the last NHWC feature map
  * ``l1_mean``        mean |a - b| of two NHWC feature maps (PerceptualLoss)
  * ``label_loss``     MSELoss / BCELoss of the predictions against step labels
                       that are never materialised (GeneratorLoss: all ones;
                       run_discriminator: ones then zeros)
  * ``image_pair_to_nhwc``  two NCHW images -> one NHWC batch, no gradient
                       (run_discriminator's real + detached recon levels)
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import functional as U
from ._lib import call, ptr, query


class ImageToNHWCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, dtype):
        out = U.image_to_nhwc(img, dtype)
        ctx.shape = img.shape
        ctx.in_dtype = img.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, H, W = ctx.shape
        gc = g.contiguous()
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device)
        call('um_nhwc_to_image', L.dtype_code(gc.dtype), ptr(gc), N, C, H, W, gc.shape[-1],
             ptr(out))
        return out.to(ctx.in_dtype), None


def image_to_nhwc(img: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    if not img.requires_grad:
        return U.image_to_nhwc(img, dtype)
    return ImageToNHWCFn.apply(img, dtype)


def image_pair_to_nhwc(a: torch.Tensor, b: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[N,C,H,W] f32 x 2 -> NHWC [2N,H,W,ceil8(C)] in ``dtype``: what
    ``image_to_nhwc(torch.cat((a, b), 0), dtype)`` gives, without the cat.
    No autograd: the inputs must not require grad (pass ``.detach()``)."""
    L.require_device(a)
    L.require_device(b)
    if a.requires_grad or b.requires_grad:
        raise L.UmamdError('image_pair_to_nhwc has no gradient: detach the inputs')
    if a.shape != b.shape or a.dim() != 4:
        raise L.UmamdError(f'image_pair_to_nhwc: {tuple(a.shape)} vs {tuple(b.shape)}')
    if a.dtype != torch.float32 or not a.is_contiguous():
        a = a.float().contiguous()
    if b.dtype != torch.float32 or not b.is_contiguous():
        b = b.float().contiguous()
    N, C, H, W = a.shape
    Cp = U.ceil8(C)
    out = torch.empty((2 * N, H, W, Cp), dtype=dtype, device=a.device)
    call('um_image_pair_to_nhwc', L.dtype_code(dtype), ptr(a), ptr(b), N, C, H, W, Cp, ptr(out))
    return out


class DiscHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        L.require_device(x)
        N, H, W, C = x.shape
        if weight.numel() != H * W * C:
            raise L.UmamdError(f'disc_head: Linear in_features {weight.numel()} != flattened '
                               f'feature {C}x{H}x{W}')
        xc = x.contiguous()
        w = weight.detach().float().contiguous()
        b = bias.detach().float().contiguous()
        prob = torch.empty((N, 1), dtype=torch.float32, device=x.device)
        call('um_disc_head_fwd', L.dtype_code(xc.dtype), ptr(xc), N, H * W, C, ptr(w), ptr(b),
             ptr(prob))
        ctx.save_for_backward(xc, w, prob)
        return prob

    @staticmethod
    def backward(ctx, dprob):
        xc, w, prob = ctx.saved_tensors
        N, H, W, C = xc.shape
        dp = dprob.float().contiguous()
        dx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        # a frozen head (the adversarial step's discriminator clone): no dw / db
        dw = torch.empty((1, H * W * C), dtype=torch.float32, device=xc.device) \
            if ctx.needs_input_grad[1] else None
        db = torch.empty((1,), dtype=torch.float32, device=xc.device) \
            if ctx.needs_input_grad[2] else None
        if dx is None and dw is None and db is None:
            return None, None, None
        call('um_disc_head_bwd', L.dtype_code(xc.dtype), ptr(xc), N, H * W, C, ptr(w), ptr(prob),
             ptr(dp), ptr(dx), ptr(dw), ptr(db))
        return dx, dw, db


def disc_head(x: torch.Tensor, linear: torch.nn.Linear) -> torch.Tensor:
    return DiscHeadFn.apply(x, linear.weight, linear.bias)


class L1MeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        L.require_device(a)
        if a.shape != b.shape or a.dtype != b.dtype:
            raise L.UmamdError(f'l1_mean: {tuple(a.shape)}/{a.dtype} vs {tuple(b.shape)}/{b.dtype}')
        ac, bc = a.contiguous(), b.contiguous()
        ws = torch.empty((query('um_l1_mean_ws') // 8,), dtype=torch.float64, device=a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        call('um_l1_mean', L.dtype_code(ac.dtype), ptr(ac), ptr(bc), ac.numel(), ptr(ws), ptr(out))
        ctx.save_for_backward(ac, bc)
        return out

    @staticmethod
    def backward(ctx, g):
        ac, bc = ctx.saved_tensors
        gc = g.float().reshape(1).contiguous()
        da = torch.empty_like(ac) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(bc) if ctx.needs_input_grad[1] else None
        call('um_l1_mean_bwd', L.dtype_code(ac.dtype), ptr(ac), ptr(bc), ac.numel(), ptr(gc),
             ptr(da), ptr(db))
        return da, db


def l1_mean(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return L1MeanFn.apply(a, b)


class LabelLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, kind, n_real):
        L.require_device(prob)
        p = prob.detach()
        if p.dtype != torch.float32 or not p.is_contiguous():
            p = p.float().contiguous()
        out = torch.empty((), dtype=torch.float32, device=p.device)
        call('um_label_loss_fwd', kind, ptr(p), p.numel(), n_real, ptr(out))
        ctx.kind, ctx.n_real = kind, n_real
        ctx.in_dtype = prob.dtype
        ctx.save_for_backward(p)
        return out

    @staticmethod
    def backward(ctx, g):
        p, = ctx.saved_tensors
        gc = g.float().reshape(1).contiguous()
        dp = torch.empty_like(p)
        call('um_label_loss_bwd', ctx.kind, ptr(p), p.numel(), ctx.n_real, ptr(gc), ptr(dp))
        return dp.to(ctx.in_dtype), None, None


def label_loss_kind(loss_module):
    """LABEL_MSE / LABEL_BCE when ``loss_module`` is exactly nn.MSELoss or
    nn.BCELoss with reduction='mean' (and no weight), which is what
    um_label_loss computes; None for anything else (a subclass, another
    reduction, a weighted BCE), which keeps the ATen path."""
    if getattr(loss_module, 'reduction', None) != 'mean':
        return None
    if type(loss_module) is torch.nn.MSELoss:
        return L.LABEL_MSE
    if type(loss_module) is torch.nn.BCELoss and loss_module.weight is None:
        return L.LABEL_BCE
    return None


def label_loss(prob: torch.Tensor, kind: int, n_real: int) -> torch.Tensor:
    """mean loss of the probabilities ``prob`` (any shape, read flat) against
    labels 1 for the first ``n_real`` and 0 for the rest"""
    return LabelLossFn.apply(prob, int(kind), int(max(0, min(n_real, prob.numel()))))
