"""The loss terms of reference train/loss.py as standalone autograd functions
over the umamd C ABI (csrc/lossterms.hip), one ``torch.autograd.Function``
per term:

  * ``image_error`` / ``wssim``  WeightedSSIMLoss.image_error / .forward
                                 (loss.py:96-151), differentiable w.r.t. both
                                 operands, ``alpha``/``c1``/``c2`` at run time
  * ``consistency``              ConsistencyLoss.forward (loss.py:167-188)
  * ``smoothness``               SmoothnessLoss.forward (loss.py:248-264)
  * ``nll``                      ReprojectionErrorLoss.loss_function
                                 (loss.py:389-403)

Inputs are f32 device tensors (other float dtypes are converted).  Strided
``[N,2,h,w]`` operands (channel slices of a channels-last prediction) are
passed by pointer and strides, without a copy.  Every scalar is reduced on the
device; nothing here synchronises.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._lib import call, ptr, query
from .lossfn import LOSS_TYPES, _f32c


def _ws(N, H, W, dev):
    return torch.empty((query('um_lossterm_ws', N, H, W) // 8,), dtype=torch.float64, device=dev)


def _strided(t: torch.Tensor):
    """(tensor, image stride, channel stride, pixel stride) of a detached f32
    [N,C,h,w] operand whose planes are row-major with one pixel stride (NCHW
    planes and NHWC channel slices qualify; anything else is copied)."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    W = t.shape[-1]
    sn, sc, sy, sx = t.stride()
    if sy != W * sx or sx < 1:
        t = t.contiguous()
        sn, sc, sy, sx = t.stride()
    return t, sn, sc, sx


def _gscalar(g: torch.Tensor) -> torch.Tensor:
    return g.detach().float().contiguous()


def _pair_geom(name, t, channels=2):
    if t.dim() != 4 or t.shape[1] != channels:
        raise L.UmamdError(f'{name}: expected [N,{channels},h,w], got {tuple(t.shape)}')
    return t.shape[0], t.shape[2], t.shape[3]


class _ImageErrorFn(torch.autograd.Function):
    """(map [N,2,H,W], mean(e_L + e_R)); the mean comes from the same launch
    (f64 block partials + finish) when ``with_mean``."""

    @staticmethod
    def forward(ctx, images, recon, alpha, c1, c2, with_mean):
        L.require_device(images)
        L.require_device(recon)
        img, rec = _f32c(images), _f32c(recon)
        N, C, H, W = img.shape
        if C != 6 or rec.shape != img.shape:
            raise L.UmamdError(f'image_error: images {tuple(img.shape)} / recon '
                               f'{tuple(rec.shape)}; expected two [N,6,H,W]')
        out = torch.empty((N, 2, H, W), dtype=torch.float32, device=img.device)
        mean = torch.empty((), dtype=torch.float32, device=img.device)
        ws = _ws(N, H, W, img.device) if with_mean else None
        call('um_image_error_k', ptr(img), ptr(rec), N, H, W, alpha, c1, c2, ptr(out), ptr(ws),
             ptr(mean) if with_mean else None)
        ctx.k = (alpha, c1, c2)
        ctx.meta = (images.dtype, recon.dtype)
        ctx.save_for_backward(img, rec)
        if not with_mean:
            ctx.mark_non_differentiable(mean)
        return out, mean

    @staticmethod
    def backward(ctx, gmap, gmean):
        img, rec = ctx.saved_tensors
        N, _, H, W = img.shape
        alpha, c1, c2 = ctx.k
        # bound until the launches are queued (no temporaries passed by pointer)
        gm = _f32c(gmap) if gmap is not None else None
        gs = _gscalar(gmean) if gmean is not None else None
        grads = [None, None]
        if gm is None and gs is None:
            return None, None, None, None, None, None
        for k, wrt in ((0, 1), (1, 0)):  # input 0 = images (wrt 1), input 1 = recon (wrt 0)
            if not ctx.needs_input_grad[k]:
                continue
            gx = torch.empty_like(img)
            call('um_image_error_bwd', ptr(img), ptr(rec), N, H, W, alpha, c1, c2, wrt, ptr(gm),
                 ptr(gs), ptr(gx))
            grads[k] = gx.to(ctx.meta[k])
        return grads[0], grads[1], None, None, None, None


def check_hw(name, t, least):
    """raised before any launch, in the message style of lossfn.tukra_loss"""
    H, W = t.shape[-2:]
    if H < least or W < least:
        raise ValueError(f'{name}: needs at least {least}x{least} pixels; got {H}x{W}')


def image_error(images, recon, alpha: float, c1: float, c2: float) -> torch.Tensor:
    check_hw('image_error', images, 3)
    return _ImageErrorFn.apply(images, recon, float(alpha), float(c1), float(c2), False)[0]


def wssim(images, recon, alpha: float, c1: float, c2: float):
    """-> (mean(e_L + e_R), error map), both with autograd history"""
    check_hw('wssim', images, 3)
    emap, mean = _ImageErrorFn.apply(images, recon, float(alpha), float(c1), float(c2), True)
    return mean, emap


class _ConsistencyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, images):
        L.require_device(disp)
        N, H, W = _pair_geom('consistency', disp)
        d, dsn, dsc, dsp = _strided(disp)
        if images is None:
            im, isn, isc, isp = d, dsn, dsc, dsp
        else:
            L.require_device(images)
            if images.shape != disp.shape:
                raise L.UmamdError(f'consistency: disp {tuple(disp.shape)} / images '
                                   f'{tuple(images.shape)}')
            im, isn, isc, isp = _strided(images)
        ws = _ws(N, H, W, d.device)
        out = torch.empty((), dtype=torch.float32, device=d.device)
        call('um_consistency_fwd', d.data_ptr(), dsn, dsc, dsp, im.data_ptr(), isn, isc, isp,
             N, H, W, ptr(ws), ptr(out))
        ctx.alias = images is None
        ctx.geom = (N, H, W)
        ctx.views = ((dsn, dsc, dsp), (isn, isc, isp))
        ctx.meta = (disp.dtype, None if images is None else images.dtype)
        ctx.save_for_backward(d, im)
        return out

    @staticmethod
    def backward(ctx, g):
        d, im = ctx.saved_tensors
        N, H, W = ctx.geom
        (dsn, dsc, dsp), (isn, isc, isp) = ctx.views
        need_d = ctx.needs_input_grad[0]
        need_i = ctx.alias or ctx.needs_input_grad[1]
        if not (need_d or need_i):
            return None, None
        gs = _gscalar(g)
        new = lambda: torch.empty((N, 2, H, W), dtype=torch.float32, device=d.device)
        gd = new() if need_d else None
        gi = new() if need_i else None
        scratch = new() if need_i else None
        call('um_consistency_bwd', d.data_ptr(), dsn, dsc, dsp, im.data_ptr(), isn, isc, isp,
             N, H, W, ptr(gs), ptr(gd), ptr(gi), ptr(scratch), 1 if ctx.alias else 0)
        if ctx.alias:  # both parts land on the one tensor: gi = direct + scatter
            return gi.to(ctx.meta[0]), None
        return (gd.to(ctx.meta[0]) if need_d else None,
                gi.to(ctx.meta[1]) if ctx.needs_input_grad[1] else None)


def consistency(disp, images=None) -> torch.Tensor:
    check_hw('consistency', disp, 2)
    return _ConsistencyFn.apply(disp, images)


class _SmoothnessFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, images):
        L.require_device(disp)
        L.require_device(images)
        N, H, W = _pair_geom('smoothness', disp)
        if tuple(images.shape) != (N, 6, H, W):
            raise L.UmamdError(f'smoothness: disp {tuple(disp.shape)} / images '
                               f'{tuple(images.shape)}; expected images [N,6,h,w]')
        d, dsn, dsc, dsp = _strided(disp)
        im = _f32c(images)
        ws = _ws(N, H, W, d.device)
        out = torch.empty((), dtype=torch.float32, device=d.device)
        call('um_smoothness_fwd', d.data_ptr(), dsn, dsc, dsp, ptr(im), N, H, W, ptr(ws), ptr(out))
        ctx.geom = (N, H, W)
        ctx.view = (dsn, dsc, dsp)
        ctx.dtype = disp.dtype
        ctx.save_for_backward(d, im)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError(_SMOOTH_IMG_GRAD)
        d, im = ctx.saved_tensors
        N, H, W = ctx.geom
        gs = _gscalar(g)
        gd = torch.empty((N, 2, H, W), dtype=torch.float32, device=d.device)
        call('um_smoothness_bwd', d.data_ptr(), *ctx.view, ptr(im), N, H, W, ptr(gs), ptr(gd))
        return gd.to(ctx.dtype), None


_SMOOTH_IMG_GRAD = ('umamd SmoothnessLoss: the gradient w.r.t. `images` (the edge weights; data '
                    'at every reference call site) is not implemented; detach `images`')


def smoothness(disp, images) -> torch.Tensor:
    check_hw('smoothness', disp, 2)
    if torch.is_grad_enabled() and images.requires_grad:
        raise NotImplementedError(_SMOOTH_IMG_GRAD)
    return _SmoothnessFn.apply(disp, images)


class _NllFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, unc, err, loss_type):
        L.require_device(unc)
        L.require_device(err)
        N, H, W = _pair_geom('nll', unc)
        if err.shape != unc.shape:
            raise L.UmamdError(f'nll: uncertainty {tuple(unc.shape)} / error {tuple(err.shape)}')
        u, usn, usc, usp = _strided(unc)
        e, esn, esc, esp = _strided(err)
        ws = _ws(N, H, W, u.device)
        out = torch.empty((), dtype=torch.float32, device=u.device)
        call('um_nll_fwd', u.data_ptr(), usn, usc, usp, e.data_ptr(), esn, esc, esp, N, H, W,
             loss_type, ptr(ws), ptr(out))
        ctx.geom = (N, H, W)
        ctx.views = ((usn, usc, usp), (esn, esc, esp))
        ctx.loss_type = loss_type
        ctx.dtype = unc.dtype
        ctx.save_for_backward(u, e)
        return out

    @staticmethod
    def backward(ctx, g):
        u, e = ctx.saved_tensors
        N, H, W = ctx.geom
        gs = _gscalar(g)
        gu = torch.empty((N, 2, H, W), dtype=torch.float32, device=u.device)
        call('um_nll_bwd', u.data_ptr(), *ctx.views[0], e.data_ptr(), *ctx.views[1], N, H, W,
             ctx.loss_type, ptr(gs), ptr(gu))
        return gu.to(ctx.dtype), None, None


def nll(uncertainty, error, loss_type: str) -> torch.Tensor:
    """The error is detached by definition (reference :418)."""
    return _NllFn.apply(uncertainty, error.detach(), LOSS_TYPES[loss_type])
