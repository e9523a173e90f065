"""Loss functions (reference train/loss.py), HIP-backed.

``TukraUncertaintyLoss.forward`` (reference :512-568) runs the fused umamd
loss stack: ONE forward launch over every scale (the six loss terms, reduced
on the device) and ONE backward launch producing d(total)/d(prediction) for
all four channels of every scale, including the WSSIM term's path through
the warp, both L-R consistency terms (with the scatter into the warped
disparity), the edge-aware smoothness and the reprojection-error NLL.

That fused path is taken when ``recon_pyramid`` is the (tagged) output of
``reconstruct_pyramid(predictions, image_pyramid)``, which is what the
reference's own training loop passes.

The sub-loss modules keep the reference's names, constructor kwargs and
attributes (``loss.wssim.previous_image_error``,
``loss.predictive_error.loss_type``...) and each has a standalone,
differentiable ``forward`` on its own HIP kernels (umamd.lossterms), so they
compose as the reference's do; ``TukraUncertaintyLoss.forward`` with any other
recon runs the reference's per-level loop over them.
"""
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor
from torch.nn import Module
from torch.nn.parallel import DistributedDataParallel

from umamd import discfn as DF
from umamd import lossfn as LF
from umamd import lossterms as LT
from umamd import packer as P

from .utils import ImagePyramid


class WeightedSSIMLoss(nn.Module):
    """SSIM/L1 photometric error (reference :15-151).  ``image_error`` and
    ``forward`` are HIP kernels (um_image_error_k / _bwd) with ``alpha``,
    ``k1``, ``k2`` at run time, differentiable w.r.t. both arguments."""

    def __init__(self, alpha: float = 0.85, k1: float = 0.01, k2: float = 0.03) -> None:
        super().__init__()
        self.alpha = alpha
        self.k1 = k1 ** 2
        self.k2 = k2 ** 2
        self.pool = nn.AvgPool2d(kernel_size=3, stride=1)
        self._previous_image_error = None

    @property
    def previous_image_error(self) -> Tensor:
        """Error map [B,2,h,w] of the last scale evaluated (reference :38-41)."""
        return self._previous_image_error

    # ssim, dssim, l1_error: torch ops on the device (on no hot path)
    def ssim(self, x: Tensor, y: Tensor) -> Tensor:
        """Per-pixel SSIM on the 3x3-pooled grid [N,C,H-2,W-2] (reference :43-74)."""
        mx, my = self.pool(x), self.pool(y)
        vx = self.pool(x * x) - mx * mx
        vy = self.pool(y * y) - my * my
        vxy = self.pool(x * y) - mx * my
        return ((2 * mx * my + self.k1) * (2 * vxy + self.k2)) / \
            ((mx * mx + my * my + self.k1) * (vx + vy + self.k2))

    def dssim(self, x: Tensor, y: Tensor) -> Tensor:
        """clamp((1 - SSIM) / 2, 0, 1) (reference :76-90)."""
        return torch.clamp((1 - self.ssim(x, y)) / 2, 0, 1)

    def l1_error(self, x: Tensor, y: Tensor) -> Tensor:
        return (x - y).abs()

    def image_error(self, images: Tensor, recon: Tensor) -> Tensor:
        """Per-pixel alpha*DSSIM(upsampled) + (1-alpha)*L1, channel mean per
        view -> [B,2,H,W] (reference :96-131).  Without a gradient to record
        and with the default constants this stays the evaluation entry
        (um_image_error): no autograd function in the evaluation loop, and the
        bits evaluation has always reported.  The two entries are separate
        kernels with the same arithmetic written down; the compiler fuses
        their multiply-adds differently, so their maps differ in the last bit
        or two (up to 6e-7 on maps up to 0.25)."""
        LT.check_hw('WeightedSSIMLoss.image_error', images, 3)
        grad = torch.is_grad_enabled() and (images.requires_grad or recon.requires_grad)
        if not grad and (self.k1, self.k2) == (0.01 ** 2, 0.03 ** 2):
            return LF.image_error(images, recon, self.alpha)
        return LT.image_error(images, recon, self.alpha, self.k1, self.k2)

    def forward(self, images: Tensor, recon: Tensor) -> Tensor:
        """mean(e_L + e_R) (reference :133-151); ``previous_image_error`` keeps
        the map with its autograd history."""
        loss, error = LT.wssim(images, recon, self.alpha, self.k1, self.k2)
        self._previous_image_error = error
        return loss


class ConsistencyLoss(nn.Module):
    """L-R consistency (reference :154-188): um_consistency_fwd / _bwd."""

    def forward(self, disp: Tensor, images: Optional[Tensor] = None) -> Tensor:
        return LT.consistency(disp, images)


class SmoothnessLoss(nn.Module):
    """Edge-aware smoothness (reference :191-264): um_smoothness_fwd / _bwd.
    Differentiable w.r.t. ``disp``; ``images`` is data."""

    def forward(self, disp: Tensor, images: Tensor) -> Tensor:
        return LT.smoothness(disp, images)


def _disc_module(disc: Module) -> Module:
    # discriminator methods are reached through .module under DDP (reference :294-299)
    return disc.module if isinstance(disc, DistributedDataParallel) else disc


class PerceptualLoss(nn.Module):
    """Discriminator feature reconstruction L1 (reference :267-305): sum over
    the discriminator stages of mean |features(image) - features(recon)|,
    on the NHWC feature maps (one fused L1 launch per stage)."""

    def forward(self, image_pyramid: ImagePyramid, recon_pyramid: ImagePyramid,
                disc: Module) -> Tensor:
        d = _disc_module(disc)
        with P.scope(d._packer):
            image_maps = d._features(image_pyramid)
            recon_maps = d._features(recon_pyramid)
        perceptual_loss = 0
        for image_map, recon_map in zip(image_maps, recon_maps):
            perceptual_loss = perceptual_loss + DF.l1_mean(image_map, recon_map)
        return perceptual_loss


class GeneratorLoss(nn.Module):
    """Loss of failing to convince the discriminator (reference :308-337):
    ``self.adversarial`` (MSE or BCE) of the discriminator's predictions on
    the reconstructions against ones.  With exactly nn.MSELoss / nn.BCELoss
    (mean reduction, no weight) on device predictions the loss and its
    gradient are one um_label_loss launch each and the ones tensor is never
    made; any other ``adversarial`` module takes the ATen path."""

    def __init__(self, loss: str = 'mse') -> None:
        super().__init__()
        self.adversarial = nn.MSELoss() if loss == 'mse' else nn.BCELoss()

    def forward(self, recon_pyramid: ImagePyramid, discriminator: Module) -> Tensor:
        predictions = discriminator(recon_pyramid)
        kind = DF.label_loss_kind(self.adversarial)
        if kind is not None and predictions.is_cuda:
            return DF.label_loss(predictions, kind, predictions.numel())
        labels = torch.ones_like(predictions)
        return self.adversarial(predictions, labels)


class ReprojectionErrorLoss(nn.Module):
    """Uncertainty loss (reference :340-434).  ``forward``: the NLL
    (um_nll_fwd / _bwd), the smoothness and the consistency of the uncertainty
    on the HIP terms; ``self.pool``, the channel split and the scalar
    arithmetic are ATen."""

    def __init__(self, loss_type: str = 'l1', smoothness_weight: float = 1.0,
                 consistency_weight: float = 1.0, pooling: bool = False) -> None:
        super().__init__()
        if loss_type not in ('l1', 'bayesian', 'log_bayesian'):
            raise ValueError('Loss must be either "l1", "bayesian" or "log_bayesian".')
        self.loss_type = loss_type
        self.smoothness_weight = smoothness_weight
        self.consistency_weight = consistency_weight
        self.smoothness = SmoothnessLoss() if smoothness_weight > 0 else None
        self.consistency = ConsistencyLoss() if consistency_weight > 0 else None
        # pooling (reference :405-434): every level's prediction, image and
        # error map are 3x3 average-pooled before the error term; evaluated
        # by the pooled stage of the fused loss (um_loss_pool_fwd / _bwd)
        self.pool = nn.AvgPool2d(kernel_size=3, stride=1) if pooling else nn.Identity()

    def loss_function(self, predicted: Tensor, error: Tensor) -> Tensor:
        """l1 / bayesian / log_bayesian of (uncertainty, error) (reference :389-403)."""
        return LT.nll(predicted, error, self.loss_type)

    def forward(self, predicted: Tensor, image: Tensor, error: Tensor) -> Tensor:
        """Reference :405-434 (F5: the consistency takes the uncertainty as
        the compared map and the shift, the disparity as the sampled image)."""
        if isinstance(self.pool, nn.AvgPool2d):
            h, w = predicted.shape[-2:]
            if h < 4 or w < 4:
                raise ValueError(f'ReprojectionErrorLoss: pooling=True needs a level of at least '
                                 f'4x4; got {h}x{w}')
        error = error.detach()
        predicted, image, error = self.pool(predicted), self.pool(image), self.pool(error)
        disparity, uncertainty = torch.split(predicted, [2, 2], dim=1)
        loss = self.loss_function(uncertainty, error)
        if self.smoothness_weight > 0:
            loss = loss + self.smoothness(uncertainty, image) * self.smoothness_weight
        if self.consistency_weight > 0:
            loss = loss + self.consistency(uncertainty, disparity) * self.consistency_weight
        return loss


class TukraUncertaintyLoss(nn.Module):
    """Total loss of the uncertainty model (reference :437-568)."""

    def __init__(self, wssim_weight: float = 1.0, consistency_weight: float = 1.0,
                 smoothness_weight: float = 1.0, adversarial_weight: float = 0.85,
                 predictive_error_weight: float = 1.0, perceptual_weight: float = 0.05,
                 wssim_alpha: float = 0.85, perceptual_start: int = 5,
                 adversarial_loss_type: str = 'mse',
                 error_loss_config: Optional[dict] = None) -> None:
        super().__init__()
        self.wssim = WeightedSSIMLoss(wssim_alpha)
        self.consistency = ConsistencyLoss()
        self.smoothness = SmoothnessLoss()
        self.adversarial = GeneratorLoss(adversarial_loss_type)
        self.perceptual = PerceptualLoss()
        self.predictive_error = ReprojectionErrorLoss(**(error_loss_config or {}))
        self.perceptual_start = perceptual_start
        self.wssim_weight = wssim_weight
        self.consistency_weight = consistency_weight
        self.smoothness_weight = smoothness_weight
        self.adversarial_weight = adversarial_weight
        self.perceptual_weight = perceptual_weight
        self.predictive_error_weight = predictive_error_weight
        self.last_terms: Optional[Tensor] = None

    def _cfg(self):
        pe = self.predictive_error
        return {'alpha': float(self.wssim.alpha), 'loss_type': LF.LOSS_TYPES[pe.loss_type],
                'esw': float(pe.smoothness_weight), 'ecw': float(pe.consistency_weight),
                'w_wssim': float(self.wssim_weight), 'w_cons': float(self.consistency_weight),
                'w_smooth': float(self.smoothness_weight),
                'w_err': float(self.predictive_error_weight),
                'pool': isinstance(pe.pool, nn.AvgPool2d)}

    def _composed(self, image_pyramid, predictions, recon_pyramid):
        """The reference's per-level loop (:539-550) over the standalone
        modules, for a recon that is not reconstruct_pyramid's own output (an
        occlusion-masked or blended one...): per level WSSIM 2 launches,
        consistency 2, smoothness 2 and the error term up to 6 forward; the
        gradients reach ``predictions`` and ``recon_pyramid``."""
        wssim = cons = smooth = err = 0
        for i, (images, prediction, recon) in enumerate(zip(image_pyramid, predictions,
                                                            recon_pyramid)):
            disparity = prediction[:, 0:2]
            wssim = wssim + self.wssim(images, recon)
            cons = cons + self.consistency(disparity)
            smooth = smooth + self.smoothness(disparity, images) / (2 ** i)
            err = err + self.predictive_error(prediction, images,
                                              self.wssim.previous_image_error)
        disp_loss = wssim * self.wssim_weight + cons * self.consistency_weight \
            + smooth * self.smoothness_weight
        error_loss = err * self.predictive_error_weight
        terms = torch.stack([t.detach().float() for t in
                             (disp_loss, error_loss, wssim, cons, smooth, err)])
        return disp_loss, error_loss, terms

    def forward(self, image_pyramid: ImagePyramid, predictions: ImagePyramid,
                recon_pyramid: ImagePyramid, epoch: Optional[int] = None,
                discriminator: Optional[Module] = None):
        return self._forward(image_pyramid, predictions, recon_pyramid, epoch, discriminator)

    def _forward(self, image_pyramid: ImagePyramid, predictions: ImagePyramid,
                 recon_pyramid: ImagePyramid, epoch: Optional[int] = None,
                 discriminator: Optional[Module] = None, gate: Optional[Tensor] = None):
        """``forward``; with ``gate`` (a 0-dim device tensor holding 0.0 or
        1.0: train.graph.CapturedTrainStep) the perceptual term is always
        evaluated and multiplied by it instead of being switched by
        ``epoch``, so one captured graph serves both sides of
        ``perceptual_start``.  gate 1.0 leaves the term's value and gradient
        bits unchanged; gate 0.0 makes them exact zeros (finite terms)."""
        pending = [r for r in recon_pyramid if getattr(r, '_umamd_pending', False)]
        if pending and len(pending) != len(recon_pyramid):
            raise ValueError('TukraUncertaintyLoss (umamd): partly deferred recon_pyramid')
        tagged = all(getattr(r, '_umamd_recon', None) == (id(p), id(im))
                     for p, im, r in zip(predictions, image_pyramid, recon_pyramid))
        if tagged:
            # the recon is reconstruct_pyramid(predictions, image_pyramid): the fused
            # kernels re-derive that warp and differentiate through it
            disp_loss, error_loss, terms, emap = LF.tukra_loss(
                self._cfg(), list(predictions), list(image_pyramid),
                list(recon_pyramid) if pending else None)
            self.wssim._previous_image_error = emap
        else:
            if pending:
                raise ValueError('TukraUncertaintyLoss (umamd): a deferred (unwritten) '
                                 'recon_pyramid is only filled by the fused loss of the '
                                 'predictions and images it was made from')
            disp_loss, error_loss, terms = self._composed(image_pyramid, predictions,
                                                          recon_pyramid)
        self.last_terms = terms  # [disp, error, wssim, consistency, smoothness, error-term]
        if discriminator is not None:
            # adversarial terms (reference :552-564); the recon pyramid carries
            # the gradient back to the disparities through the warp adjoint
            adversarial_loss = self.adversarial(recon_pyramid, discriminator)
            disp_loss = disp_loss + adversarial_loss * self.adversarial_weight
            if gate is not None:
                perceptual_loss = self.perceptual(image_pyramid, recon_pyramid, discriminator)
                disp_loss = disp_loss + perceptual_loss * self.perceptual_weight * gate
            elif epoch is not None and epoch >= self.perceptual_start:
                perceptual_loss = self.perceptual(image_pyramid, recon_pyramid, discriminator)
                disp_loss = disp_loss + perceptual_loss * self.perceptual_weight
        return disp_loss, error_loss
