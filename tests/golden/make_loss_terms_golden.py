#!/usr/bin/env python3
"""Generate tests/golden/loss_terms.npz by running the REFERENCE's own loss
modules standalone (train/loss.py: WeightedSSIMLoss, ConsistencyLoss,
SmoothnessLoss, ReprojectionErrorLoss) and one two-level TukraUncertaintyLoss
on a recon that is not reconstruct_pyramid's output.

Run in the build container only (the harness of make_goldens.py: the
reference is imported, nothing of it is stored but the numbers it computes):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_loss_terms_golden.py

B=2, 20x36, f32.  Stored: the inputs (``images``, ``recon`` = a blend of the
reference's reconstruction and the batch-flipped image, ``pred`` [2,4,20,36],
``gmap`` the upstream gradient of the error map, and the second level
``images1``/``recon1``/``pred1`` at 10x18), then per case the value and the
gradients:

  w_a{alpha}_k{k1}_{k2}_{loss,map,gimg,grec}  WeightedSSIMLoss: forward's
      scalar, image_error's map, d(sum(map * gmap))/d(images | recon)
  cons_{self,img}_{loss,gdisp[,gimg]}         ConsistencyLoss(disp[, images])
  smooth_{loss,gdisp}                         SmoothnessLoss
  err_{type}_p{0,1}_{loss,gpred}              ReprojectionErrorLoss, weights
      (0.3, 0.5), pooling off/on, gradient w.r.t. ``predicted``
  tukra_{disp,error,gpred0,gpred1}            TukraUncertaintyLoss(config.yml,
      bayesian), two levels, gradient of disp_loss + error_loss w.r.t. the
      predictions
"""
from __future__ import annotations

import json
import os
import sys

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True

import torch  # noqa: E402
import yaml  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import REPO, import_reference, pred_pyramid, save, stereo_pair  # noqa: E402

WSSIM_PARAMS = ((0.85, 0.01, 0.03), (0.5, 0.02, 0.05))
LOSS_TYPES = ('l1', 'bayesian', 'log_bayesian')
ERR_WEIGHTS = (0.3, 0.5)  # (smoothness, consistency) of the error term


def wtag(alpha, k1, k2):
    return f'w_a{alpha:g}_k{k1:g}_{k2:g}'


def leaf(t):
    return t.clone().requires_grad_(True)


def main():
    _, ref_loss, ref_utils = import_reference()
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)
    b, h, w = 2, 20, 36
    left, right, _ = stereo_pair(b, h, w)
    # 8-bit images (256 distinct values: the stored inputs compress)
    images = torch.round(torch.cat([left, right], 1) * 255) / 255
    pyr = ref_utils.scale_pyramid(images, 2)
    g = torch.Generator().manual_seed(99)
    preds = [0.3 * torch.rand(p.shape, generator=g).clamp_min(1e-3)
             for p in pred_pyramid(b, h, w, 22)[:2]]
    with torch.no_grad():
        recs = [0.7 * r + 0.3 * im.flip(0)
                for r, im in zip(ref_utils.reconstruct_pyramid(preds, pyr), pyr)]
    gmap = torch.rand(b, 2, h, w, generator=g) + 0.1
    arrays = {'images': pyr[0], 'recon': recs[0], 'pred': preds[0], 'gmap': gmap,
              'images1': pyr[1], 'recon1': recs[1], 'pred1': preds[1]}
    images, recon, pred = pyr[0], recs[0], preds[0]

    for alpha, k1, k2 in WSSIM_PARAMS:
        t = wtag(alpha, k1, k2)
        m = ref_loss.WeightedSSIMLoss(alpha, k1, k2)
        arrays[f'{t}_loss'] = m(images, recon).detach()
        im, rc = leaf(images), leaf(recon)
        emap = m.image_error(im, rc)
        gi, gr = torch.autograd.grad((emap * gmap).sum(), (im, rc))
        arrays[f'{t}_map'] = emap.detach()
        arrays[f'{t}_gimg'] = gi
        arrays[f'{t}_grec'] = gr

    cons = ref_loss.ConsistencyLoss()
    d = leaf(pred[:, 0:2])
    loss = cons(d)
    arrays['cons_self_loss'] = loss.detach()
    arrays['cons_self_gdisp'] = torch.autograd.grad(loss, d)[0]
    d, im2 = leaf(pred[:, 2:4]), leaf(pred[:, 0:2])
    loss = cons(d, im2)
    arrays['cons_img_loss'] = loss.detach()
    arrays['cons_img_gdisp'], arrays['cons_img_gimg'] = torch.autograd.grad(loss, (d, im2))

    d = leaf(pred[:, 0:2])
    loss = ref_loss.SmoothnessLoss()(d, images)
    arrays['smooth_loss'] = loss.detach()
    arrays['smooth_gdisp'] = torch.autograd.grad(loss, d)[0]

    err = ref_loss.WeightedSSIMLoss().image_error(images, recon).detach()
    for lt in LOSS_TYPES:
        for pooling in (False, True):
            m = ref_loss.ReprojectionErrorLoss(lt, ERR_WEIGHTS[0], ERR_WEIGHTS[1], pooling)
            p = leaf(pred)
            loss = m(p, images, err)
            arrays[f'err_{lt}_p{int(pooling)}_loss'] = loss.detach()
            arrays[f'err_{lt}_p{int(pooling)}_gpred'] = torch.autograd.grad(loss, p)[0]

    lcfg = json.loads(json.dumps(cfg['loss']))
    lcfg['error_loss_config']['loss_type'] = 'bayesian'
    lf = ref_loss.TukraUncertaintyLoss(**lcfg)
    ps = [leaf(p) for p in preds]
    dl, el = lf(pyr, ps, recs, 0, None)
    grads = torch.autograd.grad(dl + el, ps)
    arrays['tukra_disp'] = dl.detach()
    arrays['tukra_error'] = el.detach()
    for i in range(2):
        arrays[f'tukra_gpred{i}'] = grads[i]
    save('loss_terms.npz', **arrays)


if __name__ == '__main__':
    main()
