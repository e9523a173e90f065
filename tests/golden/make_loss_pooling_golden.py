#!/usr/bin/env python3
"""Generate tests/golden/loss_pooling.npz by running the REFERENCE's
TukraUncertaintyLoss with ``error_loss_config['pooling'] = True``.

Run in the build container only (the harness of make_goldens.py: the
reference is imported, nothing of it is stored but the numbers it computes):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_loss_pooling_golden.py

B=2, 32x64, 4 levels (the coarsest level is 4x8: a pooled grid of 2x6), the
"rough" predictions of gen_loss (seed 99).  For each loss type and each
(error smoothness weight, error consistency weight) the two loss scalars and
the gradient of each w.r.t. the four prediction levels (``gdisp{i}``, the
disparity loss's, is identical in all nine cases and stored once).  The
images and the predictions are stored too, so the tests need no generator.
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

LOSS_TYPES = ('l1', 'bayesian', 'log_bayesian')
WEIGHTS = ((0.0, 0.5), (0.3, 0.5), (0.3, 0.0))  # (esw, ecw)


def tag(lt, esw, ecw):
    return f'{lt}_s{esw:g}_c{ecw:g}'


def main():
    _, ref_loss, ref_utils = import_reference()
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)
    b, h, w = 2, 32, 64
    left, right, _ = stereo_pair(b, h, w)
    images = torch.cat([left, right], 1)
    pyr = ref_utils.scale_pyramid(images, 4)
    g = torch.Generator().manual_seed(99)
    preds = [0.3 * torch.rand(p.shape, generator=g).clamp_min(1e-3)
             for p in pred_pyramid(b, h, w, 22)]
    arrays = {'images': images}
    for i, p in enumerate(preds):
        arrays[f'pred{i}'] = p
    for lt in LOSS_TYPES:
        for esw, ecw in WEIGHTS:
            lcfg = json.loads(json.dumps(cfg['loss']))
            lcfg['error_loss_config'] = {'loss_type': lt, 'smoothness_weight': esw,
                                         'consistency_weight': ecw, 'pooling': True}
            lf = ref_loss.TukraUncertaintyLoss(**lcfg)
            ps = [p.clone().requires_grad_(True) for p in preds]
            dl, el = lf(pyr, ps, ref_utils.reconstruct_pyramid(ps, pyr), 0, None)
            gd = torch.autograd.grad(dl, ps, retain_graph=True, allow_unused=True)
            ge = torch.autograd.grad(el, ps, allow_unused=True)
            t = tag(lt, esw, ecw)
            arrays[f'{t}_disp_loss'] = dl.detach()
            arrays[f'{t}_error_loss'] = el.detach()
            for i in range(4):
                z = torch.zeros_like(preds[i])
                gdi = gd[i] if gd[i] is not None else z
                # the disparity loss does not see the error-loss config: its
                # gradient is the same tensor, bit for bit, in all nine cases
                # (checked here) and is stored once
                if f'gdisp{i}' in arrays:
                    assert torch.equal(arrays[f'gdisp{i}'], gdi), (t, i)
                arrays[f'gdisp{i}'] = gdi
                arrays[f'{t}_gerr{i}'] = ge[i] if ge[i] is not None else z
    save('loss_pooling.npz', **arrays)


if __name__ == '__main__':
    main()
