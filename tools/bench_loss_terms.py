#!/usr/bin/env python
"""What the composed loss path costs, and what it saves over torch ops.

B=8, 256x512, 4 levels, config.yml's loss weights, bayesian error term, no
pooling, seeded uniform images and predictions (channels-last, as the model's
are).  One step = TukraUncertaintyLoss forward + the backward of disp_loss +
error_loss down to the four predictions.  Three legs, launched eagerly (how a
user who changes the objective runs them), timed with device events around
``--iters`` steps, alternated a, b, c, a, b, c, ... ``--repeats`` times (>= 3)
after a warm-up of every leg:

  a  composed   a recon without reconstruct_pyramid's tag (clones of it): the
                reference's per-level loop over the standalone HIP terms
                (um_image_error_k, um_consistency_*, um_smoothness_*, um_nll_*,
                um_warp_bwd for the recon's path to the disparities)
  b  torch ops  the same composition from torch ops on the device in f32:
                oracle.loss.total_loss (what the reference's code amounts to
                under PyTorch-ROCm)
  c  fused      the tagged recon: um_loss_fwd + um_loss_bwd (for context)

Prints ONE JSON line (and writes it to ``--out`` when given): per leg the
ms/step of every repeat, median and minimum, the loss values, the launch
count of one composed step, and whether a was faster than b in every repeat.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'uncertainty-model_amd'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--iters', type=int, default=200, help='timed steps per leg and repeat')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error('--repeats must be at least 3')

    import torch
    import yaml

    import train.utils as u
    from oracle import loss as OL
    from train.loss import TukraUncertaintyLoss
    from umamd import _lib, lossfn, lossterms

    assert torch.cuda.is_available(), 'needs a GPU'
    B, H, W = args.batch, args.height, args.width
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)['loss']
    cfg['error_loss_config']['loss_type'] = 'bayesian'
    cfg['error_loss_config']['pooling'] = False
    g = torch.Generator().manual_seed(7)
    imgs = torch.rand(B, 6, H, W, generator=g).cuda()
    preds = [(0.02 + 0.2 * torch.rand(B, 4, H >> i, W >> i, generator=g)).cuda()
             .contiguous(memory_format=torch.channels_last).requires_grad_(True)
             for i in range(4)]
    pyr = u.scale_pyramid(imgs, 4)
    lf = TukraUncertaintyLoss(**cfg)

    def composed():
        rec = [r.clone() for r in u.reconstruct_pyramid(preds, pyr)]
        dl, el = lf(pyr, preds, rec, 0, None)
        (dl + el).backward()
        return dl, el

    def torch_ops():
        dl, el, _ = OL.total_loss(pyr, preds, OL.reconstruct_pyramid(preds, pyr), cfg)
        (dl + el).backward()
        return dl, el

    def fused():
        with lossfn.deferred_recon():
            rec = u.reconstruct_pyramid(preds, pyr)
        dl, el = lf(pyr, preds, rec, 0, None)
        (dl + el).backward()
        return dl, el

    legs = {'a': composed, 'b': torch_ops, 'c': fused}

    def run(step):
        for p in preds:
            p.grad = None
        return step()

    def timed(step, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run(step)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    # the C-ABI entries one composed step goes through
    names = []
    real = _lib.call

    def counting(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    lossfn.call = lossterms.call = counting
    run(composed)
    lossfn.call = lossterms.call = real
    torch.cuda.synchronize()

    values = {}
    for k, step in legs.items():
        timed(step, args.warmup)
        dl, el = run(step)
        values[k] = (float(dl.detach()), float(el.detach()))
    ms = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, step in legs.items():
            ms[k].append(timed(step, args.iters))
    out = {'bench': 'loss_terms', 'shape': [B, H, W], 'levels': 4, 'loss_type': 'bayesian',
           'pooling': False, 'iters': args.iters, 'repeats': args.repeats,
           'timing': 'HIP events around eager steps (forward + backward)',
           'legs': {'a': 'composed HIP terms', 'b': 'torch ops (oracle.loss.total_loss, f32)',
                    'c': 'fused (um_loss_fwd + um_loss_bwd)'},
           'device': torch.cuda.get_device_name(0),
           'a_entry_calls': len(names),
           'a_entries': {n: names.count(n) for n in sorted(set(names))}}
    for k in legs:
        out[f'{k}_ms'] = [round(v, 4) for v in ms[k]]
        out[f'{k}_median_ms'] = round(statistics.median(ms[k]), 4)
        out[f'{k}_min_ms'] = round(min(ms[k]), 4)
        out[f'{k}_disp_loss'], out[f'{k}_error_loss'] = values[k]
    out['a_faster_than_b_every_repeat'] = all(a < b for a, b in zip(ms['a'], ms['b']))
    out['b_over_a'] = round(out['b_median_ms'] / out['a_median_ms'], 2)
    out['a_over_c'] = round(out['a_median_ms'] / out['c_median_ms'], 2)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
