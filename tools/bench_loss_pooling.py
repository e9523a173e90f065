#!/usr/bin/env python
"""Cost of ``error_loss_config['pooling'] = True`` in the fused loss.

B=8, 256x512, 4 levels, bayesian, error consistency weight 0.5, error
smoothness weight 0 (config.yml's error-loss block with the flag turned on),
seeded uniform images and predictions.  One step = the loss forward with
gradient partials (under ``deferred_recon``, as train_step runs it) + the
backward of disp_loss + error_loss.  Each leg's step is captured once as a
HIP graph (how the training step runs it: the kernels back to back, no host
launch time) and ``--iters`` replays are timed between two HIP events; the
same steps launched eagerly are timed too (``*_eager_ms``: at this size the
eager numbers are host launch time, 0.2-0.4 ms whatever the kernels do).
Three legs in one process, alternated a, b, c, a, b, c, ... ``--repeats``
times (>= 3):

  a  pooling=False                       um_loss_fwd + um_loss_bwd
  b  pooling=True                        um_loss_pool_fwd + um_loss_pool_bwd
  c  what a user could do without (b):   pooling=False with
     predictive_error_weight=0, plus the pooled error term composed on the
     device from torch ops (avg_pool2d, the NLL) and umamd.lossfn.reconstruct
     (the consistency warp), its error maps from um_image_error of the
     loss's own reconstruction.  reconstruct() has no gradient w.r.t. its
     sampled operand, so leg c leaves that gradient out: it does less than
     leg b.

Prints ONE JSON line: per leg the graph-replay ms/step of every repeat, their
median and minimum, the eager numbers likewise; b - a; and whether b was
faster than c in every repeat (replayed and eager).
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
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30, help='timed steps per leg and repeat')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error('--repeats must be at least 3')

    import torch
    import torch.nn.functional as F

    import train.utils as u
    from train.loss import TukraUncertaintyLoss
    from umamd import lossfn as LF

    assert torch.cuda.is_available(), 'needs a GPU'
    B, H, W = args.batch, args.height, args.width
    g = torch.Generator().manual_seed(7)
    imgs = torch.rand(B, 6, H, W, generator=g).cuda()
    preds = [(0.02 + 0.2 * torch.rand(B, 4, H >> i, W >> i, generator=g)).cuda()
             .contiguous(memory_format=torch.channels_last).requires_grad_(True)
             for i in range(4)]
    pyr = u.scale_pyramid(imgs, 4)
    ecw, alpha = 0.5, 0.85

    def loss_fn(pooling, w_err=1.0):
        return TukraUncertaintyLoss(
            predictive_error_weight=w_err, wssim_alpha=alpha,
            error_loss_config={'loss_type': 'bayesian', 'smoothness_weight': 0.0,
                               'consistency_weight': ecw, 'pooling': pooling})
    lf_a, lf_b, lf_c = loss_fn(False), loss_fn(True), loss_fn(False, 0.0)

    def fused(lf):
        def step():
            with LF.deferred_recon():
                rec = u.reconstruct_pyramid(preds, pyr)
            dl, el = lf(pyr, preds, rec, 0, None)
            (dl + el).backward()
            return dl, el
        return step

    def composed():
        with LF.deferred_recon():
            rec = u.reconstruct_pyramid(preds, pyr)
        dl, _ = lf_c(pyr, preds, rec, 0, None)
        el = 0.0
        for p, im, r in zip(preds, pyr, rec):
            err = LF.image_error(im, r.detach(), alpha)
            pp, pe = F.avg_pool2d(p, 3, 1), F.avg_pool2d(err, 3, 1)
            disp, unc = pp[:, 0:2].detach(), pp[:, 2:4]
            nll = (pe / unc + torch.log(unc)).mean()
            sl, sr = unc[:, 0:1], unc[:, 1:2]
            cons = (sl - LF.reconstruct(sl, disp[:, 1:2], -1.0)).abs().mean() + \
                (sr - LF.reconstruct(sr, disp[:, 0:1], 1.0)).abs().mean()
            el = el + nll + ecw * cons
        (dl + el).backward()
        return dl, el

    legs = {'a': fused(lf_a), 'b': fused(lf_b), 'c': composed}

    def timed(run, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def eager(step):
        def run():
            for p in preds:
                p.grad = None
            step()
        return run

    def capture(step):
        """the step as one HIP graph (warmed up on a side stream first)"""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(args.warmup):
                for p in preds:
                    p.grad = None
                step()
        torch.cuda.current_stream().wait_stream(side)
        for p in preds:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            losses = step()
        return graph, losses

    values, graphs = {}, {}
    for k, step in legs.items():
        graphs[k], losses = capture(step)
        graphs[k].replay()
        torch.cuda.synchronize()
        values[k] = (float(losses[0].detach()), float(losses[1].detach()))
        timed(graphs[k].replay, args.warmup)
        timed(eager(step), args.warmup)
    ms = {k: [] for k in legs}
    ms_eager = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k in legs:
            ms[k].append(timed(graphs[k].replay, args.iters))
    for _ in range(args.repeats):
        for k, step in legs.items():
            ms_eager[k].append(timed(eager(step), args.iters))
    out = {'bench': 'loss_pooling', 'shape': [B, H, W], 'levels': 4, 'loss_type': 'bayesian',
           'ecw': ecw, 'esw': 0.0, 'iters': args.iters, 'repeats': args.repeats,
           'timing': 'HIP events around graph replays (*_eager_ms: eager launches)',
           'device': torch.cuda.get_device_name(0)}
    for k in legs:
        out[f'{k}_ms'] = [round(v, 4) for v in ms[k]]
        out[f'{k}_median_ms'] = round(statistics.median(ms[k]), 4)
        out[f'{k}_min_ms'] = round(min(ms[k]), 4)
        out[f'{k}_disp_loss'], out[f'{k}_error_loss'] = values[k]
        out[f'{k}_eager_ms'] = [round(v, 4) for v in ms_eager[k]]
        out[f'{k}_eager_median_ms'] = round(statistics.median(ms_eager[k]), 4)
    out['b_minus_a_ms'] = round(out['b_median_ms'] - out['a_median_ms'], 4)
    out['b_faster_than_c_every_repeat'] = all(b < c for b, c in zip(ms['b'], ms['c']))
    out['b_faster_than_c_every_repeat_eager'] = all(
        b < c for b, c in zip(ms_eager['b'], ms_eager['c']))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
