#!/usr/bin/env python
"""Throughput of the adversarial training step (BASELINE config 3: B=8,
256x512, bf16, bayesian, config.yml's discriminator), captured against eager.

Two legs in one process, alternated ``--repeats`` times (default 2):

  captured  train.train._GraphSteps with a discriminator (three HIP graphs
            per step, train.graph.CapturedTrainStep)
  eager     train.train.train_step with UMAMD_ADV_GRAPH=0 semantics: the same
            kernels launched from Python

Both step past ``perceptual_start`` (generator + perceptual terms on) and
refresh the discriminator clone in place every 10 steps, as the loop does.
Inputs: seeded uniform pairs (torch.Generator seed 7).  Every leg is warmed
up (the captured leg's construction + replays, eager steps), timed over
``--steps`` (>= 20) steps and ends in a synchronise.  Both legs start from
the same weights each time.

Prints ONE JSON line: pairs/s and ms/step per leg (mean over the repeats and
each repeat), the relative spread between repeats, and captured / eager.
"""
import argparse
import json
import os
import time
from copy import deepcopy

import _bench
from _bench import REPO


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=30, help='timed steps per leg (>= 20)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    args = ap.parse_args()
    if args.steps < 20:
        ap.error('--steps must be at least 20')

    import torch

    import model as M
    from train.loss import TukraUncertaintyLoss
    from train.train import _GraphSteps, train_step
    from umamd.optim import Adam

    m, cfg, g = _bench.build_model(args.dtype)  # training mode, untouched statistics
    cfg['loss']['error_loss_config']['loss_type'] = 'bayesian'
    dcfg = dict(cfg['discriminator'])
    dcfg['load_graph'] = os.path.join(REPO, dcfg['load_graph'])
    if (args.height, args.width) != (256, 512):  # the head is sized to the last feature map
        stages = len(dcfg['layers']) + 1
        ch = dcfg['final_conv']['out_channels']
        dcfg['linear_in_features'] = ch * (args.height >> stages) * (args.width >> stages)
    B = args.batch
    left = torch.rand(B, 3, args.height, args.width, generator=g).cuda()
    right = torch.rand(B, 3, args.height, args.width, generator=g).cuda()

    torch.manual_seed(0)
    d = M.RandomDiscriminator(**dcfg, dtype=args.dtype).cuda().train()
    lf = TukraUncertaintyLoss(**cfg['loss'])
    dlf = torch.nn.BCELoss()
    opt, dopt = Adam(m.parameters(), 1e-4), Adam(d.parameters(), 1e-4)
    init = (deepcopy(m.state_dict()), deepcopy(d.state_dict()))
    scale, freq, index = 0.3, 10, lf.perceptual_start
    gs = _GraphSteps(m, lf, opt, 4)
    eager_clone = deepcopy(d)

    def reset():
        m.load_state_dict(init[0])
        d.load_state_dict(init[1])

    def captured_leg(n):
        clone = gs.bind_discriminator(d, dopt, dlf, B)
        for i in range(n):
            out = gs(left, right, scale, perceptual=True)
            assert out is not None and len(out) == 3
            if i % freq == 0:
                clone.load_state_dict(d.state_dict())
        return out

    def eager_leg(n):
        # on the loop's one stream, as train_one_epoch's eager fallback (see
        # _GraphSteps.stream): the captured leg's graphs stay valid beside it
        eager_clone.load_state_dict(d.state_dict())
        cur = torch.cuda.current_stream()
        gs.stream.wait_stream(cur)
        with torch.cuda.stream(gs.stream):
            for i in range(n):
                out = train_step(m, left, right, lf, opt, scale, 4, index, d, eager_clone, dopt,
                                 dlf, batch_size=B)
                if i % freq == 0:
                    eager_clone.load_state_dict(d.state_dict())
        cur.wait_stream(gs.stream)
        return out

    legs = {'captured': captured_leg, 'eager': eager_leg}
    ms = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, leg in legs.items():
            reset()
            leg(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = leg(args.steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert all(bool(torch.isfinite(t)) for t in out), (name, [float(t) for t in out])
    assert gs.captures == 1, gs.captures

    def leg_result(v):
        mean = sum(v) / len(v)
        return {'pairs_per_s': round(B * 1e3 / mean, 2), 'ms_per_step': round(mean, 4),
                'repeats_pairs_per_s': [round(B * 1e3 / x, 2) for x in v],
                'spread_rel': round((max(v) - min(v)) / mean, 5)}
    res = {'bench': 'adversarial_step', 'config': 'C3', 'batch': B, 'height': args.height,
           'width': args.width, 'dtype': args.dtype, 'loss_type': 'bayesian',
           'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0)}
    for name, v in ms.items():
        res[name] = leg_result(v)
    res['captured_over_eager'] = round(res['captured']['pairs_per_s'] / res['eager']['pairs_per_s'], 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
