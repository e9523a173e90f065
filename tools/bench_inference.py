#!/usr/bin/env python
"""Inference latency of the depth / uncertainty model: today's eager
``model.eval()`` forward against ``umamd.infer.InferenceEngine``.

At 256x512 bf16 (config.yml, formula weights, running statistics moved by one
training-mode forward), for each batch size in ``--batches`` (default 1 and
8), three legs in one process, alternated ``--repeats`` times (default 2):

  eager     model.eval(); model(left, scale) under torch.no_grad()
  unfused   InferenceEngine(fused=False, capture=True): conv + um_bn_elu_fwd
            per layer, build-time packing and coefficients, one HIP graph
  fused     InferenceEngine(fused=True, capture=True): BN folded into the
            convs (UM_EPI_ELU), one HIP graph

Inputs: seeded uniform images (torch.Generator seed 7).  Every leg is warmed
up, then timed over max(``--calls`` (>= 20), about ``--seconds`` worth of
calls) calls ending in a synchronise.

Prints ONE JSON line: frames/s and ms/frame per leg and batch (mean over the
repeats, each repeat, the relative spread), fused / unfused and unfused /
eager, and the max-abs difference of the fused leg's output from the eager
leg's on the timed input.
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'uncertainty-model_amd'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--calls', type=int, default=20, help='minimum timed calls per leg (>= 20)')
    ap.add_argument('--seconds', type=float, default=1.0, help='timed span per leg to fill')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    args = ap.parse_args()
    if args.calls < 20 or args.repeats < 2:
        ap.error('--calls must be at least 20 and --repeats at least 2')

    import torch
    import yaml

    import model as M
    from oracle import model as OM, step as OS
    from umamd.infer import InferenceEngine

    assert torch.cuda.is_available(), 'needs a GPU'
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)
    cfg['model']['encoder']['load_graph'] = os.path.join(REPO, cfg['model']['encoder']['load_graph'])
    scale = 0.3
    m = M.RandomlyConnectedModel(**cfg['model'], dtype=args.dtype)
    graphs = OM.load_stage_graphs(cfg['model']['encoder'])
    m.load_state_dict(OS.formula_state_dict(OS.param_specs(cfg['model'], graphs)))
    m = m.cuda().train()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():  # non-trivial running statistics
        m(torch.rand(2, 3, args.height, args.width, generator=g).cuda(), scale)
    m.eval()

    res = {'bench': 'inference', 'height': args.height, 'width': args.width, 'dtype': args.dtype,
           'min_calls': args.calls, 'seconds': args.seconds, 'warmup': args.warmup,
           'repeats': args.repeats, 'device': torch.cuda.get_device_name(0), 'batches': {}}
    for B in args.batches:
        left = torch.rand(B, 3, args.height, args.width, generator=g).cuda()
        engines = {'unfused': InferenceEngine(m, B, args.height, args.width, scale, fused=False),
                   'fused': InferenceEngine(m, B, args.height, args.width, scale, fused=True)}

        def eager():
            with torch.no_grad():
                return m(left, scale)
        legs = {'eager': eager, 'unfused': lambda: engines['unfused'](left),
                'fused': lambda: engines['fused'](left)}
        ms = {k: [] for k in legs}
        calls = {}
        for _ in range(args.repeats):
            for name, leg in legs.items():
                for _ in range(args.warmup):
                    leg()
                torch.cuda.synchronize()
                if name not in calls:  # size the timed span once per leg
                    t0 = time.perf_counter()
                    for _ in range(5):
                        leg()
                    torch.cuda.synchronize()
                    per = (time.perf_counter() - t0) / 5
                    calls[name] = max(args.calls, min(5000, math.ceil(args.seconds / per)))
                t0 = time.perf_counter()
                for _ in range(calls[name]):
                    leg()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / calls[name])
        ref = eager().float()
        d, u = engines['fused'](left)
        diff = float((torch.cat([d, u], 1) - ref).abs().max())
        assert math.isfinite(diff)

        def leg_result(name):
            v = ms[name]
            mean = sum(v) / len(v)
            return {'frames_per_s': round(B * 1e3 / mean, 2), 'ms_per_frame': round(mean / B, 4),
                    'ms_per_call': round(mean, 4), 'calls': calls[name],
                    'repeats_ms_per_call': [round(x, 4) for x in v],
                    'spread_rel': round((max(v) - min(v)) / mean, 5)}
        r = {name: leg_result(name) for name in legs}
        r['fused_over_unfused'] = round(r['fused']['frames_per_s'] / r['unfused']['frames_per_s'], 4)
        r['unfused_over_eager'] = round(r['unfused']['frames_per_s'] / r['eager']['frames_per_s'], 4)
        r['fused_max_abs_diff_from_eager'] = diff
        r['output_max_abs'] = float(ref.abs().max())
        res['batches'][str(B)] = r
        del engines
    print(json.dumps(res))


if __name__ == '__main__':
    main()
