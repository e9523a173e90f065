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
import json
import math

import _bench


def main():
    ap = _bench.parser(__doc__)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
    args = ap.parse_args()
    if args.calls < 20 or args.repeats < 2:
        ap.error('--calls must be at least 20 and --repeats at least 2')

    import torch

    from umamd.infer import InferenceEngine

    scale = _bench.SCALE
    m, _, g = _bench.build_model(args.dtype, args.height, args.width)

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
        ms, calls = _bench.time_legs(legs, args.repeats, args.warmup, args.calls, args.seconds)
        ref = eager().float()
        d, u = engines['fused'](left)
        diff = float((torch.cat([d, u], 1) - ref).abs().max())
        assert math.isfinite(diff)

        def leg_result(name):
            mean = _bench.mean(ms[name])
            return {'frames_per_s': round(B * 1e3 / mean, 2), 'ms_per_frame': round(mean / B, 4),
                    **_bench.leg_result(ms[name], calls[name], _bench.mean)}
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
