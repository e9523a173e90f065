#!/usr/bin/env python
"""Frame latency of the deployment path: a uint8 camera frame to disparity,
depth, uncertainty, left-right error and validity mask at the frame's size.

1024x1280 uint8 frames -> the 256x512 bf16 model (config.yml, formula weights,
running statistics moved by one training-mode forward) -> 1024x1280 outputs,
B=1; four legs in one process, alternated ``--repeats`` times (default 2):

  forward         the bare InferenceEngine(capture=True) call on a resized input
  composed        what the APIs before umamd.deploy allow: imageprep.stereo_prep
                  with the frame as both views, the captured engine, and the
                  post-processing as torch device ops (grid_sample on the
                  reference's linspace grid, one interpolate of the three maps,
                  compare, divide)
  pipeline        umamd.deploy.DepthPipeline(capture=True)
  pipeline_eager  DepthPipeline(capture=False)

Frames: seeded uniform bytes (torch.Generator seed 7), resident on the device
for every leg (no host transfer in the timed span).  Every leg is warmed up,
then timed over max(``--calls`` (>= 20), about ``--seconds`` worth of calls)
calls ending in a synchronise.

Each repeat then also times ``--calls`` calls with a synchronise after every
one (``sync_ms_per_call``: the latency of one frame on an idle device, host
launch time included).

Prints ONE JSON line: ms per frame per leg (mean, each repeat, relative
spread), pipeline - forward (the cost of the two new stages), composed /
pipeline, whether the pipeline was faster in every repeat, and the max-abs
difference of the composed leg's outputs from the pipeline's on the timed
frames.
"""
import json
import math
import time

import _bench


def main():
    ap = _bench.parser(__doc__, frames=True)
    args = ap.parse_args()
    if args.calls < 20 or args.repeats < 2:
        ap.error('--calls must be at least 20 and --repeats at least 2')

    import torch
    import torch.nn.functional as F

    from umamd.deploy import DepthPipeline
    from umamd.imageprep import stereo_prep
    from umamd.infer import InferenceEngine

    scale = _bench.SCALE
    B, H, W, Hs, Ws = args.batch, args.height, args.width, args.src_height, args.src_width
    m, _, g = _bench.build_model(args.dtype, H, W)
    frames = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda()
    dev = frames.device

    gates = _bench.depth_gates(Ws)
    fb, min_disp, max_unc, max_lr = gates.values()
    eng = InferenceEngine(m, B, H, W, scale)
    pipes = {'pipeline': DepthPipeline(m, Hs, Ws, batch=B, height=H, width=W, scale=scale,
                                       **gates),
             'pipeline_eager': DepthPipeline(m, Hs, Ws, batch=B, height=H, width=W, scale=scale,
                                             capture=False, **gates)}
    prep8 = torch.zeros(B, 8, device=dev)
    prep8[:, 2:7] = 1
    xb = torch.linspace(0, 1, W, device=dev).repeat(B, H, 1)
    yb = torch.linspace(0, 1, H, device=dev).repeat(B, W, 1).transpose(1, 2)
    resized = stereo_prep({'left': frames, 'right': frames, 'prep': prep8}, (H, W), dev)['left']

    def composed():
        with torch.no_grad():
            left = stereo_prep({'left': frames, 'right': frames, 'prep': prep8}, (H, W),
                               dev)['left']
            d, u = eng(left)
            dl, dr, sl = d[:, 0:1], d[:, 1:2], u[:, 0:1]
            flow = torch.stack((xb - dl.squeeze(1), yb), dim=3) * 2 - 1
            e = (dl - F.grid_sample(dr, flow, mode='bilinear', padding_mode='zeros',
                                    align_corners=False)).abs()
            up = F.interpolate(torch.cat([dl, e, sl], 1), size=(Hs, Ws), mode='bilinear',
                               align_corners=True)
            disparity, lr_error, uncertainty = up[:, 0] * Ws, up[:, 1] * Ws, up[:, 2]
            far = disparity > min_disp
            depth = torch.where(far, fb / disparity, torch.zeros_like(disparity))
            valid = far & (uncertainty <= max_unc) & (lr_error <= max_lr)
        return {'disparity': disparity, 'depth': depth, 'uncertainty': uncertainty,
                'lr_error': lr_error, 'valid': valid}

    legs = {'forward': lambda: eng(resized), 'composed': composed,
            'pipeline': lambda: pipes['pipeline'](frames),
            'pipeline_eager': lambda: pipes['pipeline_eager'](frames)}
    sync_ms = {k: [] for k in legs}

    def sync_latency(name, leg):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            leg()
            torch.cuda.synchronize()
        sync_ms[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
    ms, calls = _bench.time_legs(legs, args.repeats, args.warmup, args.calls, args.seconds,
                                 after=sync_latency)

    ref = composed()
    out = pipes['pipeline'](frames)
    diff = {k: float((ref[k].float() - out[k].float()).abs().max()) for k in ref}
    diff['valid'] = float((ref['valid'] != out['valid']).float().mean())  # share of pixels
    assert all(math.isfinite(v) for v in diff.values())

    def leg_result(name):
        r = _bench.leg_result(ms[name], calls[name], _bench.mean)
        return {'ms_per_frame': round(_bench.mean(ms[name]) / B, 4), **r,
                'sync_ms_per_call': [round(x, 4) for x in sync_ms[name]]}
    res = {'bench': 'depth_pipeline', 'batch': B, 'src_height': Hs, 'src_width': Ws, 'height': H,
           'width': W, 'dtype': args.dtype, 'frames': 'device', 'min_calls': args.calls,
           'seconds': args.seconds, 'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0)}
    res.update({name: leg_result(name) for name in legs})
    res['pipeline_minus_forward_ms'] = round(
        res['pipeline']['ms_per_call'] - res['forward']['ms_per_call'], 4)
    res['composed_over_pipeline'] = round(
        res['composed']['ms_per_call'] / res['pipeline']['ms_per_call'], 4)
    res['pipeline_faster_in_every_repeat'] = all(
        p < c for p, c in zip(ms['pipeline'], ms['composed']))
    res['composed_max_abs_diff_from_pipeline'] = diff
    res['valid_share'] = float(out['valid'].float().mean())
    res['disparity_max_px'] = float(out['disparity'].max())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
