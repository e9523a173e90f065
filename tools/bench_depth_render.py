#!/usr/bin/env python
"""Cost of the display stage of the deployment path: DepthPipeline's colour-
mapped depth overlay against the same picture composed from torch device ops
and against the host path (copy back, matplotlib, numpy blend).

1024x1280 uint8 frames -> the 256x512 bf16 model (config.yml, formula weights,
running statistics moved by one training-mode forward) -> 1024x1280 outputs,
B=1; five legs in one process, alternated ``--repeats`` times (default 3):

  plain        (a) DepthPipeline(render=None)
  fixed        (b) render='depth', render_range=(lo, hi), opacity=0.6 (one
               more launch in the graph: um_depth_render)
  auto         (c) the same with render_range='auto' (three more launches:
               um_value_range's two, um_depth_render)
  torch_ops    (d) leg (a), then the same picture from torch ops on the
               device: normalise, multiply, clamp, index the table, blend in
               int32, cast
  host         (e) leg (a), then the host path of train.utils.to_heatmap /
               save_image: copy depth and valid back, matplotlib's colour map,
               the x * 255 + 0.5 rounding and the blend in numpy (the frame is
               already on the host: it came from there); ``--host-calls``
               iterations per repeat

The fixed range is the 1st and 99th percentile of the valid depths of the
timed frame, found once before timing.  Frames: seeded uniform bytes
(torch.Generator seed 7), resident on the device (the host leg holds its own
host copy).  Every leg is warmed up, then timed over max(``--calls`` (>= 20),
about ``--seconds`` worth of calls) calls ending in a synchronise; the host
leg synchronises in every call by its nature.

Prints ONE JSON line: ms per call per leg (median of the repeats, each
repeat, relative spread), fixed - plain and auto - plain (the stage's cost),
torch_ops / fixed and host / fixed, whether fixed beat torch_ops in every
repeat, and the number of bytes in which legs (d) and (e) differ from the
pipeline's picture.
"""
import json

import _bench


def main():
    ap = _bench.parser(__doc__, repeats=3, frames=True)
    ap.add_argument('--host-calls', type=int, default=30, help='timed calls of the host leg')
    ap.add_argument('--opacity', type=float, default=0.6)
    args = ap.parse_args()
    if args.calls < 20 or args.repeats < 2 or args.host_calls < 1:
        ap.error('--calls must be at least 20, --repeats at least 2, --host-calls at least 1')

    import matplotlib.pyplot as plt
    import numpy as np
    import torch

    from umamd.deploy import DepthPipeline
    from umamd.render import lut

    scale = _bench.SCALE
    B, H, W, Hs, Ws = args.batch, args.height, args.width, args.src_height, args.src_width
    m, _, g = _bench.build_model(args.dtype, H, W)
    frames_host = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    frames = frames_host.cuda()
    dev = frames.device

    gates = _bench.depth_gates(Ws)
    kw = dict(batch=B, height=H, width=W, scale=scale, **gates)
    plain = DepthPipeline(m, Hs, Ws, **kw)
    out = plain(frames)
    depths = out['depth'][out['valid']]
    assert depths.numel() > 0, 'no valid pixel on the timed frame'
    lo, hi = (float(torch.quantile(depths[:1 << 20], q)) for q in (0.01, 0.99))
    assert hi > lo
    op = args.opacity
    fixed = DepthPipeline(m, Hs, Ws, render='depth', render_range=(lo, hi), opacity=op, **kw)
    auto = DepthPipeline(m, Hs, Ws, render='depth', render_range='auto', opacity=op, **kw)

    table = lut('inferno')
    table_dev = table.to(dev).to(torch.int32)
    a_ok = int(min(max(op, 0.0), 1.0) * 256 + 0.5)
    lo32, den32 = np.float32(lo), np.float32(hi) - np.float32(lo)
    lo_t, den_t = torch.tensor(lo32, device=dev), torch.tensor(den32, device=dev)

    def torch_ops():
        o = plain(frames)
        s = (o['depth'] - lo_t) / den_t * 256
        idx = torch.where(torch.isnan(s), torch.zeros_like(s), s.clamp(0, 255)).long()
        c = table_dev[idx]
        a = torch.where(o['valid'], a_ok, 0).unsqueeze(-1)
        return ((c * a + frames.int() * (256 - a) + 128) >> 8).to(torch.uint8)

    cmap = plt.get_cmap('inferno')

    def host():
        o = plain(frames)
        depth = o['depth'].cpu().numpy()  # synchronises
        valid = o['valid'].cpu().numpy()
        heat = cmap((depth - lo32) / den32)[..., :3]  # to_heatmap: f32 in, f64 colours
        c = np.clip(heat.astype(np.float32) * 255 + 0.5, 0, 255).astype(np.uint8)  # save_image
        a = np.where(valid, a_ok, 0).astype(np.int32)[..., None]
        f = frames_host.numpy().astype(np.int32)
        return ((c.astype(np.int32) * a + f * (256 - a) + 128) >> 8).astype(np.uint8)

    legs = {'plain': lambda: plain(frames), 'fixed': lambda: fixed(frames),
            'auto': lambda: auto(frames), 'torch_ops': torch_ops, 'host': host}
    ms, calls = _bench.time_legs(legs, args.repeats, {'default': args.warmup, 'host': 2},
                                 args.calls, args.seconds, fixed_calls={'host': args.host_calls})

    # the same picture?  bytes that differ from the pipeline's
    pic = fixed(frames)['render'].clone()
    pic_auto = auto(frames)['render'].clone()
    rng = auto._render_stage._range.tolist()
    diff = {'torch_ops': int((torch_ops() != pic).sum()),
            'host': int((torch.from_numpy(host()).to(dev) != pic).sum())}
    o = plain(frames)
    vd = o['depth'][o['valid']]
    assert rng == [float(vd.min()), float(vd.max())], rng

    res = {'bench': 'depth_render', 'batch': B, 'src_height': Hs, 'src_width': Ws, 'height': H,
           'width': W, 'dtype': args.dtype, 'frames': 'device', 'render': 'depth',
           'colour_map': 'inferno', 'render_range': [lo, hi], 'opacity': op,
           'min_calls': args.calls, 'seconds': args.seconds, 'warmup': args.warmup,
           'repeats': args.repeats, 'statistic': 'median of the repeats',
           'device': torch.cuda.get_device_name(0)}
    res.update({name: _bench.leg_result(ms[name], calls[name]) for name in legs})
    med = {k: res[k]['ms_per_call'] for k in legs}
    res['fixed_minus_plain_ms'] = round(med['fixed'] - med['plain'], 4)
    res['auto_minus_plain_ms'] = round(med['auto'] - med['plain'], 4)
    res['torch_ops_minus_plain_ms'] = round(med['torch_ops'] - med['plain'], 4)
    res['host_minus_plain_ms'] = round(med['host'] - med['plain'], 4)
    res['torch_ops_over_fixed'] = round(med['torch_ops'] / med['fixed'], 4)
    res['host_over_fixed'] = round(med['host'] / med['fixed'], 4)
    res['fixed_faster_than_torch_ops_in_every_repeat'] = all(
        b < d for b, d in zip(ms['fixed'], ms['torch_ops']))
    res['fixed_minus_plain_ms_per_repeat'] = [round(b - a, 4)
                                              for a, b in zip(ms['plain'], ms['fixed'])]
    res['auto_minus_plain_ms_per_repeat'] = [round(c - a, 4)
                                             for a, c in zip(ms['plain'], ms['auto'])]
    res['bytes_differing_from_pipeline'] = diff
    res['picture_bytes'] = pic.numel()
    res['auto_range'] = rng
    res['auto_differs_from_fixed_bytes'] = int((pic_auto != pic).sum())
    res['valid_share'] = float(o['valid'].float().mean())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
