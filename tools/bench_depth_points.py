#!/usr/bin/env python
"""Cost of the point stage of the deployment path: DepthPipeline's organised
XYZ map and packed, coloured cloud against the same cloud composed from torch
device ops (nonzero and gathers, which synchronise with the host).

1024x1280 uint8 frames -> the 256x512 bf16 model (config.yml, formula weights,
running statistics moved by one training-mode forward) -> 1024x1280 outputs,
B=1; six legs in one process, alternated ``--repeats`` times (default 3):

  plain          (a) DepthPipeline(points=None)
  map            (b) points='map' (one more launch in the graph:
                 um_depth_backproject)
  cloud          (c) points='cloud' (three more launches: um_depth_cloud's
                 count, scan and pack)
  cloud_stride2  (d) the same with point_stride=2
  both           (e) points='both' (four more launches)
  torch_ops      (f) leg (a), then the cloud of leg (c) from torch ops on the
                 device: valid.nonzero() (which synchronises), the gathers of
                 depth, uncertainty and frame, the arithmetic, the stacks and
                 the per-image offsets

Gates as tools/bench_depth_render.py; the intrinsics put the principal point
at the frame's centre.  Frames: seeded uniform bytes (torch.Generator seed 7),
resident on the device.  Every leg is warmed up, then timed over
max(``--calls`` (>= 20), about ``--seconds`` worth of calls) calls ending in a
synchronise.

Prints ONE JSON line: ms per call per leg (median of the repeats, each repeat,
relative spread), each stage's cost over plain, torch_ops / cloud, whether
cloud beat torch_ops in every repeat, the number of bytes in which the
torch_ops cloud differs from the pipeline's, the kept share, and each stage's
bytes moved over its added time (GB/s, to be read against the HBM rate).
"""
import json

import _bench


def main():
    ap = _bench.parser(__doc__, repeats=3, frames=True)
    args = ap.parse_args()
    if args.calls < 20 or args.repeats < 3:
        ap.error('--calls must be at least 20 and --repeats at least 3')

    import torch

    from umamd.deploy import DepthPipeline

    scale = _bench.SCALE
    B, H, W, Hs, Ws = args.batch, args.height, args.width, args.src_height, args.src_width
    m, _, g = _bench.build_model(args.dtype, H, W)
    frames = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda()
    dev = frames.device

    gates = _bench.depth_gates(Ws)
    kw = dict(batch=B, height=H, width=W, scale=scale, **gates)
    intr = (0.9 * Ws, 0.9 * Ws, (Ws - 1) / 2, (Hs - 1) / 2)
    pkw = dict(intrinsics=intr, **kw)
    pipes = {'plain': DepthPipeline(m, Hs, Ws, **kw),
             'map': DepthPipeline(m, Hs, Ws, points='map', **pkw),
             'cloud': DepthPipeline(m, Hs, Ws, points='cloud', **pkw),
             'cloud_stride2': DepthPipeline(m, Hs, Ws, points='cloud', point_stride=2, **pkw),
             'both': DepthPipeline(m, Hs, Ws, points='both', **pkw)}
    plain = pipes['plain']
    fx, fy, cx, cy = (torch.tensor(x, dtype=torch.float32, device=dev) for x in intr)

    def torch_ops():
        o = plain(frames)
        n, v, u = o['valid'].nonzero(as_tuple=True)  # synchronises
        z = o['depth'][n, v, u]
        x = (u.float() - cx) * z / fx
        y = (v.float() - cy) * z / fy
        xyzu = torch.stack([x, y, z, o['uncertainty'][n, v, u]], 1)
        rgb = frames[n, v, u]
        rgba = torch.cat([rgb, torch.full_like(rgb[:, :1], 255)], 1)
        counts = o['valid'].view(B, -1).sum(1)
        offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()
        return xyzu, rgba, offsets

    legs = {k: (lambda p=p: p(frames)) for k, p in pipes.items()}
    legs['torch_ops'] = torch_ops
    ms, calls = _bench.time_legs(legs, args.repeats, args.warmup, args.calls, args.seconds)

    # the same cloud?  bytes that differ from the pipeline's
    oc = pipes['cloud'](frames)
    k = int(oc['cloud_offsets'][-1])
    tx, tc, to = torch_ops()
    assert len(tx) == k, (len(tx), k)
    diff = int((tx.view(torch.uint8) != oc['cloud_xyzu'][:k].view(torch.uint8)).sum()) + \
        int((tc != oc['cloud_rgba'][:k]).sum()) + \
        int((to.view(torch.uint8) != oc['cloud_offsets'].view(torch.uint8)).sum())
    ob = pipes['both'](frames)
    assert torch.equal(ob['cloud_xyzu'][:k], oc['cloud_xyzu'][:k])
    assert torch.equal(ob['xyz'], pipes['map'](frames)['xyz'])
    o = plain(frames)
    valid = o['valid']
    k2 = int(pipes['cloud_stride2'](frames)['cloud_offsets'][-1])
    assert k == int(valid.sum()) and k2 == int(valid[:, ::2, ::2].sum())

    res = {'bench': 'depth_points', 'batch': B, 'src_height': Hs, 'src_width': Ws, 'height': H,
           'width': W, 'dtype': args.dtype, 'frames': 'device', 'intrinsics': list(intr),
           'min_calls': args.calls, 'seconds': args.seconds, 'warmup': args.warmup,
           'repeats': args.repeats, 'statistic': 'median of the repeats',
           'device': torch.cuda.get_device_name(0)}
    res.update({name: _bench.leg_result(ms[name], calls[name]) for name in legs})
    med = {name: res[name]['ms_per_call'] for name in legs}
    # bytes a stage moves: the map reads depth (4) and valid (1) and writes 12
    # per pixel; the cloud reads valid twice (count, pack), depth, uncertainty
    # and the frame (4 + 4 + 3) per lattice site and writes 16 + 4 per point
    # (a strided lattice touches whole 64-byte lines: this is the useful part)
    px = B * Hs * Ws
    sites2 = B * -(-Hs // 2) * -(-Ws // 2)
    moved = {'map': 17 * px, 'cloud': 13 * px + 20 * k, 'cloud_stride2': 13 * sites2 + 20 * k2}
    moved['both'] = moved['map'] + moved['cloud']
    for name in ('map', 'cloud', 'cloud_stride2', 'both', 'torch_ops'):
        added = med[name] - med['plain']
        res[f'{name}_minus_plain_ms'] = round(added, 4)
        res[f'{name}_minus_plain_ms_per_repeat'] = [round(b - a, 4)
                                                    for a, b in zip(ms['plain'], ms[name])]
        if name in moved:
            res[f'{name}_bytes_moved'] = moved[name]
            res[f'{name}_gb_per_s_of_added_time'] = \
                round(moved[name] / (added * 1e-3) / 1e9, 1) if added > 0 else None
    res['torch_ops_over_cloud'] = round(med['torch_ops'] / med['cloud'], 4)
    res['cloud_faster_than_torch_ops_in_every_repeat'] = all(
        c < t for c, t in zip(ms['cloud'], ms['torch_ops']))
    res['torch_ops_bytes_differing_from_pipeline'] = diff
    res['cloud_bytes'] = 20 * k + 4 * (B + 1)
    res['points'] = k
    res['points_stride2'] = k2
    res['kept_share'] = float(valid.float().mean())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
