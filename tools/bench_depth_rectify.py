#!/usr/bin/env python
"""Cost of stage 0 of the deployment path: DepthPipeline(rectify=...), the raw
camera frame undistorted and stereo-rectified inside the captured graph,
against the same frame made from torch device ops and on the host ahead of the
plain pipeline.

1024x1280 raw uint8 frames -> 1024x1280 rectified -> the 256x512 bf16 model
(config.yml, formula weights, running statistics moved by one training-mode
forward) -> 1024x1280 outputs, B=1; five legs in one process, alternated
``--repeats`` times (default 3):

  plain      (a) DepthPipeline(rectify=None) on an already rectified frame
  analytic   (b) rectify=Calibration: two more launches in the graph
             (um_frame_rectify with the map computed in the kernel, um_valid_and)
  table      (c) rectify=RemapTable of the same map (8 more bytes read per pixel)
  torch_ops  (d) the rectified frame from torch device ops -- the frame to f32
             NCHW, grid_sample (bilinear, zeros, align_corners=True) on the f32
             map, round, clamp, uint8 NHWC -- then leg (a)
  host       (e) the rectified frame on the host --
             scipy.ndimage.map_coordinates(order=1, cval=0) per channel on the
             f32 map, round, uint8 -- then leg (a) on that host frame (cv2 is
             not a dependency of this project)

The camera: K = (1035.3, 1034.9, 596.5, 520.4), dist = (-0.0006, 0.0041, 0.0003,
-0.0009, -0.002), R = Rz(0.003) Ry(-0.012) Rx(0.004), P = (1035, 1035, 640,
512).  Gates as tools/bench_depth_render.py.  Frames: seeded uniform bytes
(torch.Generator seed 7), resident on the device (leg (e): on the host, which
is where a host remap finds them).  Every leg is warmed up, then timed over
max(``--calls`` (>= 20), about ``--seconds`` worth of calls) calls ending in a
synchronise; the host leg over ``--host-calls`` calls.

Prints ONE JSON line (``--out FILE`` also stores it): ms per call per leg
(median of the repeats, each repeat, relative spread), each leg's cost over
plain, torch_ops and host over the analytic stage's cost, whether the stage
beat torch_ops in every repeat, the number of bytes in which the torch_ops and
host frames differ from the pipeline's (the roundings differ: reported, not
gated), the inside share and the stage's bytes moved over its added time.
"""
import json

import _bench

CAMERA = dict(K=(1035.3, 1034.9, 596.5, 520.4), dist=(-0.0006, 0.0041, 0.0003, -0.0009, -0.002),
              angles=(0.003, -0.012, 0.004), P=(1035.0, 1035.0, 640.0, 512.0))


def rot(rz, ry, rx):
    """Rz(rz) @ Ry(ry) @ Rx(rx)"""
    import numpy as np
    cz, sz, cy, sy, cx, sx = (f(a) for a in (rz, ry, rx) for f in (np.cos, np.sin))
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ \
        np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def f32_map(block, Hr, Wr):
    """(mx, my) f32 [Hr, Wr]: the map of include/umamd.h "rectification" in
    numpy f32, one operation per step"""
    import numpy as np
    f = np.float32
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (f(x) for x in block[:12])
    m = [f(x) for x in block[12:21]]
    u = np.arange(Wr, dtype=f)[None, :]
    v = np.arange(Hr, dtype=f)[:, None]
    X = (m[0] * u + m[1] * v) + m[2]
    Y = (m[3] * u + m[4] * v) + m[5]
    W = (m[6] * u + m[7] * v) + m[8]
    x, y = X / W, Y / W
    x2, y2, xy = x * x, y * y, x * y
    r2 = x2 + y2
    kr = (f(1) + r2 * (k1 + r2 * (k2 + r2 * k3))) / (f(1) + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = (x * kr + (f(2) * p1) * xy) + p2 * (r2 + f(2) * x2)
    yd = (y * kr + p1 * (r2 + f(2) * y2)) + (f(2) * p2) * xy
    return fx * xd + cx, fy * yd + cy


def main():
    ap = _bench.parser(__doc__, repeats=3, frames=True)
    ap.add_argument('--host-calls', type=int, default=5, help='timed calls of the host leg')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    if args.calls < 20 or args.repeats < 3 or args.host_calls < 1:
        ap.error('--calls must be at least 20, --repeats at least 3, --host-calls at least 1')

    import numpy as np
    import torch
    import torch.nn.functional as F
    from scipy import ndimage

    from umamd.deploy import DepthPipeline
    from umamd.rectify import Calibration, RemapTable

    scale = _bench.SCALE
    B, H, W, Hs, Ws = args.batch, args.height, args.width, args.src_height, args.src_width
    m, _, g = _bench.build_model(args.dtype, H, W)
    host_frames = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    frames = host_frames.cuda()
    dev = frames.device

    cal = Calibration(CAMERA['K'], CAMERA['dist'], R=rot(*CAMERA['angles']), P=CAMERA['P'])
    mx, my = f32_map(cal.block(), Hs, Ws)
    gates = _bench.depth_gates(Ws)
    kw = dict(batch=B, height=H, width=W, scale=scale, **gates)
    plain = DepthPipeline(m, Hs, Ws, **kw)
    analytic = DepthPipeline(m, Hs, Ws, rectify=cal, **kw)
    table = DepthPipeline(m, Hs, Ws, rectify=RemapTable(mx, my), **kw)

    # align_corners=True: -1 and 1 are the centres of the first and last pixel
    grid = torch.from_numpy(np.stack([2 * mx / np.float32(Ws - 1) - 1,
                                      2 * my / np.float32(Hs - 1) - 1], -1)).to(dev)
    grid = grid[None].expand(B, -1, -1, -1).contiguous()

    def torch_frame():
        x = frames.permute(0, 3, 1, 2).float()
        y = F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        return y.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    coords = np.stack([my, mx])
    host_np = host_frames.numpy()

    def host_frame():
        out = np.empty((B, Hs, Ws, 3), np.uint8)
        for n in range(B):
            for ch in range(3):
                r = ndimage.map_coordinates(host_np[n, :, :, ch].astype(np.float32), coords,
                                            order=1, mode='constant', cval=0.0)
                out[n, :, :, ch] = np.clip(np.rint(r), 0, 255)
        return torch.from_numpy(out)

    rect = analytic(frames)['frame'].clone()
    legs = {'plain': lambda: plain(rect),
            'analytic': lambda: analytic(frames),
            'table': lambda: table(frames),
            'torch_ops': lambda: plain(torch_frame()),
            'host': lambda: plain(host_frame())}
    ms, calls = _bench.time_legs(legs, args.repeats, {'default': args.warmup, 'host': 1},
                                 args.calls, args.seconds, fixed_calls={'host': args.host_calls})

    # the same frame?  bytes that differ from the pipeline's (the roundings differ)
    oa = {k: v.clone() for k, v in analytic(frames).items()}
    ot = table(frames)
    assert torch.equal(oa['frame'], ot['frame']) and torch.equal(oa['inside'], ot['inside'])
    op = plain(rect)
    for k in ('disparity', 'depth', 'uncertainty', 'lr_error'):
        assert torch.equal(op[k], oa[k]), k
    assert torch.equal(oa['valid'], op['valid'] & oa['inside'][None])
    diff_torch = int((torch_frame() != oa['frame']).sum())
    diff_host = int((host_frame().to(dev) != oa['frame']).sum())
    step_torch = int((torch_frame().int() - oa['frame'].int()).abs().max())
    step_host = int((host_frame().to(dev).int() - oa['frame'].int()).abs().max())

    res = {'bench': 'depth_rectify', 'batch': B, 'src_height': Hs, 'src_width': Ws,
           'rect_height': Hs, 'rect_width': Ws, 'height': H, 'width': W, 'dtype': args.dtype,
           'frames': 'device (host leg: host)', 'camera': CAMERA, 'min_calls': args.calls,
           'seconds': args.seconds, 'warmup': args.warmup, 'repeats': args.repeats,
           'statistic': 'median of the repeats', 'device': torch.cuda.get_device_name(0)}
    res.update({name: _bench.leg_result(ms[name], calls[name]) for name in legs})
    med = {name: res[name]['ms_per_call'] for name in legs}
    # bytes the stage moves per output pixel: 3 written + 1 of inside, about 3
    # read (every raw byte once through the caches; the four taps of a pixel
    # share lines with its neighbours), the table mode 8 more; um_valid_and
    # reads 2 and writes 1
    px = B * Hs * Ws
    moved = {'analytic': 10 * px, 'table': 18 * px}
    for name in ('analytic', 'table', 'torch_ops', 'host'):
        added = med[name] - med['plain']
        res[f'{name}_minus_plain_ms'] = round(added, 4)
        res[f'{name}_minus_plain_ms_per_repeat'] = [round(b - a, 4)
                                                    for a, b in zip(ms['plain'], ms[name])]
        if name in moved:
            res[f'{name}_bytes_moved'] = moved[name]
            res[f'{name}_gb_per_s_of_added_time'] = \
                round(moved[name] / (added * 1e-3) / 1e9, 1) if added > 0 else None
    stage = med['analytic'] - med['plain']
    for other in ('torch_ops', 'host'):
        res[f'{other}_added_over_analytic_added'] = \
            round((med[other] - med['plain']) / stage, 2) if stage > 0 else None
    for mode in ('analytic', 'table'):
        res[f'{mode}_faster_than_torch_ops_in_every_repeat'] = all(
            a < t for a, t in zip(ms[mode], ms['torch_ops']))
    res['torch_ops_bytes_differing_from_pipeline'] = diff_torch
    res['torch_ops_largest_difference'] = step_torch
    res['host_bytes_differing_from_pipeline'] = diff_host
    res['host_largest_difference'] = step_host
    res['frame_bytes'] = 3 * px
    res['inside_share'] = float(oa['inside'].float().mean())
    res['valid_share'] = float(oa['valid'].float().mean())
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
