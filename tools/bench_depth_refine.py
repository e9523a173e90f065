#!/usr/bin/env python
"""Cost of the refine stage of the deployment path: DepthPipeline's guided,
confidence-weighted smoothing and its per-pixel temporal fusion against the
same maps composed from torch device ops.

1024x1280 uint8 frames -> the 256x512 bf16 model (config.yml, formula weights,
running statistics moved by one training-mode forward) -> 1024x1280 outputs,
B=1; five legs in one process, alternated ``--repeats`` times (default 3):

  plain      (a) DepthPipeline(refine=None)
  spatial    (b) refine='spatial' (two more launches in the graph:
             um_disp_smooth, um_disp_fuse without state)
  temporal   (c) refine='temporal' (one more launch: um_disp_fuse)
  both       (d) refine='both' (two more launches)
  torch_ops  (e) leg (a), then the maps of leg (d) from torch ops on the
             device: the (2R+1)^2 taps as shifted slices accumulated in the
             definition's order, the recursive filter and the gates as
             elementwise ops, the state in two tensors of its own

Gates as tools/bench_depth_render.py; radius, step and the seven parameters
are the pipeline's defaults (radius 2, step round(1280 / 512) = 2).  Frames:
seeded uniform bytes (torch.Generator seed 7), resident on the device -- the
hardest guide there is: every colour-table lookup of a wave goes elsewhere.
Every leg is warmed up, then timed over max(``--calls`` (>= 20), about
``--seconds`` worth of calls) calls ending in a synchronise.

Prints ONE JSON line: ms per call per leg (median of the repeats, each repeat,
relative spread), each stage's cost over plain of the same run, torch_ops /
both over plain, whether both beat torch_ops in every repeat, in how many
elements the torch_ops maps differ from the pipeline's after two calls from an
empty state and by how much at most, and the net bytes the temporal stage
moves over its added time.
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
    from umamd.refine import tables

    B, H, W, Hs, Ws = args.batch, args.height, args.width, args.src_height, args.src_width
    m, _, g = _bench.build_model(args.dtype, H, W)
    frames = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda()
    dev = frames.device

    gates = _bench.depth_gates(Ws)
    kw = dict(batch=B, height=H, width=W, scale=_bench.SCALE, **gates)
    pipes = {'plain': DepthPipeline(m, Hs, Ws, **kw)}
    for mode in ('spatial', 'temporal', 'both'):
        pipes[mode] = DepthPipeline(m, Hs, Ws, refine=mode, **kw)
    plain, both = pipes['plain'], pipes['both']
    R, step, q = both.refine_radius, both.refine_step, both.refine_params

    def f32(x):
        return torch.tensor(x, dtype=torch.float32, device=dev)
    S, G = (t.to(dev) for t in tables(R, q['sigma_space'], q['sigma_colour']))
    eps, a, floor, pn = (f32(q[k]) for k in ('conf_eps', 'noise_scale', 'var_floor',
                                             'process_noise'))
    g2 = f32(q['gate'] * q['gate'])
    fb, min_disp, max_unc, max_lr = (f32(gates[k]) for k in (
        'focal_baseline', 'min_disparity', 'max_uncertainty', 'max_lr_error'))
    colours = frames.to(torch.int16)
    state = [torch.zeros((B, Hs, Ws), device=dev), torch.full((B, Hs, Ws), -1.0, device=dev)]
    zero = torch.zeros((), device=dev)

    def torch_ops():
        o = plain(frames)
        d, u, lr = o['disparity'], o['uncertainty'], o['lr_error']
        # um_disp_smooth
        live = torch.isfinite(d) & torch.isfinite(u)
        c = 1.0 / (u * u + eps)
        num, nus, den = torch.zeros_like(d), torch.zeros_like(d), torch.zeros_like(d)
        for j in range(-R, R + 1):
            for i in range(-R, R + 1):
                dy, dx = j * step, i * step
                py = slice(max(0, -dy), min(Hs, Hs - dy))
                px = slice(max(0, -dx), min(Ws, Ws - dx))
                ty = slice(py.start + dy, py.stop + dy)
                tx = slice(px.start + dx, px.stop + dx)
                k = (colours[:, py, px] - colours[:, ty, tx]).abs().sum(-1).long()
                w = (S[abs(j) * (R + 1) + abs(i)] * G[k]) * c[:, ty, tx]
                w = torch.where(live[:, ty, tx], w, zero)
                num[:, py, px] += w * d[:, ty, tx].nan_to_num(0.0, 0.0, 0.0)
                nus[:, py, px] += w * u[:, ty, tx].nan_to_num(0.0, 0.0, 0.0)
                den[:, py, px] += w
        ok = (den > 0) & torch.isfinite(den)
        d = torch.where(ok, num / den, d)
        u = torch.where(ok, nus / den, u)
        # um_disp_fuse
        mean, var = state
        t = a * u
        mm = t * t + floor
        fresh = torch.isfinite(d) & torch.isfinite(mm)
        p = var + pn
        e = d - mean
        pm = p + mm
        keep = fresh & (var >= 0) & (e * e <= g2 * pm)
        K = p / pm
        state[0] = torch.where(keep, mean + K * e, torch.where(fresh, d, mean))
        state[1] = torch.where(keep, p - K * p, torch.where(fresh, mm, var))
        D = torch.where(state[1] >= 0, state[0], d)
        far = D > min_disp
        return {'disparity': D, 'uncertainty': u, 'depth': torch.where(far, fb / D, zero),
                'valid': far & (u <= max_unc) & (lr <= max_lr), 'disparity_var': state[1]}

    legs = {k: (lambda p=p: p(frames)) for k, p in pipes.items()}
    legs['torch_ops'] = torch_ops
    ms, calls = _bench.time_legs(legs, args.repeats, args.warmup, args.calls, args.seconds)

    # the same maps?  two calls from an empty state (the second one fuses)
    both.reset_refine()
    state[1].fill_(-1.0)
    for _ in range(2):
        ob = both(frames)
        ot = torch_ops()
    differing, worst = {}, {}
    for k, t in ot.items():
        if t.dtype == torch.bool:
            differing[k] = int((t != ob[k]).sum())
        else:
            differing[k] = int((t.view(torch.int32) != ob[k].view(torch.int32)).sum())
            worst[k] = float((t - ob[k]).abs().nan_to_num(0.0).max())
    sp = pipes['spatial'](frames)
    changed = float((sp['disparity'] != sp['raw_disparity']).float().mean())

    res = {'bench': 'depth_refine', 'batch': B, 'src_height': Hs, 'src_width': Ws, 'height': H,
           'width': W, 'dtype': args.dtype, 'frames': 'device', 'radius': R, 'step': step,
           'refine_params': q, 'min_calls': args.calls, 'seconds': args.seconds,
           'warmup': args.warmup, 'repeats': args.repeats, 'statistic': 'median of the repeats',
           'device': torch.cuda.get_device_name(0)}
    res.update({name: _bench.leg_result(ms[name], calls[name]) for name in legs})
    med = {name: res[name]['ms_per_call'] for name in legs}
    for name in ('spatial', 'temporal', 'both', 'torch_ops'):
        res[f'{name}_minus_plain_ms'] = round(med[name] - med['plain'], 4)
        res[f'{name}_minus_plain_ms_per_repeat'] = [round(b - a, 4)
                                                    for a, b in zip(ms['plain'], ms[name])]
    res['torch_ops_over_both_added'] = round((med['torch_ops'] - med['plain']) /
                                             (med['both'] - med['plain']), 2)
    res['both_faster_than_torch_ops_in_every_repeat'] = all(
        b < t for b, t in zip(ms['both'], ms['torch_ops']))
    res['torch_ops_elements_differing_from_pipeline'] = differing
    res['torch_ops_max_abs_difference'] = worst
    res['elements_per_map'] = B * Hs * Ws
    res['share_of_pixels_the_smoothing_changed'] = round(changed, 4)
    # um_disp_fuse with state reads disp, unc, lr_error, mean, var and writes mean, var,
    # disparity, uncertainty, depth (4 bytes each) and valid (1): 41 bytes per pixel, and
    # um_depth_post leaves its depth and valid stores (5 bytes) to it: 36 net
    px = B * Hs * Ws
    added = med['temporal'] - med['plain']
    res['temporal_net_bytes_moved'] = 36 * px
    res['temporal_gb_per_s_of_added_time'] = round(36 * px / (added * 1e-3) / 1e9, 1) \
        if added > 0 else None
    print(json.dumps(res))


if __name__ == '__main__':
    main()
