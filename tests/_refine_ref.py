"""References of the refine stage (csrc/refine.hip, umamd/refine.py): the
definition of um_disp_smooth and um_disp_fuse in include/umamd.h restated op
for op in numpy f32 -- every step one exactly rounded f32 operation, in the
definition's order, so the device result equals it bit for bit -- and the
inputs the tests plant.  ``dtype=np.float64`` evaluates the same steps in f64
(from the same f32 inputs, tables and blocks)."""
import numpy as np
import torch


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _block(values, dtype):
    """a device block is f32: its values as ``dtype`` scalars"""
    return [dtype(np.float32(v)) for v in values]


def smooth_ref(disp, unc, frame, radius, step, S, G, eps, dtype=np.float32):
    """um_disp_smooth: disp, unc [N, H, W], frame u8 [N, H, W, 3] -> (disp_out,
    unc_out) as torch tensors of ``dtype``.  The taps in row-major order; one
    that is outside the image or not finite leaves the three sums as they are."""
    d, u = _np(disp).astype(dtype), _np(unc).astype(dtype)
    f = _np(frame).astype(np.int32)
    S, G = _np(S).astype(dtype), _np(G).astype(dtype)
    eps, = _block([eps], dtype)
    n, h, w = d.shape
    R = radius
    live = np.isfinite(d) & np.isfinite(u)
    with np.errstate(all='ignore'):
        c = dtype(1) / (u * u + eps)
        num, nus, den = (np.zeros(d.shape, dtype) for _ in range(3))
        for j in range(-R, R + 1):
            for i in range(-R, R + 1):
                dy, dx = j * step, i * step
                py = slice(max(0, -dy), min(h, h - dy))  # the pixels whose tap is inside
                px = slice(max(0, -dx), min(w, w - dx))
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                ty = slice(py.start + dy, py.stop + dy)
                tx = slice(px.start + dx, px.stop + dx)
                k = np.abs(f[:, py, px] - f[:, ty, tx]).sum(-1)
                wgt = (S[abs(j) * (R + 1) + abs(i)] * G[k]) * c[:, ty, tx]
                m = live[:, ty, tx]
                num[:, py, px] = np.where(m, num[:, py, px] + wgt * d[:, ty, tx], num[:, py, px])
                nus[:, py, px] = np.where(m, nus[:, py, px] + wgt * u[:, ty, tx], nus[:, py, px])
                den[:, py, px] = np.where(m, den[:, py, px] + wgt, den[:, py, px])
        ok = (den > 0) & np.isfinite(den)
        out_d = np.where(ok, num / den, d)
        out_u = np.where(ok, nus / den, u)
    assert out_d.dtype == dtype and out_u.dtype == dtype
    return torch.from_numpy(out_d), torch.from_numpy(out_u)


def fuse_ref(disp, unc, lr_error, params, fp, state=None, dtype=np.float32):
    """um_disp_fuse: maps of any one shape; ``params`` = (fb, min_disp,
    max_unc, max_lr), ``fp`` = (eps, a, floor, q, g2, ...); ``state`` = (mean,
    var) or None, NOT modified -> dict of torch tensors: disparity,
    uncertainty, depth, valid (bool) and, with state, mean, var (the new
    state; var is also disp_var) and the branch masks keep, reset, stale."""
    d, s, lr = (_np(x).astype(dtype) for x in (disp, unc, lr_error))
    fb, min_disp, max_unc, max_lr = _block(params, dtype)
    _, a, floor, q, g2 = _block(list(fp)[:5], dtype)
    out = {}
    with np.errstate(all='ignore'):
        D = d
        if state is not None:
            mean, var = (_np(x).astype(dtype) for x in state)
            t = a * s
            m = t * t + floor
            fresh = np.isfinite(d) & np.isfinite(m)
            p = var + q
            e = d - mean
            pm = p + m
            keep = fresh & (var >= 0) & (e * e <= g2 * pm)
            K = p / pm
            new_mean = np.where(keep, mean + K * e, np.where(fresh, d, mean))
            new_var = np.where(keep, p - K * p, np.where(fresh, m, var))
            D = np.where(new_var >= 0, new_mean, d)
            out.update(mean=new_mean, var=new_var, keep=keep, reset=fresh & ~keep, stale=~fresh)
        far = D > min_disp
        out.update(disparity=D, uncertainty=s, depth=np.where(far, fb / D, dtype(0)),
                   valid=far & (s <= max_unc) & (lr <= max_lr))
    assert out['depth'].dtype == dtype and out['disparity'].dtype == dtype
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def empty_state(shape):
    return torch.zeros(shape), torch.full(shape, -1.0)


# ------------------------------------------------------------ planted inputs --
EDGE_STEP = 120   # the darker side's grey level below the brighter side's: > sigma_colour
D_LEFT, D_RIGHT = 40.0, 20.0


def edge_scene(shape, seed, noise=0.5):
    """(disp f32, unc f32, frame u8 [.., 3]) of ``shape`` = (N, H, W): the
    frame has a vertical colour edge at column W // 2, the right side darker by
    EDGE_STEP levels per channel (+- 3 of seeded noise), and the disparity
    jumps there from D_LEFT to D_RIGHT (+- ``noise``); unc uniform in
    (0.02, 0.32)"""
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    right = (torch.arange(w) >= w // 2)[None, None, :].expand(n, h, w)
    base = torch.where(right, 180 - EDGE_STEP, 180)
    frame = (base[..., None] + torch.randint(-3, 4, (n, h, w, 3), generator=g)).to(torch.uint8)
    disp = torch.where(right, D_RIGHT, D_LEFT) + (torch.rand(shape, generator=g) - 0.5) * 2 * noise
    unc = torch.rand(shape, generator=g) * 0.3 + 0.02
    return disp.float().contiguous(), unc.float().contiguous(), frame.contiguous()


BAD = (float('nan'), float('inf'), float('-inf'))


def taps_of(shape, y, x, radius, step):
    """the taps of pixel (y, x) that lie inside an image of ``shape``"""
    _, h, w = shape
    return [(y + j * step, x + i * step) for j in range(-radius, radius + 1)
            for i in range(-radius, radius + 1)
            if 0 <= y + j * step < h and 0 <= x + i * step < w]


def planted(shape, seed, radius, step):
    """edge_scene with, seeded: NaN, +inf and -inf in disp at about 3 % of the
    pixels and in unc at another 3 %, unc = 1e30 (confidence exactly 0) and
    1e12 (tiny) at 2 % each -- and two pixels whose every tap is skipped or
    weightless, so the raw values pass through: ``lone[0]`` (image 0) has +inf
    at the centre and a non-finite disp or unc at every other tap; ``lone[1]``
    (the last image) has unc = 1e30 at every tap, so den = 0 with finite
    values.  -> (disp, unc, frame, lone)"""
    disp, unc, frame = edge_scene(shape, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    n, h, w = shape
    r = torch.rand(shape, generator=g)
    for k, x in enumerate(BAD):
        disp[(r >= 0.01 * k) & (r < 0.01 * (k + 1))] = x
        unc[(r >= 0.03 + 0.01 * k) & (r < 0.03 + 0.01 * (k + 1))] = x
    unc[(r >= 0.06) & (r < 0.08)] = 1e30
    unc[(r >= 0.08) & (r < 0.10)] = 1e12
    lone = [(0, h // 3, w // 4), (n - 1, h - 1 - h // 3, w - 1 - w // 4)]
    if lone[0] == lone[1]:
        lone = lone[:1]
    (n0, y0, x0) = lone[0]
    for q, (y, x) in enumerate(taps_of(shape, y0, x0, radius, step)):
        if q % 2:
            disp[n0, y, x] = BAD[q % 3]
        else:
            unc[n0, y, x] = BAD[q % 3]
    disp[n0, y0, x0] = float('inf')
    unc[n0, y0, x0] = 0.125
    if len(lone) > 1:
        (n1, y1, x1) = lone[1]
        for y, x in taps_of(shape, y1, x1, radius, step):
            if (n1, y, x) != (n0, y0, x0):
                disp[n1, y, x] = D_RIGHT + 0.25 * ((y + x) % 5)
                unc[n1, y, x] = 1e30
    return disp, unc, frame, lone


def sequence(shape, seed, frames=4):
    """``frames`` measurements (disp, unc, lr_error) of a static scene for the
    recursive filter: frame 0 fills the state; from frame 1 on about 5 % of
    the pixels jump by 15 (far past any gate: the reset branch), about 4 % are
    NaN / +-inf in disp or inf in unc (m not finite: the not-fresh branch),
    the rest moves by +- 0.3 (the keep branch); lr_error uniform in (0, 2)"""
    g = torch.Generator().manual_seed(seed)
    base, unc0, _ = edge_scene(shape, seed, noise=0.0)
    out = []
    for t in range(frames):
        d = base + (torch.rand(shape, generator=g) - 0.5) * 0.6
        u = unc0 * (0.8 + 0.4 * torch.rand(shape, generator=g))
        r = torch.rand(shape, generator=g)
        if t > 0:
            d[r < 0.05] += 15.0
        for k, x in enumerate(BAD):
            d[(r >= 0.05 + 0.01 * k) & (r < 0.06 + 0.01 * k)] = x
        u[(r >= 0.08) & (r < 0.09)] = float('inf')
        d.view(-1)[1] = float('nan')  # and one of each branch in the smallest map
        if t > 0:
            d.view(-1)[0] = base.view(-1)[0] + 15.0
            d.view(-1)[2], u.view(-1)[2] = base.view(-1)[2] + 0.1, unc0.view(-1)[2]
        out.append((d.float().contiguous(), u.float().contiguous(),
                    (torch.rand(shape, generator=g) * 2).float()))
    return out


def same_bits(a, b):
    """equal bit for bit (NaN payloads included); bool and uint8 by value"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)
