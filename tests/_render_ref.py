"""References of the display stage (csrc/render.hip, umamd/render.py): the
definition of um_depth_render in include/umamd.h restated op for op in f32
torch on the CPU, the masked min/max of um_value_range, the table rule, and
the special values the tests plant."""
import numpy as np
import torch


def lut_rule(name):
    """floor(cmap(arange(256))[:, :3] * 255 + 0.5) of a matplotlib colour map:
    uint8 [256, 3]"""
    import matplotlib.pyplot as plt
    t = np.floor(plt.get_cmap(name)(np.arange(256))[:, :3] * 255 + 0.5).astype(np.uint8)
    return torch.from_numpy(t)


def alpha_q(x):
    """q(x) = (int)(clamp(x, 0, 1) * 256 + 0.5) in f32, q(NaN) = 0"""
    x = torch.tensor(float(x), dtype=torch.float32)
    if bool(torch.isnan(x)):
        return 0
    return int((x.clamp(0, 1) * 256 + 0.5).to(torch.int32))


def blend(c, f, a):
    """(c * a + f * (256 - a) + 128) >> 8 per channel; c, f integer tensors,
    a an integer tensor broadcastable to them"""
    return (c * a + f * (256 - a) + 128) >> 8


def render_ref(value, lut, lo, hi, opacity=1.0, invalid_opacity=0.0, valid=None, frame=None,
               inverse=False):
    """value f32 [...] -> uint8 [..., 3].  lo, hi: floats or 0-dim f32 tensors
    (taken to f32, as the device block holds them)"""
    v = value.detach().cpu().to(torch.float32)
    lo = torch.as_tensor(lo).to(torch.float32)
    hi = torch.as_tensor(hi).to(torch.float32)
    t = (v - lo) / (hi - lo)
    if inverse:
        t = 1 - t
    s = t * 256
    nan = torch.isnan(s)
    idx = torch.where(s < 0, torch.zeros_like(s), torch.clamp(s, max=255.0))
    idx = torch.where(nan, torch.zeros_like(s), idx).to(torch.int64)  # truncates
    c = lut.cpu().to(torch.int32)[idx]
    c[nan] = 0
    a_ok, a_bad = alpha_q(opacity), alpha_q(invalid_opacity)
    if valid is None:
        a = torch.full(v.shape, a_ok, dtype=torch.int32)
    else:
        ok = valid.detach().cpu() != 0
        a = torch.where(ok, torch.tensor(a_ok, dtype=torch.int32),
                        torch.tensor(a_bad, dtype=torch.int32))
    f = torch.zeros_like(c) if frame is None else frame.detach().cpu().to(torch.int32)
    return blend(c, f, a.unsqueeze(-1)).to(torch.uint8)


def value_range_ref(value, valid=None):
    """(lo, hi) of the valid, non-NaN pixels as an f32 [2] tensor; none:
    (+inf, -inf)"""
    v = value.detach().cpu().to(torch.float32)
    m = ~torch.isnan(v)
    if valid is not None:
        m &= valid.detach().cpu() != 0
    if not bool(m.any()):
        return torch.tensor([float('inf'), float('-inf')])
    return torch.stack([v[m].min(), v[m].max()])


def planted(shape, seed, lo=0.0, hi=1.0):
    """f32 values over [lo - 0.1 w, hi + 0.1 w] (w = hi - lo) with the special
    values planted at fixed places: the bin edges lo + w k / 256, both ends,
    -0.0, the first f32 above 1 (in units of the range), NaN and +-inf"""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    w = hi - lo
    v = (torch.rand(n, generator=g) * 1.2 - 0.1) * w + lo
    special = [lo + w * k / 256 for k in range(257)] + \
        [lo, hi, -0.0, lo + w * 1.0000001, float('nan'), float('inf'), float('-inf')]
    special = torch.tensor(special, dtype=torch.float32)
    if n >= 2 * len(special):
        pos = torch.randperm(n, generator=g)[:len(special)]
        v[pos] = special
    else:  # a tiny map: the last few special values
        k = min(n, 7)
        v[:k] = special[-k:]
    return v.view(shape)
