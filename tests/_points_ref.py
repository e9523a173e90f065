"""References of the point stage (csrc/points.hip, umamd/points.py): the
definition of um_depth_backproject and um_depth_cloud in include/umamd.h
restated op for op in numpy f32 -- every step one exactly rounded f32
operation, so the device result equals it bit for bit -- and the inputs the
tests plant."""
import numpy as np
import torch


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _xyz(depth, intr, dtype):
    """(X, Y, Z) of every pixel of depth [N, H, W] in ``dtype``, nothing zeroed"""
    z = _np(depth).astype(dtype)
    fx, fy, cx, cy = (dtype(np.float32(x)) for x in intr)  # the device block is f32
    n, h, w = z.shape
    u = np.arange(w).astype(dtype)[None, None, :]
    v = np.arange(h).astype(dtype)[None, :, None]
    with np.errstate(all='ignore'):
        x = ((u - cx) * z) / fx  # sub, mul, div: three operations
        y = ((v - cy) * z) / fy
    out = np.stack([x, y, z], -1)
    assert out.dtype == dtype
    return out


def _kept(depth, valid):
    shape = tuple(_np(depth).shape)
    return np.ones(shape, bool) if valid is None else _np(valid).view(np.uint8) != 0


def backproject_ref(depth, intr, valid=None, dtype=np.float32):
    """the organised map: depth [N, H, W] -> torch f32 [N, H, W, 3], (0, 0, 0)
    where valid == 0 whatever depth holds there"""
    xyz = _xyz(depth, intr, dtype)
    xyz[~_kept(depth, valid)] = 0
    return torch.from_numpy(xyz)


def cloud_ref(depth, intr, valid=None, uncertainty=None, frame=None, stride=1,
              dtype=np.float32):
    """the packed cloud: the kept sites of the lattice [::stride, ::stride] in
    np.nonzero's order (image-major, then row-major) -> (xyzu [K, 4], rgba
    [K, 4] or None, offsets int32 [N + 1]) as torch tensors, K the total"""
    s = stride
    xyz = _xyz(depth, intr, dtype)[:, ::s, ::s]
    kept = _kept(depth, valid)[:, ::s, ::s]
    idx = np.nonzero(kept)
    if uncertainty is None:
        fourth = np.zeros(len(idx[0]), dtype)
    else:
        fourth = _np(uncertainty).astype(dtype)[:, ::s, ::s][idx]
    xyzu = np.concatenate([xyz[idx], fourth[:, None]], 1)
    rgba = None
    if frame is not None:
        rgb = _np(frame)[:, ::s, ::s][idx]
        rgba = torch.from_numpy(np.concatenate([rgb, np.full((len(rgb), 1), 255, np.uint8)], 1))
    counts = kept.reshape(kept.shape[0], -1).sum(1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return torch.from_numpy(xyzu), rgba, torch.from_numpy(offsets)


INTR = (517.3, 516.5, 63.25, 31.75)  # fx, fy, cx, cy


def planted(shape, seed, keep=0.6):
    """(depth f32, valid u8, uncertainty f32, frame u8 [.., 3]) of ``shape`` =
    (N, H, W): depth uniform in (0.5, 50); about ``keep`` of the pixels valid;
    NaN, +-inf and negative depths planted ONLY where valid == 0 (four of
    every six invalid pixels), so nothing of them may reach an output"""
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(shape, generator=g) * 49.5 + 0.5
    valid = (torch.rand(shape, generator=g) < keep).to(torch.uint8)
    unc = torch.rand(shape, generator=g) * 0.3
    frame = torch.randint(0, 256, tuple(shape) + (3,), generator=g, dtype=torch.uint8)
    bad = (valid.view(-1) == 0).nonzero().view(-1)
    flat = depth.view(-1)
    for k, x in enumerate((float('nan'), float('inf'), float('-inf'), -3.0)):
        flat[bad[k::6]] = x
    return depth, valid, unc, frame
