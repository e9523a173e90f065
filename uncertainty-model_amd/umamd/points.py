"""3-D points on the device: a depth map back-projected through pinhole
intrinsics into an organised map and a packed, coloured cloud (csrc/points.hip,
include/umamd.h "deployment").

For pixel (row v, column u) of a depth map, with ``intrinsics = (fx, fy, cx,
cy)`` in pixels of that map, each step its own f32 operation:

  Z = depth[v, u];  X = ((u - cx) * Z) / fx;  Y = ((v - cy) * Z) / fy

The pixel centre sits at the integer coordinate (no half-pixel shift: with the
other convention pass ``cx - 0.5, cy - 0.5``).

  backproject(depth, intrinsics, valid)   f32 depth.shape + (3,)
  cloud(depth, intrinsics, ...)           (xyzu, rgba or None, offsets)
  split(xyzu, rgba, offsets)              one (xyzu_n, rgba_n) per image

``umamd.deploy.DepthPipeline(points=...)`` runs the same entries inside its
captured graph: ``PointStage`` is that stage.
"""
from __future__ import annotations

import math

import torch

from ._lib import call, check_same_device, check_tensor, ptr, query, write_block

INTR_PARAMS = ('fx', 'fy', 'cx', 'cy')
POINTS = ('map', 'cloud', 'both')


def check_intrinsics(intrinsics, who: str = 'umamd.points') -> tuple:
    """(fx, fy, cx, cy) as floats: four finite numbers, fx and fy not 0;
    ValueError otherwise"""
    try:
        vals = tuple(intrinsics)
    except TypeError:
        raise ValueError(f'{who}: intrinsics={intrinsics!r}: (fx, fy, cx, cy) expected') from None
    if len(vals) != 4:
        raise ValueError(f'{who}: intrinsics={intrinsics!r}: (fx, fy, cx, cy) expected')
    for k, v in zip(INTR_PARAMS, vals):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f'{who}: intrinsics: {k}={v!r}: a finite number expected')
    if vals[0] == 0 or vals[1] == 0:
        raise ValueError(f'{who}: intrinsics: fx={vals[0]} fy={vals[1]}: a focal length of 0')
    return tuple(float(v) for v in vals)


def check_stride(stride, who: str = 'umamd.points', name: str = 'stride') -> int:
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError(f'{who}: {name}={stride!r}: an integer >= 1 expected')
    return stride


def _check_maps(who, depth, valid, uncertainty=None, frame=None):
    """dtype and shape of the inputs -> (N, Hs, Ws)"""
    check_tensor(who, 'depth', depth, (torch.float32,), 'f32')
    if depth.dim() not in (2, 3) or not depth.is_contiguous() or depth.numel() == 0:
        raise ValueError(f'{who}: depth must be a contiguous, non-empty [H, W] or [N, H, W] map '
                         f'(shape {tuple(depth.shape)}, strides {depth.stride()})')
    shape = tuple(depth.shape)
    if valid is not None:
        check_tensor(who, 'valid', valid, (torch.bool, torch.uint8), 'bool or uint8', shape)
    if uncertainty is not None:
        check_tensor(who, 'uncertainty', uncertainty, (torch.float32,), 'f32', shape)
    if frame is not None:
        check_tensor(who, 'frame', frame, (torch.uint8,), 'uint8', shape + (3,))
    n = shape[0] if len(shape) == 3 else 1
    if n * shape[-2] > 2 ** 31 - 1:
        raise ValueError(f'{who}: {n} x {shape[-2]} rows, at most 2^31 - 1')
    return n, shape[-2], shape[-1]


def _capacity(n, hs, ws, stride):
    """the lattice sites of a batch: the rows of a cloud's buffers"""
    return n * -(-hs // stride) * -(-ws // stride)


def _u8(valid):
    return valid.view(torch.uint8) if valid is not None and valid.dtype == torch.bool else valid


def _block(intr, dev):
    return torch.tensor(intr, dtype=torch.float32).to(dev)


def _backproject(depth, valid, n, hs, ws, block, xyz):
    """um_depth_backproject on the current stream; no checks"""
    call('um_depth_backproject', ptr(depth), ptr(valid), n, hs, ws, ptr(block), ptr(xyz))
    return xyz


def _cloud_buffers(new, dev, n, hs, ws, stride, rgba=True):
    """(xyzu, rgba or None, offsets, work) of a cloud, made by ``new``
    (torch.empty or torch.zeros)"""
    capacity = _capacity(n, hs, ws, stride)
    return (new((capacity, 4), dtype=torch.float32, device=dev),
            new((capacity, 4), dtype=torch.uint8, device=dev) if rgba else None,
            new(n + 1, dtype=torch.int32, device=dev),
            new(query('um_depth_cloud_ws', n, hs, ws, stride), dtype=torch.uint8, device=dev))


def _cloud(depth, valid, uncertainty, frame, n, hs, ws, stride, block, buffers):
    """um_depth_cloud on the current stream into ``buffers`` -> (xyzu, rgba,
    offsets); no checks"""
    xyzu, rgba, offsets, work = buffers
    call('um_depth_cloud', ptr(depth), ptr(valid), ptr(uncertainty), ptr(frame), n, hs, ws,
         stride, ptr(block), ptr(work), ptr(xyzu), ptr(rgba), ptr(offsets))
    return xyzu, rgba, offsets


def backproject(depth: torch.Tensor, intrinsics, valid=None) -> torch.Tensor:
    """``depth`` (f32, contiguous [H, W] or [N, H, W], on the device) -> the
    organised map, f32 ``depth.shape + (3,)``: (X, Y, Z) where ``valid`` (bool
    or uint8 of ``depth``'s shape; None: everywhere), (0, 0, 0) elsewhere.
    Runs on the current stream, never synchronises."""
    who = 'umamd.points.backproject'
    intr = check_intrinsics(intrinsics, who)
    n, hs, ws = _check_maps(who, depth, valid)
    check_same_device(who, 'depth', depth, valid=valid)
    dev = depth.device
    with torch.cuda.device(dev):
        xyz = torch.empty(tuple(depth.shape) + (3,), dtype=torch.float32, device=dev)
        return _backproject(depth, _u8(valid), n, hs, ws, _block(intr, dev), xyz)


def cloud(depth: torch.Tensor, intrinsics, valid=None, uncertainty=None, frame=None,
          stride: int = 1):
    """The packed cloud of the kept pixels (``valid``; None: all) on the
    lattice ``v % stride == 0 and u % stride == 0``, image-major then
    row-major -> ``(xyzu, rgba, offsets)`` on the device:

    ``xyzu`` f32 [capacity, 4], rows (X, Y, Z, ``uncertainty`` at the pixel; 0
    without it); ``rgba`` uint8 [capacity, 4], rows (r, g, b, 255) of ``frame``
    (uint8 ``depth.shape + (3,)``), None without it; ``offsets`` int32 [N + 1]:
    image n owns rows ``offsets[n]:offsets[n + 1]``.  ``capacity`` is the number
    of lattice sites; the rows from ``offsets[N]`` on are UNSPECIFIED (never
    written).  Runs on the current stream and never synchronises: ``split``
    reads the offsets."""
    who = 'umamd.points.cloud'
    intr = check_intrinsics(intrinsics, who)
    stride = check_stride(stride, who)
    n, hs, ws = _check_maps(who, depth, valid, uncertainty, frame)
    capacity = _capacity(n, hs, ws, stride)
    if capacity > 2 ** 31 - 1:
        raise ValueError(f'{who}: {capacity} lattice sites, at most 2^31 - 1')
    check_same_device(who, 'depth', depth, valid=valid, uncertainty=uncertainty, frame=frame)
    dev = depth.device
    with torch.cuda.device(dev):
        return _cloud(depth, _u8(valid), uncertainty, frame, n, hs, ws, stride, _block(intr, dev),
                      _cloud_buffers(torch.empty, dev, n, hs, ws, stride, rgba=frame is not None))


def split(xyzu: torch.Tensor, rgba, offsets: torch.Tensor) -> list:
    """one ``(xyzu_n, rgba_n)`` pair of views per image (``rgba_n`` None
    without colours); reads ``offsets`` once -- the only synchronisation of
    the point stage"""
    o = offsets.tolist()
    return [(xyzu[a:b], None if rgba is None else rgba[a:b]) for a, b in zip(o[:-1], o[1:])]


class PointStage:
    """The point stage of ``umamd.deploy.DepthPipeline``: its arguments,
    checked on the host, its buffers, its launches and its outputs."""

    keys = INTR_PARAMS  # of ``params`` and ``block``: what set_params takes

    def __init__(self, points, intrinsics, point_stride):
        who = 'DepthPipeline'
        if not isinstance(points, str) or points not in POINTS:
            raise ValueError(f'{who}: points={points!r}: None or one of {POINTS}')
        if intrinsics is None:
            raise ValueError(f'{who}: points={points!r} needs intrinsics=(fx, fy, cx, cy) in '
                             f'source pixels')
        self.params = dict(zip(INTR_PARAMS, check_intrinsics(intrinsics, who)))
        self.stride = check_stride(point_stride, who, 'point_stride')
        if self.stride != 1 and points == 'map':
            raise ValueError(f"{who}: point_stride={self.stride} with points='map': the "
                             f"organised map has every pixel (the stride thins the cloud)")
        self.mode = points

    def allocate(self, dev, B, Hs, Ws):
        self._size = (B, Hs, Ws)
        self.block = _block(tuple(self.params.values()), dev)
        if self.mode in ('map', 'both'):
            self._xyz = torch.zeros((B, Hs, Ws, 3), dtype=torch.float32, device=dev)
        if self.mode in ('cloud', 'both'):
            self._cloud = _cloud_buffers(torch.zeros, dev, B, Hs, Ws, self.stride)

    def run(self, maps, frames):
        """``maps``: the pipeline's disparity, depth, uncertainty, lr_error and
        valid (uint8) buffers; ``frames`` the frame they were computed from"""
        if self.mode in ('map', 'both'):
            _backproject(maps['depth'], maps['valid'], *self._size, self.block, self._xyz)
        if self.mode in ('cloud', 'both'):
            _cloud(maps['depth'], maps['valid'], maps['uncertainty'], frames, *self._size,
                   self.stride, self.block, self._cloud)

    def outputs(self):
        out = {}
        if self.mode in ('map', 'both'):
            out['xyz'] = self._xyz
        if self.mode in ('cloud', 'both'):
            out.update(zip(('cloud_xyzu', 'cloud_rgba', 'cloud_offsets'), self._cloud))
        return out

    def check_params(self, kw):
        """the stage's part of set_params, checked (nothing is written yet)"""
        new = [kw.get(k, self.params[k]) for k in INTR_PARAMS]
        return dict(zip(INTR_PARAMS, check_intrinsics(new, 'DepthPipeline.set_params')))

    def write(self, checked):
        """``checked`` into the host dict and the device block, in place"""
        write_block(self.block, self.params, self.keys, checked)
