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
captured graph.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from ._lib import call, ptr, query

INTR_PARAMS = ('fx', 'fy', 'cx', 'cy')


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


def _kind(t):
    return t.dtype if torch.is_tensor(t) else type(t).__name__


def _check_maps(who, depth, valid, uncertainty=None, frame=None):
    """dtype and shape of the inputs -> (N, Hs, Ws); then the device"""
    if not torch.is_tensor(depth) or depth.dtype != torch.float32:
        raise TypeError(f'{who}: depth: f32 tensor expected, got '
                        f'{_kind(depth)}')
    if depth.dim() not in (2, 3) or not depth.is_contiguous() or depth.numel() == 0:
        raise ValueError(f'{who}: depth must be a contiguous, non-empty [H, W] or [N, H, W] map '
                         f'(shape {tuple(depth.shape)}, strides {depth.stride()})')
    shape = tuple(depth.shape)
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f'{who}: valid: bool or uint8 tensor expected, got '
                            f'{_kind(valid)}')
        if tuple(valid.shape) != shape or not valid.is_contiguous():
            raise ValueError(f'{who}: valid: contiguous {shape} expected, got '
                             f'{tuple(valid.shape)} with strides {valid.stride()}')
    if uncertainty is not None:
        if not torch.is_tensor(uncertainty) or uncertainty.dtype != torch.float32:
            raise TypeError(f'{who}: uncertainty: f32 tensor expected, got '
                            f'{_kind(uncertainty)}')
        if tuple(uncertainty.shape) != shape or not uncertainty.is_contiguous():
            raise ValueError(f'{who}: uncertainty: contiguous {shape} expected, got '
                             f'{tuple(uncertainty.shape)} with strides {uncertainty.stride()}')
    if frame is not None:
        if not torch.is_tensor(frame) or frame.dtype != torch.uint8:
            raise TypeError(f'{who}: frame: uint8 tensor expected, got '
                            f'{_kind(frame)}')
        if tuple(frame.shape) != shape + (3,) or not frame.is_contiguous():
            raise ValueError(f'{who}: frame: contiguous {shape + (3,)} expected, got '
                             f'{tuple(frame.shape)} with strides {frame.stride()}')
    n = shape[0] if len(shape) == 3 else 1
    if n * shape[-2] > 2 ** 31 - 1:
        raise ValueError(f'{who}: {n} x {shape[-2]} rows, at most 2^31 - 1')
    return n, shape[-2], shape[-1]


def _check_device(who, depth, **others):
    L.require_device(depth)
    for name, t in others.items():
        if t is not None and t.device != depth.device:
            raise L.UmamdError(f'{who}: {name} on {t.device}, depth on {depth.device}')


def _u8(valid):
    return valid.view(torch.uint8) if valid is not None and valid.dtype == torch.bool else valid


def backproject(depth: torch.Tensor, intrinsics, valid=None) -> torch.Tensor:
    """``depth`` (f32, contiguous [H, W] or [N, H, W], on the device) -> the
    organised map, f32 ``depth.shape + (3,)``: (X, Y, Z) where ``valid`` (bool
    or uint8 of ``depth``'s shape; None: everywhere), (0, 0, 0) elsewhere.
    Runs on the current stream, never synchronises."""
    who = 'umamd.points.backproject'
    intr = check_intrinsics(intrinsics, who)
    n, hs, ws = _check_maps(who, depth, valid)
    _check_device(who, depth, valid=valid)
    dev = depth.device
    with torch.cuda.device(dev):
        xyz = torch.empty(tuple(depth.shape) + (3,), dtype=torch.float32, device=dev)
        block = torch.tensor(intr, dtype=torch.float32).to(dev)
        call('um_depth_backproject', ptr(depth), ptr(_u8(valid)), n, hs, ws, ptr(block), ptr(xyz))
    return xyz


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
    capacity = n * -(-hs // stride) * -(-ws // stride)
    if capacity > 2 ** 31 - 1:
        raise ValueError(f'{who}: {capacity} lattice sites, at most 2^31 - 1')
    _check_device(who, depth, valid=valid, uncertainty=uncertainty, frame=frame)
    dev = depth.device
    with torch.cuda.device(dev):
        work = torch.empty(query('um_depth_cloud_ws', n, hs, ws, stride), dtype=torch.uint8,
                           device=dev)
        xyzu = torch.empty((capacity, 4), dtype=torch.float32, device=dev)
        rgba = None if frame is None else torch.empty((capacity, 4), dtype=torch.uint8, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
        block = torch.tensor(intr, dtype=torch.float32).to(dev)
        call('um_depth_cloud', ptr(depth), ptr(_u8(valid)), ptr(uncertainty), ptr(frame), n, hs,
             ws, stride, ptr(block), ptr(work), ptr(xyzu), ptr(rgba), ptr(offsets))
    return xyzu, rgba, offsets


def split(xyzu: torch.Tensor, rgba, offsets: torch.Tensor) -> list:
    """one ``(xyzu_n, rgba_n)`` pair of views per image (``rgba_n`` None
    without colours); reads ``offsets`` once -- the only synchronisation of
    the point stage"""
    o = offsets.tolist()
    return [(xyzu[a:b], None if rgba is None else rgba[a:b]) for a, b in zip(o[:-1], o[1:])]
