"""Rectification on the device: a raw camera frame undistorted and
stereo-rectified into the pinhole image the rest of the deployment path
assumes (csrc/rectify.hip, include/umamd.h "rectification").

For every pixel (row v, column u) of the rectified image a source coordinate
(mx, my) in the raw frame is found -- from a ``Calibration`` (pinhole +
Brown-Conrady in the arrangement of OpenCV's initUndistortRectifyMap, computed
inside the kernel in f32) or from a ``RemapTable`` (any map the user already
has) -- rounded to 1/32 pixel and sampled bilinearly in integer arithmetic with
border value 0.  Same model as OpenCV, own rounding: the header fixes every
step, the result is not bit-equal to cv2.remap.  The pixel centre sits at the
integer coordinate, as in umamd.points.

  Calibration(K, dist, R=None, P=None, size=None, baseline=None)
  RemapTable(map_x, map_y)
  rectify(frames, how, out=None, inside=None)  -> (rectified, inside)

``umamd.deploy.DepthPipeline(rectify=...)`` runs the same entry as stage 0 of
its captured graph (``RectifyStage``).  Not built: R and P from stereo extrinsics (stereoRectify),
fisheye and thin-prism models (use a RemapTable), bicubic sampling.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, check_same_device, check_tensor, ptr

OUT = -2 ** 31  # the Q5 coordinate of a source position that is not finite or past 2^20
MAX_SRC = 32767  # largest raw height / width (include/umamd.h)
INT_MAX = 2 ** 31 - 1


def q5(c) -> np.ndarray:
    """the Q5 fixed point of f32 coordinates: (int)rint(c * 32) where c is
    finite and |c| < 2^20, else OUT (numpy int32)"""
    c = np.asarray(c, np.float32)
    with np.errstate(all='ignore'):
        ok = np.abs(c) < np.float32(2 ** 20)  # False for NaN and inf
        q = np.rint(np.where(ok, c, np.float32(0)) * np.float32(32)).astype(np.int32)
    return np.where(ok, q, np.int32(OUT)).astype(np.int32)


def _numbers(who, name, x, shapes):
    """x as an f64 array of one of ``shapes``, all finite; ValueError otherwise"""
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    try:
        a = np.asarray(x)
        if a.dtype == bool or a.dtype.kind not in 'iuf':
            raise TypeError
        a = a.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: {name}={x!r}: numbers expected') from None
    if a.shape not in shapes:
        raise ValueError(f'{who}: {name} of shape {a.shape}: one of {shapes} expected')
    if not np.isfinite(a).all():
        raise ValueError(f'{who}: {name} must be finite, got {a.tolist()}')
    return a


def _camera(who, name, x, shapes):
    """a camera matrix given as 3x3 (3x4) or (fx, fy, cx, cy) -> 3x3 f64"""
    a = _numbers(who, name, x, shapes)
    if a.shape == (4,):
        fx, fy, cx, cy = a
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    return a[:, :3].copy()


def _size(who, name, size):
    try:
        h, w = size
        ok = all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in (h, w))
    except (TypeError, ValueError):
        ok = False
    if not ok or h < 2 or w < 2:
        raise ValueError(f'{who}: {name}={size!r}: (height, width), integers >= 2 expected')
    return int(h), int(w)


class Calibration:
    """One camera of a calibrated rig: ``K`` the raw camera matrix (3x3 or
    ``(fx, fy, cx, cy)``), ``dist`` 4, 5 or 8 distortion coefficients in
    OpenCV's order ``(k1, k2, p1, p2[, k3[, k4, k5, k6]])``, ``R`` the 3x3
    rectifying rotation (default: identity), ``P`` the rectified camera (3x3,
    3x4 or ``(fx', fy', cx', cy')``; default: ``K``), ``size = (Hr, Wr)`` of the
    rectified image (default: the raw size at use) and the stereo ``baseline``.
    ``R`` and ``P`` are what the rig's calibration (OpenCV's stereoRectify: R1,
    P1) delivers; they are not computed here.

    ``block()`` is the 24-float device block of um_frame_rectify,
    ``intrinsics`` the rectified ``(fx', fy', cx', cy')`` for
    ``DepthPipeline(intrinsics=)``, ``focal_baseline`` is ``fx' * baseline``
    for ``focal_baseline=``.  Everything is checked here, on the host."""

    mode = 'analytic'

    def __init__(self, K, dist, R=None, P=None, size=None, baseline=None):
        who = 'Calibration'
        k = _camera(who, 'K', K, ((3, 3), (4,)))
        d = _numbers(who, 'dist', dist, ((4,), (5,), (8,)))
        r = np.eye(3) if R is None else _numbers(who, 'R', R, ((3, 3),))
        p = k.copy() if P is None else _camera(who, 'P', P, ((3, 3), (3, 4), (4,)))
        if k[0, 0] == 0 or k[1, 1] == 0:
            raise ValueError(f'{who}: K: fx={k[0, 0]} fy={k[1, 1]}: a focal length of 0')
        if p[0, 0] * p[1, 1] == 0:
            raise ValueError(f"{who}: P: fx'={p[0, 0]} fy'={p[1, 1]}: a focal length of 0")
        a = p @ r
        if not abs(np.linalg.det(a)) > 1e-12 * max(np.abs(a).max(), 1.0) ** 3:
            raise ValueError(f'{who}: P[:, :3] @ R is not invertible (det {np.linalg.det(a):g})')
        m = np.linalg.inv(a)
        if not np.isfinite(m).all():
            raise ValueError(f'{who}: P[:, :3] @ R is not invertible')
        self.size = None if size is None else _size(who, 'size', size)
        if baseline is not None:
            baseline = float(_numbers(who, 'baseline', baseline, ((),)))
        self.baseline = baseline
        self.K, self.R, self.P = k, r, p
        self.dist = np.concatenate([d, np.zeros(8 - len(d))])
        k1, k2, p1, p2, k3, k4, k5, k6 = self.dist
        self._block = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2], k1, k2, p1, p2, k3, k4, k5,
                                k6, *m.reshape(-1), 0, 0, 0], np.float64).astype(np.float32)
        if not np.isfinite(self._block).all():
            raise ValueError(f'{who}: a value does not fit f32')

    def block(self) -> np.ndarray:
        """f32[24] = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, m0..m8, 0,
        0, 0) with m = inv(P[:, :3] @ R), made in f64 and rounded"""
        return self._block.copy()

    @property
    def intrinsics(self) -> tuple:
        p = self.P
        return float(p[0, 0]), float(p[1, 1]), float(p[0, 2]), float(p[1, 2])

    @property
    def focal_baseline(self) -> float:
        if self.baseline is None:
            raise ValueError('Calibration.focal_baseline: built without baseline=')
        return float(self.P[0, 0]) * self.baseline

    def out_size(self, raw):
        """(Hr, Wr) for raw frames of size ``raw`` = (Hs, Ws)"""
        return self.size if self.size is not None else (int(raw[0]), int(raw[1]))

    def data(self, device=None) -> torch.Tensor:
        """the block as a tensor (on ``device`` if given)"""
        t = torch.from_numpy(self._block.copy())
        return t if device is None else t.to(device)


class RemapTable:
    """A ready map: ``map_x`` and ``map_y``, float arrays or tensors [Hr, Wr]
    holding for every rectified pixel the source column and row (taken as f32;
    the convention of cv2.remap's map1 / map2).  ``table(device)`` is the Q5
    int32 [Hr, Wr, 2] of um_frame_rectify: ``q5`` of both, NaN, inf and
    anything past 2^20 become OUT (a black pixel outside the mask)."""

    mode = 'table'

    def __init__(self, map_x, map_y):
        who = 'RemapTable'
        maps = []
        for name, m in (('map_x', map_x), ('map_y', map_y)):
            if torch.is_tensor(m):
                m = m.detach().cpu().numpy()
            m = np.asarray(m)
            if m.dtype.kind != 'f':
                raise TypeError(f'{who}: {name}: a float array or tensor expected, got {m.dtype}')
            if m.ndim != 2 or m.shape[0] < 2 or m.shape[1] < 2:
                raise ValueError(f'{who}: {name} of shape {m.shape}: [Hr, Wr] with both >= 2 '
                                 f'expected')
            maps.append(m.astype(np.float32))
        if maps[0].shape != maps[1].shape:
            raise ValueError(f'{who}: map_x {maps[0].shape} and map_y {maps[1].shape} differ')
        self.size = tuple(int(s) for s in maps[0].shape)
        self._table = np.ascontiguousarray(np.stack([q5(maps[0]), q5(maps[1])], -1))

    def out_size(self, raw):
        return self.size

    def table(self, device=None) -> torch.Tensor:
        t = torch.from_numpy(self._table.copy())
        return t if device is None else t.to(device)

    data = table


def check_how(how, who: str):
    if not isinstance(how, (Calibration, RemapTable)):
        raise TypeError(f'{who}: a Calibration or a RemapTable expected, got '
                        f'{type(how).__name__}')
    return how


def check_sizes(who: str, n: int, hs: int, ws: int, hr: int, wr: int):
    """the limits of um_frame_rectify; ValueError before any GPU work"""
    if hs < 2 or ws < 2 or hs > MAX_SRC or ws > MAX_SRC:
        raise ValueError(f'{who}: raw size {hs}x{ws}: height and width from 2 to {MAX_SRC}')
    if hr < 2 or wr < 2:
        raise ValueError(f'{who}: rectified size {hr}x{wr}: height and width at least 2')
    if n < 1 or n * hr * wr > INT_MAX:
        raise ValueError(f'{who}: {n} x {hr} x {wr} output pixels: from 1 to 2^31 - 1')


def _remap(frames, mode, data, out, inside):
    """um_frame_rectify on the current stream: ``frames`` [B, Hs, Ws, 3] ->
    ``out`` [B, Hr, Wr, 3] and ``inside`` [Hr, Wr] through ``data``, the block
    (``mode`` 'analytic') or the Q5 table ('table') on the device; no checks"""
    b, hs, ws, _ = frames.shape
    cal, table = (data, None) if mode == 'analytic' else (None, data)
    call('um_frame_rectify', ptr(frames), b, hs, ws, out.shape[1], out.shape[2], ptr(cal),
         ptr(table), ptr(out), ptr(inside))
    return out, inside


def rectify(frames: torch.Tensor, how, out=None, inside=None):
    """``frames`` uint8 [B, Hs, Ws, 3], contiguous, on the device -> ``(rectified
    uint8 [B, Hr, Wr, 3], inside uint8 [Hr, Wr])``: the frames sampled at the
    source coordinates of ``how`` (a Calibration or a RemapTable), 0 where the
    source lies outside the raw frame, and the mask of the pixels whose source
    lies inside it.  ``out`` / ``inside``: buffers to fill (same shapes, uint8,
    contiguous, on the frames' device).  Runs on the current stream, never
    synchronises."""
    who = 'umamd.rectify.rectify'
    check_how(how, who)
    check_tensor(who, 'frames', frames, (torch.uint8,), 'uint8')
    if frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f'{who}: frames must be a contiguous [B, Hs, Ws, 3] batch (shape '
                         f'{tuple(frames.shape)}, strides {frames.stride()})')
    b, hs, ws, _ = frames.shape
    hr, wr = how.out_size((hs, ws))
    check_sizes(who, b, hs, ws, hr, wr)
    for name, t, shape in (('out', out, (b, hr, wr, 3)), ('inside', inside, (hr, wr))):
        if t is not None:
            check_tensor(who, name, t, (torch.uint8,), 'uint8', shape)
    check_same_device(who, 'frames', frames, out=out, inside=inside)
    dev = frames.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((b, hr, wr, 3), dtype=torch.uint8, device=dev)
        if inside is None:
            inside = torch.empty((hr, wr), dtype=torch.uint8, device=dev)
        return _remap(frames, how.mode, how.data(dev), out, inside)


class RectifyStage:
    """Stage 0 of ``umamd.deploy.DepthPipeline``: ``how`` and the sizes, checked
    on the host, its buffers, its two launches and its outputs."""

    def __init__(self, how, batch, raw_height, raw_width):
        self.how = check_how(how, 'DepthPipeline: rectify')
        self.raw = (raw_height, raw_width)
        self.size = tuple(how.out_size(self.raw))
        if batch >= 1:  # the pipeline refuses another batch after its size checks
            check_sizes('DepthPipeline: rectify', batch, *self.raw, *self.size)

    def allocate(self, dev, B, Hs, Ws):
        """(Hs, Ws): the rectified size, as for every later stage"""
        self.raw_frames = torch.zeros((B,) + self.raw + (3,), dtype=torch.uint8, device=dev)
        self.frames = torch.zeros((B, Hs, Ws, 3), dtype=torch.uint8, device=dev)
        self._inside = torch.zeros((Hs, Ws), dtype=torch.uint8, device=dev)
        self._data = self.how.data(dev)  # the f32[24] block or the Q5 table

    def before_prep(self):
        _remap(self.raw_frames, self.how.mode, self._data, self.frames, self._inside)

    def after_post(self, valid):
        """valid &= inside: the display and point stages see the combined mask"""
        call('um_valid_and', ptr(valid), ptr(self._inside), valid.shape[0], self._inside.numel())

    def outputs(self):
        return {'frame': self.frames, 'inside': self._inside.view(torch.bool)}

    def set_calibration(self, how):
        who = 'DepthPipeline.set_calibration'
        check_how(how, who)
        if how.mode != self.how.mode:
            raise ValueError(f'{who}: a {type(how).__name__} on a pipeline built with a '
                             f'{type(self.how).__name__}: build another pipeline')
        size = tuple(how.out_size(self.raw))
        if size != self.size:
            raise ValueError(f'{who}: rectified size {size}, the pipeline was built for '
                             f'{self.size}: build another pipeline')
        self._data.copy_(how.data(None))
        self.how = how
