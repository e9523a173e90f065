"""Frame-to-depth pipeline: a uint8 camera frame in, metric depth with a
confidence mask out, as one replayed HIP graph around the inference engine.

``InferenceEngine`` maps a resized f32 [B,3,H,W] image to disparity (as a
fraction of the width) and uncertainty at model resolution.  ``DepthPipeline``
adds both ends of the deployment path,

  um_frame_prep   uint8 [B,Hs,Ws,3] -> the engine's static f32 input
                  (ResizeImage -> ToTensor, reference train/transforms.py:
                  15-41: Pillow's bilinear resize, bit-exact, one launch)
  -> forward      (umamd.infer.InferenceEngine: folded BatchNorm, packed weights)
  -> um_depth_post  at the frame's size, left view: disparity in pixels,
                  depth = focal x baseline / disparity, the upsampled
                  uncertainty, the left-right consistency error and the
                  validity mask (include/umamd.h "deployment")
  -> um_depth_render  only with ``render=``: one of the maps coloured and
                  blended over the frame, uint8 [B,Hs,Ws,3] (umamd/render.py;
                  after um_value_range with ``render_range='auto'``)
  -> um_depth_backproject / um_depth_cloud  only with ``points=``: the depth
                  back-projected through the camera intrinsics into an
                  organised [B,Hs,Ws,3] map and / or a packed, coloured cloud
                  (umamd/points.py; after um_depth_post, independent of the
                  display stage)

captured as ONE torch.cuda.CUDAGraph over static buffers.  ``__call__``
copies the frames in and replays; it never synchronises with the host.  The
calibration and the three thresholds live in a 4-float device block the kernel
reads, so ``set_params`` needs no recapture; the display stage has a block of
its own (range and opacities) and so has the point stage (the intrinsics).

With ``rectify=`` a stage 0 runs in front, in the same graph (umamd/rectify.py):

  um_frame_rectify  the RAW uint8 frame [B,Hs,Ws,3] undistorted and
                  stereo-rectified into the uint8 [B,Hr,Wr,3] frame that every
                  stage above reads, plus the mask of the pixels whose source
                  lies inside the raw frame
  um_valid_and    straight after um_depth_post: valid &= inside, so the display
                  and point stages see the combined mask

The calibration block (or the table) is read by the kernel too:
``set_calibration`` needs no recapture.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from . import points as P
from . import rectify as Q
from . import render as R
from ._lib import call, ptr, query
from .imageprep import resize_coeffs
from .infer import InferenceEngine, _eval_mode

PARAMS = ('focal_baseline', 'min_disparity', 'max_uncertainty', 'max_lr_error')
RENDERS = ('disparity', 'depth', 'uncertainty', 'lr_error')
POINTS = ('map', 'cloud', 'both')


def _check_render(render, colour_map, render_range, opacity, invalid_opacity):
    """the display stage's arguments -> (table, (lo, hi) or None for 'auto',
    opacity, invalid_opacity); raises before any GPU work"""
    if not isinstance(render, str) or render not in RENDERS:
        raise ValueError(f'DepthPipeline: render={render!r}: None or one of {RENDERS}')
    table = R.lut(colour_map)
    if isinstance(render_range, str):
        if render_range != 'auto':
            raise ValueError(f"DepthPipeline: render_range={render_range!r}: (lo, hi) or 'auto'")
        rng = None
    else:
        try:
            lo, hi = render_range
        except (TypeError, ValueError):
            raise ValueError(f"DepthPipeline: render_range={render_range!r}: (lo, hi) or "
                             f"'auto'") from None
        rng = R.check_range(lo, hi, 'DepthPipeline: render_range')
        if rng is None:
            raise ValueError("DepthPipeline: render_range=(None, None): (lo, hi) or 'auto'")
    return table, rng, R.check_number('DepthPipeline: opacity', opacity), \
        R.check_number('DepthPipeline: invalid_opacity', invalid_opacity)


def _check_points(points, intrinsics, point_stride):
    """the point stage's arguments -> ((fx, fy, cx, cy), stride); raises before
    any GPU work"""
    who = 'DepthPipeline'
    if not isinstance(points, str) or points not in POINTS:
        raise ValueError(f'{who}: points={points!r}: None or one of {POINTS}')
    if intrinsics is None:
        raise ValueError(f'{who}: points={points!r} needs intrinsics=(fx, fy, cx, cy) in source '
                         f'pixels')
    intr = P.check_intrinsics(intrinsics, who)
    stride = P.check_stride(point_stride, who, 'point_stride')
    if stride != 1 and points == 'map':
        raise ValueError(f"{who}: point_stride={stride} with points='map': the organised map "
                         f"has every pixel (the stride thins the cloud)")
    return intr, stride


def _check_frames(frames, shape):
    """a frame batch must be a uint8 tensor of exactly ``shape``"""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise TypeError(f'DepthPipeline: uint8 frames expected, got '
                        f'{frames.dtype if torch.is_tensor(frames) else type(frames)}')
    if tuple(frames.shape) != tuple(shape):
        raise ValueError(f'DepthPipeline built for frames {tuple(shape)} (uint8 [B, Hs, Ws, 3]), '
                         f'got {tuple(frames.shape)}')


class DepthPipeline:
    """``pipe = DepthPipeline(model, src_height, src_width, batch=1, height=256,
    width=512, scale=1.0, focal_baseline=1.0, min_disparity=1e-3,
    max_uncertainty=inf, max_lr_error=inf)``; ``out = pipe(frames)`` with
    ``frames`` uint8 [B,Hs,Ws,3] on the host (pinned or not) or the device.

    ``out`` holds, for the left view at the frame's size ([B,Hs,Ws]):
    ``disparity`` (source pixels), ``depth`` (``focal_baseline / disparity``
    where ``disparity > min_disparity``, else 0; the unit of the baseline),
    ``uncertainty`` (the model's sigma, upsampled), ``lr_error`` (left-right
    consistency error, source pixels), ``valid`` (bool: ``disparity >
    min_disparity and uncertainty <= max_uncertainty and lr_error <=
    max_lr_error``), and ``prediction``, the engine's [B,4,H,W] output.

    These are VIEWS OF THE PIPELINE'S STATIC BUFFERS: valid until the next
    call (or refresh), which overwrites them -- clone what must outlive that.

    ``focal_baseline`` is the focal length in source pixels times the
    baseline; ``min_disparity`` and ``max_lr_error`` are in source pixels.
    ``set_params`` changes any of the four without recapture.  ``refresh()``
    must be called after the model's weights or running statistics changed.
    ``fused`` is the InferenceEngine's switch; ``capture=False`` runs the same
    three stages eagerly.

    ``render='disparity' | 'depth' | 'uncertainty' | 'lr_error'`` adds a
    display stage to the same graph: ``out['render']``, uint8 [B,Hs,Ws,3], is
    that map coloured through ``colour_map`` (a name or a uint8 [256, 3]
    table, ``umamd.render.lut``) over ``render_range=(lo, hi)`` -- or
    ``'auto'``, the min and max over the valid pixels of the batch, per call
    -- ``1 -`` that if ``inverse``, blended over the input frame with
    ``opacity`` where ``valid`` and ``invalid_opacity`` elsewhere (0: the
    camera image shows through).  ``set_params`` then also takes
    ``render_lo``, ``render_hi`` (not with ``'auto'``), ``opacity`` and
    ``invalid_opacity``.  With ``render=None`` (the default) nothing of this
    is allocated, launched or returned.

    ``points='map' | 'cloud' | 'both'`` with ``intrinsics=(fx, fy, cx, cy)``
    (source pixels; the pixel centre at the integer coordinate) adds the point
    stage to the same graph (umamd/points.py has the definition).  ``'map'``:
    ``out['xyz']``, f32 [B,Hs,Ws,3], (X, Y, Z) where ``valid`` and 0 elsewhere.
    ``'cloud'``: the valid pixels of every ``point_stride``-th row and column,
    packed image by image in row-major order: ``out['cloud_xyzu']`` f32
    [capacity, 4] (X, Y, Z, uncertainty), ``out['cloud_rgba']`` uint8
    [capacity, 4] (the frame's colour, 255) and ``out['cloud_offsets']`` int32
    [B + 1] -- image n owns rows ``offsets[n]:offsets[n + 1]``, the rows from
    ``offsets[B]`` on are unspecified.  ``cloud()`` reads the offsets (the
    stage's only synchronisation) and returns one ``(xyzu, rgba)`` pair of
    views per image.  ``set_params`` then also takes ``fx``, ``fy``, ``cx``,
    ``cy``.  With ``points=None`` (the default) nothing of this is allocated,
    launched or returned.

    ``rectify=`` a ``umamd.rectify.Calibration`` or ``RemapTable`` adds stage 0
    to the same graph: ``src_height`` and ``src_width`` stay the camera's RAW
    size, the frames passed to the call are raw, and the rectified size (Hr,
    Wr) -- the calibration's ``size`` (default: the raw size) or the table's
    shape -- is the frame size of every later stage and of every output.
    ``out['frame']`` is the rectified frame, uint8 [B,Hr,Wr,3], ``out['inside']``
    (bool [Hr,Wr]) marks the pixels whose source lies inside the raw frame, and
    ``valid`` is restricted to them.  ``focal_baseline`` and ``intrinsics`` are
    those of the RECTIFIED camera: ``Calibration.focal_baseline`` and
    ``.intrinsics``.  ``set_calibration(how)`` replaces the block or the table
    in place (same mode and sizes), seen by the next call without recapture.
    With ``rectify=None`` (the default) nothing of this is allocated, launched
    or returned."""

    def __init__(self, model, src_height: int, src_width: int, batch: int = 1, height: int = 256,
                 width: int = 512, scale: float = 1.0, focal_baseline: float = 1.0,
                 min_disparity: float = 1e-3, max_uncertainty: float = math.inf,
                 max_lr_error: float = math.inf, fused: bool = True, capture: bool = True,
                 render=None, colour_map='inferno', render_range='auto', opacity: float = 1.0,
                 invalid_opacity: float = 0.0, inverse: bool = False, points=None,
                 intrinsics=None, point_stride: int = 1, rectify=None):
        rcfg = None if render is None else _check_render(render, colour_map, render_range,
                                                         opacity, invalid_opacity)
        pcfg = None if points is None else _check_points(points, intrinsics, point_stride)
        B, H, W, Hs, Ws = int(batch), int(height), int(width), int(src_height), int(src_width)
        raw = None
        if rectify is not None:
            # stage 0: (Hs, Ws) is the rectified size from here on, raw the camera's
            Q.check_how(rectify, 'DepthPipeline: rectify')
            raw = (Hs, Ws)
            Hs, Ws = rectify.out_size(raw)
            if B >= 1:
                Q.check_sizes('DepthPipeline: rectify', B, raw[0], raw[1], Hs, Ws)
        if H <= 0 or W <= 0 or H % 32 or W % 32:
            raise ValueError(f'image size {H}x{W}: height and width must be multiples of 32')
        if Hs < 2 or Ws < 2:
            raise ValueError(f'source size {Hs}x{Ws}: height and width must be at least 2')
        if B < 1:
            raise ValueError(f'batch {B}')
        bh, kh, ksh = resize_coeffs(Ws, W)
        bv, kv, ksv = resize_coeffs(Hs, H)
        if not query('um_frame_prep_ok', Hs, Ws, H, W, ksh, ksv):
            raise ValueError(
                f'source size {Hs}x{Ws} -> {H}x{W} is past the limit of um_frame_prep: every '
                f'upscale, a vertical downscale up to 56x (ceil(7 * Hs / H) + 1 + ks_v <= 512 '
                f'source rows of a tile in 64 KiB of LDS; here '
                f'{-(-7 * Hs // H) + 1 + ksv}) and a horizontal one up to 128x (ks_h <= 257; '
                f'here {ksh})')
        self.infer = InferenceEngine(model, B, H, W, scale, fused=fused, capture=False)
        self.model = self.infer.model
        self.shape = (B, 3, H, W)
        self.src_shape = (B, Hs, Ws, 3) if raw is None else (B, raw[0], raw[1], 3)
        self.frame_shape = (B, Hs, Ws, 3)  # what the stages after stage 0 read
        self.scale = float(scale)
        self.capture = bool(capture)
        dev = self.infer._in.device
        self._frames = torch.zeros(self.frame_shape, dtype=torch.uint8, device=dev)
        self.rectify = rectify
        if rectify is not None:
            self._raw = torch.zeros(self.src_shape, dtype=torch.uint8, device=dev)
            self._inside = torch.zeros((Hs, Ws), dtype=torch.uint8, device=dev)
            self._rect = rectify.data(dev)  # the f32[24] block or the Q5 table
        self._tables = tuple(torch.from_numpy(a).to(dev) for a in (bh, kh, bv, kv))
        self._ks = (ksh, ksv)
        f32 = dict(dtype=torch.float32, device=dev)
        self._disparity = torch.zeros((B, Hs, Ws), **f32)
        self._depth = torch.zeros((B, Hs, Ws), **f32)
        self._uncertainty = torch.zeros((B, Hs, Ws), **f32)
        self._lr_error = torch.zeros((B, Hs, Ws), **f32)
        self._valid = torch.zeros((B, Hs, Ws), dtype=torch.uint8, device=dev)
        self.params = {'focal_baseline': float(focal_baseline),
                       'min_disparity': float(min_disparity),
                       'max_uncertainty': float(max_uncertainty),
                       'max_lr_error': float(max_lr_error)}
        self._params = torch.tensor([self.params[k] for k in PARAMS], **f32)
        self.render = render
        if rcfg is not None:
            table, rng, op, iop = rcfg
            self.inverse = bool(inverse)
            self.render_auto = rng is None
            lo, hi = rng or (0.0, 1.0)  # 'auto': replaced by the device range
            self.render_params = {'render_lo': lo, 'render_hi': hi, 'opacity': op,
                                  'invalid_opacity': iop}
            self._rparams = torch.tensor([self.render_params[k] for k in R.RENDER_PARAMS], **f32)
            self._lut = table.to(dev)
            self._render = torch.zeros((B, Hs, Ws, 3), dtype=torch.uint8, device=dev)
            self._range = self._range_ws = None
            if self.render_auto:
                self._range = torch.zeros(2, **f32)
                self._range_ws = torch.zeros(query('um_value_range_ws', B * Hs * Ws),
                                             dtype=torch.uint8, device=dev)
        self.points = points
        if pcfg is not None:
            intr, self.point_stride = pcfg
            self.intrinsics = dict(zip(P.INTR_PARAMS, intr))
            self._intr = torch.tensor(intr, **f32)
            if points in ('map', 'both'):
                self._xyz = torch.zeros((B, Hs, Ws, 3), **f32)
            if points in ('cloud', 'both'):
                s = self.point_stride
                capacity = B * -(-Hs // s) * -(-Ws // s)
                self._cloud_xyzu = torch.zeros((capacity, 4), **f32)
                self._cloud_rgba = torch.zeros((capacity, 4), dtype=torch.uint8, device=dev)
                self._cloud_offsets = torch.zeros(B + 1, dtype=torch.int32, device=dev)
                self._cloud_ws = torch.zeros(query('um_depth_cloud_ws', B, Hs, Ws, s),
                                             dtype=torch.uint8, device=dev)
        self._graph = None
        self._out = None
        self._called = False
        with torch.cuda.device(dev):
            if self.capture:
                self._capture()

    # ---------------------------------------------------------------- runs --
    def _run(self):
        B, _, H, W = self.shape
        _, Hs, Ws, _ = self.frame_shape
        bh, kh, bv, kv = self._tables
        if self.rectify is not None:
            cal, table = (self._rect, None) if self.rectify.mode == 'analytic' else \
                (None, self._rect)
            call('um_frame_rectify', ptr(self._raw), B, self.src_shape[1], self.src_shape[2], Hs,
                 Ws, ptr(cal), ptr(table), ptr(self._frames), ptr(self._inside))
        call('um_frame_prep', B, Hs, Ws, ptr(self._frames), H, W, ptr(bh), ptr(kh), self._ks[0],
             ptr(bv), ptr(kv), self._ks[1], ptr(self.infer._in))
        out = self.infer._forward()
        if out.dtype != torch.float32 or out.stride(3) != 1 or out.stride(1) != W * out.stride(2):
            raise L.UmamdError(f'DepthPipeline: prediction {out.dtype} with strides '
                               f'{out.stride()} is not an NHWC f32 image')
        call('um_depth_post', ptr(out), out.stride(0), out.stride(2), B, H, W, Hs, Ws,
             ptr(self._params), ptr(self._disparity), ptr(self._depth), ptr(self._uncertainty),
             ptr(self._lr_error), ptr(self._valid))
        if self.rectify is not None:
            call('um_valid_and', ptr(self._valid), ptr(self._inside), B, Hs * Ws)
        if self.render is not None:
            value = getattr(self, '_' + self.render)
            if self.render_auto:
                R.value_range(value, self._valid, out=self._range, ws=self._range_ws)
            call('um_depth_render', ptr(value), ptr(self._valid), ptr(self._frames), B * Hs * Ws,
                 ptr(self._lut), ptr(self._rparams), ptr(self._range), int(self.inverse),
                 ptr(self._render))
        if self.points in ('map', 'both'):
            call('um_depth_backproject', ptr(self._depth), ptr(self._valid), B, Hs, Ws,
                 ptr(self._intr), ptr(self._xyz))
        if self.points in ('cloud', 'both'):
            call('um_depth_cloud', ptr(self._depth), ptr(self._valid), ptr(self._uncertainty),
                 ptr(self._frames), B, Hs, Ws, self.point_stride, ptr(self._intr),
                 ptr(self._cloud_ws), ptr(self._cloud_xyzu), ptr(self._cloud_rgba),
                 ptr(self._cloud_offsets))
        return out

    def _capture(self):
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.no_grad(), _eval_mode(self.model):
            with torch.cuda.stream(side):
                self._run()  # warm-up (allocator, constants)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                out = self._run()
        cur.wait_stream(side)
        self._graph, self._out = g, out

    def refresh(self):
        """Re-fold and re-pack from the model's current weights and running
        statistics (in place: the captured graph stays valid unless a
        parameter's storage moved, which captures again)."""
        before = self.infer._sites()
        self.infer.refresh()
        if self.capture and self.infer._sites() != before:
            with torch.cuda.device(self._frames.device):
                self._capture()

    def set_params(self, **kw):
        """any of focal_baseline, min_disparity, max_uncertainty, max_lr_error
        and, with ``render=``, render_lo, render_hi (a fixed range only),
        opacity, invalid_opacity and, with ``points=``, fx, fy, cx, cy: written
        into the device blocks in place, seen by the next call"""
        known = PARAMS + (R.RENDER_PARAMS if self.render is not None else ()) + \
            (P.INTR_PARAMS if self.points is not None else ())
        bad = sorted(set(kw) - set(known))
        if bad:
            raise TypeError(f'DepthPipeline.set_params: unknown {bad}; one of {known}')
        rkw = {k: kw.pop(k) for k in R.RENDER_PARAMS if k in kw}
        if rkw:
            fixed = [k for k in ('render_lo', 'render_hi') if k in rkw]
            if fixed and self.render_auto:
                raise ValueError(f"DepthPipeline.set_params: {fixed} on a pipeline built with "
                                 f"render_range='auto' (the range is found per call)")
            rkw = {k: R.check_number(f'DepthPipeline.set_params: {k}', v)
                   for k, v in rkw.items()}
        ikw = {k: kw.pop(k) for k in P.INTR_PARAMS if k in kw}
        if ikw:
            intr = P.check_intrinsics([ikw.get(k, self.intrinsics[k]) for k in P.INTR_PARAMS],
                                      'DepthPipeline.set_params')
        if kw:
            self.params.update({k: float(v) for k, v in kw.items()})
            self._params.copy_(torch.tensor([self.params[k] for k in PARAMS],
                                            dtype=torch.float32))
        if rkw:
            self.render_params.update(rkw)
            self._rparams.copy_(torch.tensor([self.render_params[k] for k in R.RENDER_PARAMS],
                                             dtype=torch.float32))
        if ikw:
            self.intrinsics = dict(zip(P.INTR_PARAMS, intr))
            self._intr.copy_(torch.tensor(intr, dtype=torch.float32))

    def set_calibration(self, how):
        """Another Calibration (or RemapTable) of the same mode and sizes:
        written into the device block (table) in place, seen by the next call
        without recapture.  Another mode or size is a ValueError."""
        who = 'DepthPipeline.set_calibration'
        if self.rectify is None:
            raise ValueError(f'{who} on a pipeline built with rectify=None')
        Q.check_how(how, who)
        if how.mode != self.rectify.mode:
            raise ValueError(f'{who}: a {type(how).__name__} on a pipeline built with a '
                             f'{type(self.rectify).__name__}: build another pipeline')
        size = tuple(how.out_size(self.src_shape[1:3]))
        if size != tuple(self.frame_shape[1:3]):
            raise ValueError(f'{who}: rectified size {size}, the pipeline was built for '
                             f'{tuple(self.frame_shape[1:3])}: build another pipeline')
        self._rect.copy_(how.data(None))
        self.rectify = how

    def __call__(self, frames: torch.Tensor):
        _check_frames(frames, self.src_shape)
        (self._frames if self.rectify is None else self._raw).copy_(frames, non_blocking=True)
        if self._graph is not None:
            self._graph.replay()
        else:
            with torch.cuda.device(self._frames.device), torch.no_grad(), \
                    _eval_mode(self.model):
                self._out = self._run()
        self._called = True
        return self.last()

    def last(self):
        """views of the static buffers of the last call (valid until the next one)"""
        if not self._called:
            raise L.UmamdError('DepthPipeline.last() before the first call')
        out = {'disparity': self._disparity, 'depth': self._depth,
               'uncertainty': self._uncertainty, 'lr_error': self._lr_error,
               'valid': self._valid.view(torch.bool),
               'prediction': self._out.permute(0, 3, 1, 2)[:, :4]}
        if self.rectify is not None:
            out['frame'] = self._frames
            out['inside'] = self._inside.view(torch.bool)
        if self.render is not None:
            out['render'] = self._render
        if self.points in ('map', 'both'):
            out['xyz'] = self._xyz
        if self.points in ('cloud', 'both'):
            out.update(cloud_xyzu=self._cloud_xyzu, cloud_rgba=self._cloud_rgba,
                       cloud_offsets=self._cloud_offsets)
        return out

    def cloud(self):
        """the cloud of the last call, one ``(xyzu, rgba)`` pair of views per
        image (umamd.points.split: reads the offsets, which synchronises)"""
        if self.points not in ('cloud', 'both'):
            raise L.UmamdError(f"DepthPipeline.cloud() on a pipeline built with "
                               f"points={self.points!r}")
        if not self._called:
            raise L.UmamdError('DepthPipeline.cloud() before the first call')
        return P.split(self._cloud_xyzu, self._cloud_rgba, self._cloud_offsets)
