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

With ``refine=`` a stage sits straight after um_depth_post, in the same graph
(umamd/refine.py), and the display and point stages read what it wrote:

  um_disp_smooth  only 'spatial' and 'both': disparity and uncertainty
                  filtered along the edges of the full-resolution frame, each
                  tap weighted by its confidence
  um_disp_fuse    'temporal' and 'both': the disparity fused per pixel with
                  the stream's state; always: depth and the mask of the
                  refined maps (um_depth_post leaves these two to it)

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
from ._lib import call, ptr, query, write_block
from .imageprep import resize_coeffs
from .infer import InferenceEngine, _eval_mode, capture_graph, check_prediction, refresh_engine
from .points import POINTS, PointStage, split  # noqa: F401 (POINTS: a name of this module too)
from .rectify import RectifyStage
from .refine import NOISE_SCALE, PROCESS_NOISE, REFINES, VAR_FLOOR, RefineStage  # noqa: F401
from .render import RENDERS, RenderStage

PARAMS = ('focal_baseline', 'min_disparity', 'max_uncertainty', 'max_lr_error')


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
    or returned.

    ``refine='spatial' | 'temporal' | 'both'`` adds the refine stage to the
    same graph (umamd/refine.py; include/umamd.h has the definition).
    ``disparity``, ``uncertainty``, ``depth`` and ``valid`` are then the
    REFINED maps -- the display and point stages read them -- ``lr_error``
    stays raw, and ``out['raw_disparity']`` and ``out['raw_uncertainty']`` hold
    what um_depth_post produced.  ``'spatial'``: a joint-bilateral filter of
    ``(2 * refine_radius + 1)^2`` taps ``refine_step`` pixels apart (None:
    ``max(1, round(Ws / width))``, one model pixel), weighted by distance
    (``sigma_space``, taps), by the colour difference to the centre in the
    frame (``sigma_colour``, summed 8-bit levels) and by the tap's confidence
    ``1 / (uncertainty^2 + conf_eps)``.  ``'temporal'``: a per-pixel recursive
    filter over the calls, the measurement noise ``(noise_scale *
    uncertainty)^2 + var_floor``, the state's variance growing by
    ``process_noise`` per call, a measurement further than ``gate`` standard
    deviations from the state restarting it; ``out['disparity_var']`` is the
    state's variance (source pixels squared).  There is no motion
    compensation: the filter suits a camera that moves little between frames.
    ``'both'``: the first, then the second.  The state is empty after
    construction, ``refresh()`` and ``reset_refine()``.  ``set_params`` then
    also takes the seven float parameters (tables and block rewritten in
    place); radius and step are fixed.  With ``refine=None`` (the default)
    nothing of this is allocated, launched or returned."""

    def __init__(self, model, src_height: int, src_width: int, batch: int = 1, height: int = 256,
                 width: int = 512, scale: float = 1.0, focal_baseline: float = 1.0,
                 min_disparity: float = 1e-3, max_uncertainty: float = math.inf,
                 max_lr_error: float = math.inf, fused: bool = True, capture: bool = True,
                 render=None, colour_map='inferno', render_range='auto', opacity: float = 1.0,
                 invalid_opacity: float = 0.0, inverse: bool = False, points=None,
                 intrinsics=None, point_stride: int = 1, rectify=None, refine=None,
                 refine_radius: int = 2, refine_step=None, sigma_space: float = 1.5,
                 sigma_colour: float = 30.0, conf_eps: float = 1e-4,
                 noise_scale: float = NOISE_SCALE, var_floor: float = VAR_FLOOR,
                 process_noise: float = PROCESS_NOISE, gate: float = 3.0):
        # every stage checks its own arguments, in this order, before any GPU work
        self._render_stage = None if render is None else RenderStage(
            render, colour_map, render_range, opacity, invalid_opacity, inverse)
        self._point_stage = None if points is None else PointStage(points, intrinsics,
                                                                   point_stride)
        B, H, W, Hs, Ws = int(batch), int(height), int(width), int(src_height), int(src_width)
        rect = self._rect_stage = None if rectify is None else RectifyStage(rectify, B, Hs, Ws)
        self.render, self.points = render, points
        self.src_shape = (B, Hs, Ws, 3)  # the camera's raw size
        if rect is not None:
            Hs, Ws = rect.size  # the rectified size from here on
        if refine_step is None and W > 0:
            refine_step = max(1, round(Ws / W))  # one model pixel
        self._refine_stage = None if refine is None else RefineStage(
            refine, refine_radius, refine_step, sigma_space, sigma_colour, conf_eps, noise_scale,
            var_floor, process_noise, gate)
        self.refine = refine
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
        self.frame_shape = (B, Hs, Ws, 3)  # what the stages after stage 0 read
        self.scale = float(scale)
        self.capture = bool(capture)
        dev = self.infer._in.device
        self._after = [st for st in (self._render_stage, self._point_stage) if st is not None]
        self._tunable = [st for st in [self._refine_stage] + self._after if st is not None]
        self._stages = [st for st in (rect, self._refine_stage) if st is not None] + self._after
        for st in self._stages:
            st.allocate(dev, B, Hs, Ws)
        self._frames = torch.zeros(self.frame_shape, dtype=torch.uint8, device=dev) \
            if rect is None else rect.frames
        self._input = self._frames if rect is None else rect.raw_frames  # what a call fills
        self._tables = tuple(torch.from_numpy(a).to(dev) for a in (bh, kh, bv, kv))
        self._ks = (ksh, ksv)
        f32 = dict(dtype=torch.float32, device=dev)
        self._maps = {k: torch.zeros((B, Hs, Ws), **f32) for k in RENDERS}
        self._maps['valid'] = torch.zeros((B, Hs, Ws), dtype=torch.uint8, device=dev)
        self.params = {'focal_baseline': float(focal_baseline),
                       'min_disparity': float(min_disparity),
                       'max_uncertainty': float(max_uncertainty),
                       'max_lr_error': float(max_lr_error)}
        self._params = torch.tensor([self.params[k] for k in PARAMS], **f32)
        self._graph = None
        self._out = None
        self._called = False
        with torch.cuda.device(dev):
            if self.capture:
                self._capture()

    # what the stages hold, readable as the pipeline's (AttributeError without the stage)
    rectify = property(lambda self: self._rect_stage and self._rect_stage.how)
    render_params = property(lambda self: self._render_stage.params)
    render_auto = property(lambda self: self._render_stage.auto)
    inverse = property(lambda self: self._render_stage.inverse)
    intrinsics = property(lambda self: self._point_stage.params)
    point_stride = property(lambda self: self._point_stage.stride)
    refine_params = property(lambda self: self._refine_stage.params)
    refine_radius = property(lambda self: self._refine_stage.radius)
    refine_step = property(lambda self: self._refine_stage.step)

    # ---------------------------------------------------------------- runs --
    def _run(self):
        """rectify -> prep -> forward -> post -> refine -> mask-and -> render ->
        points"""
        B, _, H, W = self.shape
        _, Hs, Ws, _ = self.frame_shape
        bh, kh, bv, kv = self._tables
        if self._rect_stage is not None:
            self._rect_stage.before_prep()
        call('um_frame_prep', B, Hs, Ws, ptr(self._frames), H, W, ptr(bh), ptr(kh), self._ks[0],
             ptr(bv), ptr(kv), self._ks[1], ptr(self.infer._in))
        out = self.infer._forward()
        check_prediction('DepthPipeline', out, W)
        post = self._maps
        if self._refine_stage is not None:
            post = {**post, **self._refine_stage.post_targets()}
        call('um_depth_post', ptr(out), out.stride(0), out.stride(2), B, H, W, Hs, Ws,
             ptr(self._params), *[ptr(post[k]) for k in RENDERS + ('valid',)])
        if self._refine_stage is not None:
            self._refine_stage.run(self._maps, self._frames, self._params)
        if self._rect_stage is not None:
            self._rect_stage.after_post(self._maps['valid'])
        for st in self._after:
            st.run(self._maps, self._frames)
        return out

    def _capture(self):
        self._graph, self._out = capture_graph(self.model, self._run)
        self.reset_refine()  # the warm-up run before the capture fused a frame

    def reset_refine(self):
        """Empty the temporal state of the refine stage: the next call starts
        a new stream.  Nothing to do without the stage or with 'spatial'."""
        if self._refine_stage is not None:
            self._refine_stage.reset()

    def refresh(self):
        """Re-fold and re-pack from the model's current weights and running
        statistics (in place: the captured graph stays valid unless a
        parameter's storage moved, which captures again)."""
        refresh_engine(self)
        self.reset_refine()  # other weights: the stream starts again

    def set_params(self, **kw):
        """any of focal_baseline, min_disparity, max_uncertainty, max_lr_error
        and, with ``render=``, render_lo, render_hi (a fixed range only),
        opacity, invalid_opacity and, with ``points=``, fx, fy, cx, cy and, with
        ``refine=``, sigma_space, sigma_colour, conf_eps, noise_scale, var_floor,
        process_noise, gate: written into the device blocks (and tables) in
        place, seen by the next call"""
        known = PARAMS + sum((st.keys for st in self._tunable), ())
        bad = sorted(set(kw) - set(known))
        if bad:
            raise TypeError(f'DepthPipeline.set_params: unknown {bad}; one of {known}')
        todo = []  # every stage checks its keys before anything is written
        for st in self._tunable:
            mine = {k: kw.pop(k) for k in st.keys if k in kw}
            if mine:
                todo.append((st, st.check_params(mine)))
        if kw:
            write_block(self._params, self.params, PARAMS, {k: float(v) for k, v in kw.items()})
        for st, checked in todo:
            st.write(checked)

    def set_calibration(self, how):
        """Another Calibration (or RemapTable) of the same mode and sizes:
        written into the device block (table) in place, seen by the next call
        without recapture.  Another mode or size is a ValueError."""
        if self._rect_stage is None:
            raise ValueError('DepthPipeline.set_calibration on a pipeline built with '
                             'rectify=None')
        self._rect_stage.set_calibration(how)

    def __call__(self, frames: torch.Tensor):
        _check_frames(frames, self.src_shape)
        self._input.copy_(frames, non_blocking=True)
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
        out = {k: self._maps[k] for k in RENDERS}
        out['valid'] = self._maps['valid'].view(torch.bool)
        out['prediction'] = self._out.permute(0, 3, 1, 2)[:, :4]
        for st in self._stages:
            out.update(st.outputs())
        return out

    def cloud(self):
        """the cloud of the last call, one ``(xyzu, rgba)`` pair of views per
        image (umamd.points.split: reads the offsets, which synchronises)"""
        if self.points not in ('cloud', 'both'):
            raise L.UmamdError(f"DepthPipeline.cloud() on a pipeline built with "
                               f"points={self.points!r}")
        if not self._called:
            raise L.UmamdError('DepthPipeline.cloud() before the first call')
        o = self._point_stage.outputs()
        return split(o['cloud_xyzu'], o['cloud_rgba'], o['cloud_offsets'])
