"""Refinement on the device: the pipeline's disparity and uncertainty
smoothed along the full-resolution frame's edges and fused over the frames of a
stream (csrc/refine.hip, include/umamd.h "deployment" has the definition, to
the bit).

  tables(radius, sigma_space, sigma_colour)   the (S, G) weight tables
  smooth(disparity, uncertainty, frame, ...)  um_disp_smooth: a dilated
                     joint-bilateral filter, each tap weighted by distance, by
                     its colour difference to the centre in ``frame`` and by
                     its confidence 1 / (sigma^2 + conf_eps)
  new_state(like)    an empty (mean, var) state of a stream
  fuse(disparity, uncertainty, ...)           um_disp_fuse: a per-pixel
                     recursive filter over the calls that share a ``state``,
                     then depth and the mask as um_depth_post defines them

``umamd.deploy.DepthPipeline(refine=...)`` runs the same entries inside its
captured graph: ``RefineStage`` is that stage.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._lib import call, check_same_device, check_tensor, ptr

REFINES = ('spatial', 'temporal', 'both')
REFINE_PARAMS = ('sigma_space', 'sigma_colour', 'conf_eps', 'noise_scale', 'var_floor',
                 'process_noise', 'gate')
MAX_RADIUS, MAX_HALO, COLOURS = 3, 16, 768
# Starting points, not measured optima ("Refinement")
NOISE_SCALE, VAR_FLOOR, PROCESS_NOISE = 20.0, 0.25, 1.0


def check_window(radius, step, who: str = 'umamd.refine'):
    """(radius, step) as ints within the kernel's limits; ValueError otherwise"""
    for k, v in (('radius', radius), ('step', step)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f'{who}: {k}={v!r}: an integer expected')
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f'{who}: radius={radius}: 1 <= radius <= {MAX_RADIUS}')
    if step < 1:
        raise ValueError(f'{who}: step={step}: an integer >= 1 expected')
    if radius * step > MAX_HALO:
        raise ValueError(f'{who}: radius * step = {radius * step}: at most {MAX_HALO} (the halo '
                         f'a tile stages)')
    return radius, step


def check_values(values: dict, who: str = 'umamd.refine') -> dict:
    """the seven float parameters (any subset) as floats: sigmas and gate > 0,
    the others >= 0, all finite but ``gate`` (inf: nothing is gated out)"""
    out = {}
    for k, v in values.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ValueError(f'{who}: {k}={v!r}: a number expected')
        positive = k in ('sigma_space', 'sigma_colour', 'gate')
        if v < 0 or (positive and v == 0) or (math.isinf(v) and k != 'gate'):
            raise ValueError(f'{who}: {k}={v!r}: a finite number '
                             f'{"> 0" if positive else ">= 0"} expected')
        out[k] = float(v)
    return out


def tables(radius: int, sigma_space: float, sigma_colour: float):
    """``(S, G)``, f32 on the host: ``S[|j| * (radius + 1) + |i|] = exp(-(i^2 +
    j^2) / (2 sigma_space^2))`` (sigma_space in taps) and ``G[k] = exp(-k^2 /
    (2 sigma_colour^2))`` for k = 0..767 (sigma_colour in summed 8-bit
    levels), made in f64 and rounded"""
    who = 'umamd.refine.tables'
    radius, _ = check_window(radius, 1, who)
    v = check_values(dict(sigma_space=sigma_space, sigma_colour=sigma_colour), who)
    a = np.arange(radius + 1, dtype=np.float64)
    S = np.exp(-(a[None, :] ** 2 + a[:, None] ** 2) / (2.0 * v['sigma_space'] ** 2))
    k = np.arange(COLOURS, dtype=np.float64)
    G = np.exp(-(k ** 2) / (2.0 * v['sigma_colour'] ** 2))
    return (torch.from_numpy(S.astype(np.float32).reshape(-1)),
            torch.from_numpy(G.astype(np.float32)))


def block(conf_eps, noise_scale, var_floor, process_noise, gate):
    """the f32[8] block of both kernels, on the host: (eps, a, floor, q, g2 =
    gate * gate, 0, 0, 0)"""
    return torch.tensor([conf_eps, noise_scale, var_floor, process_noise, gate * gate, 0, 0, 0],
                        dtype=torch.float32)


def _check_maps(who, disparity, **others):
    """f32 contiguous [H, W] or [N, H, W] maps of one shape -> (N, Hs, Ws)"""
    check_tensor(who, 'disparity', disparity, (torch.float32,), 'f32')
    if disparity.dim() not in (2, 3) or not disparity.is_contiguous() or disparity.numel() == 0:
        raise ValueError(f'{who}: disparity must be a contiguous, non-empty [H, W] or [N, H, W] '
                         f'map (shape {tuple(disparity.shape)}, strides {disparity.stride()})')
    shape = tuple(disparity.shape)
    for k, t in others.items():
        if t is not None:
            check_tensor(who, k, t, (torch.float32,), 'f32', shape)
    if disparity.numel() > 2 ** 31 - 1:
        raise ValueError(f'{who}: {disparity.numel()} pixels, at most 2^31 - 1')
    return (shape[0] if len(shape) == 3 else 1), shape[-2], shape[-1]


def _overlap(a, b):
    lo, hi = a.data_ptr(), a.data_ptr() + a.numel() * a.element_size()
    return b.data_ptr() < hi and lo < b.data_ptr() + b.numel() * b.element_size()


def _smooth(disp, unc, frame, n, hs, ws, radius, step, S, G, fp, disp_out, unc_out):
    """um_disp_smooth on the current stream; no checks"""
    call('um_disp_smooth', ptr(disp), ptr(unc), ptr(frame), n, hs, ws, radius, step, ptr(S),
         ptr(G), ptr(fp), ptr(disp_out), ptr(unc_out))


def _fuse(disp, unc, lr_error, count, params, fp, mean, var, disparity, uncertainty, depth,
          valid, disp_var=None):
    """um_disp_fuse on the current stream; no checks"""
    call('um_disp_fuse', ptr(disp), ptr(unc), ptr(lr_error), count, ptr(params), ptr(fp),
         ptr(mean), ptr(var), ptr(disparity), ptr(uncertainty), ptr(depth), ptr(valid),
         ptr(disp_var))


def smooth(disparity: torch.Tensor, uncertainty: torch.Tensor, frame: torch.Tensor,
           radius: int = 2, step: int = 1, sigma_space: float = 1.5, sigma_colour: float = 30.0,
           conf_eps: float = 1e-4, weights=None, out=None):
    """``disparity`` and ``uncertainty`` (f32, contiguous [H, W] or [N, H, W],
    on the device) filtered along the edges of ``frame`` (uint8, their shape +
    (3,)) -> ``(disparity, uncertainty)``, new tensors (or ``out``, a pair that
    overlaps no input).  ``weights=(S, G)`` replaces the Gaussian tables.  Runs
    on the current stream, never synchronises."""
    who = 'umamd.refine.smooth'
    radius, step = check_window(radius, step, who)
    eps = check_values(dict(conf_eps=conf_eps), who)['conf_eps']
    S, G = tables(radius, sigma_space, sigma_colour) if weights is None else weights
    check_tensor(who, 'S', S, (torch.float32,), 'f32', ((radius + 1) ** 2,))
    check_tensor(who, 'G', G, (torch.float32,), 'f32', (COLOURS,))
    n, hs, ws = _check_maps(who, disparity, uncertainty=uncertainty)
    check_tensor(who, 'frame', frame, (torch.uint8,), 'uint8', tuple(disparity.shape) + (3,))
    check_same_device(who, 'disparity', disparity, uncertainty=uncertainty, frame=frame)
    dev = disparity.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(disparity), torch.empty_like(uncertainty)
        _check_maps(who, disparity, disparity_out=out[0], uncertainty_out=out[1])
        check_same_device(who, 'disparity', disparity, disparity_out=out[0],
                          uncertainty_out=out[1])
        if any(_overlap(o, i) for o in out for i in (disparity, uncertainty)) or \
                _overlap(out[0], out[1]):
            raise ValueError(f'{who}: an output overlaps an input (every pixel reads its '
                             f'neighbours: the filter cannot run in place)')
        _smooth(disparity, uncertainty, frame, n, hs, ws, radius, step, S.to(dev), G.to(dev),
                block(eps, 0, 0, 0, 0).to(dev), *out)
    return out


def new_state(like: torch.Tensor):
    """an empty ``(mean, var)`` state for maps shaped as ``like``: var = -1"""
    return torch.zeros_like(like), torch.full_like(like, -1.0)


def fuse(disparity: torch.Tensor, uncertainty: torch.Tensor, lr_error=None, state=None,
         focal_baseline: float = 1.0, min_disparity: float = 1e-3,
         max_uncertainty: float = math.inf, max_lr_error: float = math.inf,
         noise_scale: float = NOISE_SCALE, var_floor: float = VAR_FLOOR,
         process_noise: float = PROCESS_NOISE, gate: float = 3.0) -> dict:
    """One step of the recursive filter: ``state`` (``new_state``; updated IN
    PLACE) fused with the measurement ``disparity`` of noise ``(noise_scale *
    uncertainty)^2 + var_floor`` -> dict of new tensors ``disparity`` (the
    state's mean where it holds one), ``uncertainty`` (unchanged), ``depth``,
    ``valid`` (bool; ``lr_error`` None counts as 0) and ``disparity_var`` (the
    state's variance).  ``state=None``: no filter, only depth and the mask of
    the inputs.  Runs on the current stream, never synchronises."""
    who = 'umamd.refine.fuse'
    v = check_values(dict(noise_scale=noise_scale, var_floor=var_floor,
                          process_noise=process_noise, gate=gate), who)
    mean, var = (None, None) if state is None else state
    _check_maps(who, disparity, uncertainty=uncertainty, lr_error=lr_error, mean=mean, var=var)
    check_same_device(who, 'disparity', disparity, uncertainty=uncertainty, lr_error=lr_error,
                      mean=mean, var=var)
    dev = disparity.device
    with torch.cuda.device(dev):
        if lr_error is None:
            lr_error = torch.zeros_like(disparity)
        params = torch.tensor([focal_baseline, min_disparity, max_uncertainty, max_lr_error],
                              dtype=torch.float32).to(dev)
        out = {k: torch.empty_like(disparity) for k in ('disparity', 'uncertainty', 'depth')}
        valid = torch.empty(disparity.shape, dtype=torch.uint8, device=dev)
        if state is not None:
            out['disparity_var'] = torch.empty_like(disparity)
        _fuse(disparity, uncertainty, lr_error, disparity.numel(), params,
              block(0, v['noise_scale'], v['var_floor'], v['process_noise'], v['gate']).to(dev),
              mean, var, out['disparity'], out['uncertainty'], out['depth'], valid,
              out.get('disparity_var'))
    out['valid'] = valid.view(torch.bool)
    return out


class RefineStage:
    """The refine stage of ``umamd.deploy.DepthPipeline``: its arguments,
    checked on the host, its buffers, tables and device block, its launches
    and its outputs.  um_depth_post writes disparity and uncertainty into the
    stage's raw buffers (``post_targets``); ``run`` fills the pipeline's maps
    from them."""

    keys = REFINE_PARAMS  # of ``params``: what set_params takes

    def __init__(self, refine, radius, step, sigma_space, sigma_colour, conf_eps, noise_scale,
                 var_floor, process_noise, gate):
        who = 'DepthPipeline'
        if not isinstance(refine, str) or refine not in REFINES:
            raise ValueError(f'{who}: refine={refine!r}: None or one of {REFINES}')
        self.mode = refine
        self.radius, self.step = check_window(radius, step, f'{who}: refine')
        self.params = check_values(dict(zip(REFINE_PARAMS, (
            sigma_space, sigma_colour, conf_eps, noise_scale, var_floor, process_noise, gate))),
            who)

    spatial = property(lambda self: self.mode in ('spatial', 'both'))
    temporal = property(lambda self: self.mode in ('temporal', 'both'))

    def _host(self, p):
        """(S, G, block) of parameters ``p`` on the host"""
        return tables(self.radius, p['sigma_space'], p['sigma_colour']) + (
            block(*[p[k] for k in REFINE_PARAMS[2:]]),)

    def allocate(self, dev, B, Hs, Ws):
        self._size = (B, Hs, Ws)
        f32 = dict(dtype=torch.float32, device=dev)
        self._S, self._G, self.block = (t.to(dev) for t in self._host(self.params))
        self._raw = {k: torch.zeros(self._size, **f32) for k in ('disparity', 'uncertainty')}
        self._mean = self._var = None
        if self.temporal:
            self._mean = torch.zeros(self._size, **f32)
            self._var = torch.full(self._size, -1.0, **f32)

    def post_targets(self):
        """where um_depth_post writes with this stage: disparity and uncertainty
        into the raw buffers; depth and the mask are um_disp_fuse's"""
        return dict(self._raw, depth=None, valid=None)

    def run(self, maps, frames, params):
        """``maps``: the pipeline's buffers (lr_error already um_depth_post's);
        ``params``: its 4-float block"""
        n, hs, ws = self._size
        d, u = self._raw['disparity'], self._raw['uncertainty']
        if self.spatial:
            _smooth(d, u, frames, n, hs, ws, self.radius, self.step, self._S, self._G,
                    self.block, maps['disparity'], maps['uncertainty'])
            d, u = maps['disparity'], maps['uncertainty']  # fused in place from here
        _fuse(d, u, maps['lr_error'], n * hs * ws, params, self.block, self._mean, self._var,
              maps['disparity'] if self.temporal else None,
              None if self.spatial else maps['uncertainty'], maps['depth'], maps['valid'])

    def reset(self):
        """empty the temporal state: the next call starts a new stream"""
        if self.temporal:
            self._var.fill_(-1.0)

    def outputs(self):
        out = {'raw_' + k: t for k, t in self._raw.items()}
        if self.temporal:
            out['disparity_var'] = self._var
        return out

    def check_params(self, kw):
        """the stage's part of set_params, checked (nothing is written yet)"""
        return check_values(kw, 'DepthPipeline.set_params')

    def write(self, checked):
        """``checked`` into the host dict, the tables and the block, in place"""
        self.params.update(checked)
        for dst, src in zip((self._S, self._G, self.block), self._host(self.params)):
            dst.copy_(src)
