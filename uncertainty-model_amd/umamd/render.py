"""Display images on the device: a float map coloured through a 256-entry
table and blended over the camera frame (csrc/render.hip, include/umamd.h
"deployment").

This is the reference's host path -- ``train.utils.to_heatmap`` (matplotlib's
colour map), the min/max scaling of ``get_comparison(add_scaled=True)`` and
``save_image``'s ``x * 255 + 0.5`` rounding -- as one launch (three with the
automatic range), bit for bit: the table is ``floor(cmap(arange(256))[:, :3] *
255 + 0.5)`` and the kernel indexes it exactly as ``Colormap.__call__`` does
for an f32 array.

  lut(colour_map)   the uint8 [256, 3] table of a colour map
  colourise(value)  uint8 value.shape + (3,), on the device

``umamd.deploy.DepthPipeline(render=...)`` runs the same two entries inside
its captured graph: ``RenderStage`` is that stage.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._lib import call, check_same_device, check_tensor, ptr, query, write_block

# floor(plt.get_cmap('inferno')(arange(256))[:, :3] * 255 + 0.5), r g b per
# entry: data, so that a deployment box needs no matplotlib for the default
# map (tests/test_render_cpu.py compares it with matplotlib's)
_INFERNO = bytes.fromhex(
    '00000401000501010601010802010a02020c02020e03021004031204031405041706041907051b08051d09061f0a0722'
    '0b07240c08260d08290e092b10092d110a30120a32140b34150b37160b39180c3c190c3e1b0c411c0c431e0c451f0c48'
    '210c4a230c4c240c4f260c51280b53290b552b0b572d0b592f0a5b310a5c320a5e340a5f3609613809623909633b0964'
    '3d09653e0966400a67420a68440a68450a69470b6a490b6a4a0c6b4c0c6b4d0d6c4f0d6c510e6c520e6d540f6d550f6d'
    '57106e59106e5a116e5c126e5d126e5f136e61136e62146e64156e65156e67166e69166e6a176e6c186e6d186e6f196e'
    '71196e721a6e741a6e751b6e771c6d781c6d7a1d6d7c1d6d7d1e6d7f1e6c801f6c82206c84206b85216b87216b88226a'
    '8a226a8c23698d23698f24699025689225689326679526679727669827669a28659b29649d29649f2a63a02a63a22b62'
    'a32c61a52c60a62d60a82e5fa92e5eab2f5ead305dae305cb0315bb1325ab3325ab43359b63458b73557b93556ba3655'
    'bc3754bd3853bf3952c03a51c13a50c33b4fc43c4ec63d4dc73e4cc83f4bca404acb4149cc4248ce4347cf4446d04545'
    'd24644d34743d44842d54a41d74b3fd84c3ed94d3dda4e3cdb503bdd513ade5238df5337e05536e15635e25734e35933'
    'e45a31e55c30e65d2fe75e2ee8602de9612bea632aeb6429eb6628ec6726ed6925ee6a24ef6c23ef6e21f06f20f1711f'
    'f1731df2741cf3761bf37819f47918f57b17f57d15f67e14f68013f78212f78410f8850ff8870ef8890cf98b0bf98c0a'
    'f98e09fa9008fa9207fa9407fb9606fb9706fb9906fb9b06fb9d07fc9f07fca108fca309fca50afca60cfca80dfcaa0f'
    'fcac11fcae12fcb014fcb216fcb418fbb61afbb81dfbba1ffbbc21fbbe23fac026fac228fac42afac62df9c72ff9c932'
    'f9cb35f8cd37f8cf3af7d13df7d340f6d543f6d746f5d949f5db4cf4dd4ff4df53f4e156f3e35af3e55df2e661f2e865'
    'f2ea69f1ec6df1ed71f1ef75f1f179f2f27df2f482f3f586f3f68af4f88ef5f992f6fa96f8fb9af9fc9dfafda1fcffa4')

RENDER_PARAMS = ('render_lo', 'render_hi', 'opacity', 'invalid_opacity')
RENDERS = ('disparity', 'depth', 'uncertainty', 'lr_error')


def lut(colour_map='inferno') -> torch.Tensor:
    """The uint8 [256, 3] table (host tensor) of a colour map: ``'inferno'``
    from the committed table, any other name through matplotlib
    (``ImportError`` if it is missing, ``ValueError`` for a name it does not
    know or a map without 256 entries), a uint8 [256, 3] tensor or array as it
    is."""
    if isinstance(colour_map, str):
        if colour_map == 'inferno':
            return torch.frombuffer(bytearray(_INFERNO), dtype=torch.uint8).view(256, 3)
        try:
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError(f'umamd.render.lut: colour map {colour_map!r} needs matplotlib '
                              f'(only \'inferno\' is built in): {e}') from None
        import numpy as np
        cmap = plt.get_cmap(colour_map)  # ValueError for an unknown name
        if cmap.N != 256:
            raise ValueError(f'umamd.render.lut: colour map {colour_map!r} has {cmap.N} entries, '
                             f'256 expected')
        table = np.floor(cmap(np.arange(256))[:, :3] * 255 + 0.5).astype(np.uint8)
        return torch.from_numpy(table)
    if not torch.is_tensor(colour_map):
        import numpy as np
        if not isinstance(colour_map, np.ndarray):
            raise TypeError(f'umamd.render.lut: a colour map name or a uint8 [256, 3] tensor or '
                            f'array expected, got {type(colour_map).__name__}')
        if colour_map.dtype != np.uint8:
            raise TypeError(f'umamd.render.lut: uint8 table expected, got {colour_map.dtype}')
        colour_map = torch.from_numpy(np.ascontiguousarray(colour_map))
    if colour_map.dtype != torch.uint8:
        raise TypeError(f'umamd.render.lut: uint8 table expected, got {colour_map.dtype}')
    if tuple(colour_map.shape) != (256, 3):
        raise ValueError(f'umamd.render.lut: table of shape [256, 3] expected, got '
                         f'{tuple(colour_map.shape)}')
    return colour_map.contiguous()


def check_number(name: str, x) -> float:
    """a parameter of the device block is a real number (the kernel clamps an
    opacity to [0, 1])"""
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise TypeError(f'{name}: a number expected, got {type(x).__name__}')
    return float(x)


def check_range(lo, hi, who: str):
    """(lo, hi) as floats, or None for the automatic range (both None);
    exactly one of them is a ValueError"""
    if lo is None and hi is None:
        return None
    if lo is None or hi is None:
        raise ValueError(f'{who}: lo and hi go together (both, or neither for the range of the '
                         f'valid pixels), got lo={lo} hi={hi}')
    for k, v in (('lo', lo), ('hi', hi)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f'{who}: {k}: a number expected, got {type(v).__name__}')
    return float(lo), float(hi)


def value_range(value: torch.Tensor, valid=None, out=None, ws=None) -> torch.Tensor:
    """um_value_range on the current stream: f32 [2] = (min, max) of ``value``
    over its valid, non-NaN pixels ((+inf, -inf) if there is none).  ``value``
    f32 contiguous, ``valid`` uint8 of the same size or None; no checks (the
    callers made them)."""
    n = value.numel()
    if ws is None:
        ws = torch.empty(query('um_value_range_ws', n), dtype=torch.uint8, device=value.device)
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=value.device)
    call('um_value_range', ptr(value), ptr(valid), n, ptr(out), ptr(ws))
    return out


def paint(value, valid, frame, table, block, auto, inverse, out) -> torch.Tensor:
    """um_depth_render on the current stream into ``out``: ``block`` f32 [4]
    (RENDER_PARAMS), ``auto`` None or the f32 [2] of ``value_range``, ``valid``
    uint8 or None; no checks (the callers made them)."""
    call('um_depth_render', ptr(value), ptr(valid), ptr(frame), value.numel(), ptr(table),
         ptr(block), ptr(auto), int(bool(inverse)), ptr(out))
    return out


def colourise(value: torch.Tensor, lo=None, hi=None, valid=None, frame=None,
              colour_map='inferno', opacity: float = 1.0, invalid_opacity: float = 0.0,
              inverse: bool = False, out=None) -> torch.Tensor:
    """``value`` (f32, contiguous, on the device) -> uint8 ``value.shape +
    (3,)``: the colour of ``(value - lo) / (hi - lo)`` (``1 -`` that if
    ``inverse``) in ``colour_map``, blended over ``frame`` (uint8 ``value.shape
    + (3,)``; None: black) with ``opacity`` where ``valid`` (bool or uint8 of
    ``value``'s shape; None: everywhere) and ``invalid_opacity`` elsewhere.
    ``lo`` and ``hi`` both None: the min and max of the valid, non-NaN pixels,
    found on the device.  NaN is black.  Runs on the current stream, never
    synchronises; ``out`` takes the result if given."""
    who = 'umamd.render.colourise'
    check_tensor(who, 'value', value, (torch.float32,), 'f32')
    if not value.is_contiguous() or value.numel() == 0:
        raise ValueError(f'{who}: value must be contiguous and not empty (shape '
                         f'{tuple(value.shape)}, strides {value.stride()})')
    rng = check_range(lo, hi, who)
    op, iop = check_number(f'{who}: opacity', opacity), \
        check_number(f'{who}: invalid_opacity', invalid_opacity)
    table = lut(colour_map)
    shape = tuple(value.shape)
    if valid is not None:
        check_tensor(who, 'valid', valid, (torch.bool, torch.uint8), 'bool or uint8', shape)
    for name, t in (('frame', frame), ('out', out)):
        if t is not None:
            check_tensor(who, name, t, (torch.uint8,), 'uint8', shape + (3,))
    check_same_device(who, 'value', value, valid=valid, frame=frame, out=out)
    dev = value.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape + (3,), dtype=torch.uint8, device=dev)
        if valid is not None and valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
        block = torch.tensor([*(rng or (0.0, 1.0)), op, iop], dtype=torch.float32).to(dev)
        auto = value_range(value, valid) if rng is None else None
        return paint(value, valid, frame, table.to(dev), block, auto, inverse, out)


class RenderStage:
    """The display stage of ``umamd.deploy.DepthPipeline``: its arguments,
    checked on the host, its buffers, its launches and its output."""

    keys = RENDER_PARAMS  # of ``params`` and ``block``: what set_params takes

    def __init__(self, render, colour_map, render_range, opacity, invalid_opacity, inverse):
        if not isinstance(render, str) or render not in RENDERS:
            raise ValueError(f'DepthPipeline: render={render!r}: None or one of {RENDERS}')
        self.which = render
        self.table = lut(colour_map)
        bad = ValueError(f"DepthPipeline: render_range={render_range!r}: (lo, hi) or 'auto'")
        if isinstance(render_range, str):
            if render_range != 'auto':
                raise bad
            rng = None
        else:
            try:
                lo, hi = render_range
            except (TypeError, ValueError):
                raise bad from None
            rng = check_range(lo, hi, 'DepthPipeline: render_range')
            if rng is None:
                raise ValueError("DepthPipeline: render_range=(None, None): (lo, hi) or 'auto'")
        self.auto = rng is None
        lo, hi = rng or (0.0, 1.0)  # 'auto': replaced by the device range
        self.params = {'render_lo': lo, 'render_hi': hi,
                       'opacity': check_number('DepthPipeline: opacity', opacity),
                       'invalid_opacity': check_number('DepthPipeline: invalid_opacity',
                                                       invalid_opacity)}
        self.inverse = bool(inverse)

    def allocate(self, dev, B, Hs, Ws):
        self.block = torch.tensor(list(self.params.values()), dtype=torch.float32, device=dev)
        self._lut = self.table.to(dev)
        self._out = torch.zeros((B, Hs, Ws, 3), dtype=torch.uint8, device=dev)
        self._range = self._range_ws = None
        if self.auto:
            self._range = torch.zeros(2, dtype=torch.float32, device=dev)
            self._range_ws = torch.zeros(query('um_value_range_ws', B * Hs * Ws),
                                         dtype=torch.uint8, device=dev)

    def run(self, maps, frames):
        """``maps``: the pipeline's disparity, depth, uncertainty, lr_error and
        valid (uint8) buffers; ``frames`` the frame they were computed from"""
        value = maps[self.which]
        if self.auto:
            value_range(value, maps['valid'], out=self._range, ws=self._range_ws)
        paint(value, maps['valid'], frames, self._lut, self.block, self._range, self.inverse,
              self._out)

    def outputs(self):
        return {'render': self._out}

    def check_params(self, kw):
        """the stage's part of set_params, checked (nothing is written yet)"""
        fixed = [k for k in ('render_lo', 'render_hi') if k in kw]
        if fixed and self.auto:
            raise ValueError(f"DepthPipeline.set_params: {fixed} on a pipeline built with "
                             f"render_range='auto' (the range is found per call)")
        return {k: check_number(f'DepthPipeline.set_params: {k}', v) for k, v in kw.items()}

    def write(self, checked):
        """``checked`` into the host dict and the device block, in place"""
        write_block(self.block, self.params, self.keys, checked)
