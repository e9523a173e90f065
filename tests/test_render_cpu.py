"""The display stage without a GPU: the committed table against matplotlib,
the reference of tests/_render_ref.py against the host path it restates
(train.utils.to_heatmap -> save_image's rounding, and the min/max-scaled
heatmap of get_comparison), the integer blend, and every error that
umamd.render and DepthPipeline raise before any GPU work."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import _render_ref as R

ENTRIES = ('um_value_range_ws', 'um_value_range', 'um_depth_render')


def _save_image_bytes(img):
    """save_image's rounding of a [3, H, W] image in [0, 1] -> uint8 [H, W, 3]"""
    return img.float().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def test_entries_in_header_and_binding():
    from umamd import _lib
    src = open(os.path.join(REPO, 'include', 'umamd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib._SIG and hasattr(L, name), name
    assert os.path.isfile(os.path.join(REPO, 'uncertainty-model_amd', 'csrc', 'render.hip'))
    # the workspace: one (lo, hi) pair per workgroup of 1024 pixels, at most 256
    q = _lib.query
    assert [q('um_value_range_ws', n) for n in (0, 1, 1024, 1025, 480 * 640, 1 << 33)] == \
        [0, 8, 8, 16, 2048, 2048]


def test_inferno_table_is_matplotlibs():
    from umamd.render import lut
    t = lut('inferno')
    assert t.dtype == torch.uint8 and tuple(t.shape) == (256, 3)
    assert torch.equal(t, R.lut_rule('inferno'))
    assert torch.equal(lut(), t)
    assert torch.equal(lut('viridis'), R.lut_rule('viridis'))


@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('cmap', ['inferno', 'viridis'])
def test_reference_is_to_heatmap_then_save_image(cmap, inverse):
    from train.utils import to_heatmap
    from umamd.render import lut
    v = R.planted((67, 129), seed=3)
    assert int(torch.isnan(v).sum()) == 1 and int(torch.isinf(v).sum()) == 2
    want = _save_image_bytes(to_heatmap(v.unsqueeze(0), inverse=inverse, colour_map=cmap))
    got = R.render_ref(v, lut(cmap), 0.0, 1.0, inverse=inverse)
    assert got.dtype == torch.uint8 and got.shape == (67, 129, 3)
    assert torch.equal(got, want)


def test_reference_is_get_comparisons_scaled_heatmap():
    """(v - min) / (max - min) as get_comparison(add_scaled=True) forms it,
    then to_heatmap: the reference with lo = min, hi = max"""
    from train.utils import get_comparison, to_heatmap
    from umamd.render import lut
    g = torch.Generator().manual_seed(4)
    pred = torch.rand(2, 37, 53, generator=g) * 0.3 + 0.01
    lo, hi = pred.min(), pred.max()
    got = R.render_ref(pred[0], lut('inferno'), lo, hi)
    scaled = (pred[:1] - lo) / (hi - lo)
    assert torch.equal(got, _save_image_bytes(to_heatmap(scaled)))
    assert torch.equal(torch.stack([lo, hi]), R.value_range_ref(pred))
    # ... and as the grid holds it: row 3 (scaled left | scaled right), left cell
    grid = get_comparison(torch.rand(6, 37, 53, generator=g), pred, None, add_scaled=True)
    cell = grid[:, 2 + 2 * 39:2 + 2 * 39 + 37, 2:2 + 53]
    assert torch.equal(got, _save_image_bytes(cell))


def test_integer_blend_end_points():
    from umamd.render import lut
    assert [R.alpha_q(x) for x in (1.0, 0.0, 0.6, 0.25, -3.0, 7.0, float('nan'))] == \
        [256, 0, 154, 64, 0, 256, 0]
    c = torch.arange(256, dtype=torch.int32).view(-1, 1).expand(256, 256)
    f = torch.arange(256, dtype=torch.int32).view(1, -1).expand(256, 256)
    assert torch.equal(R.blend(c, f, torch.tensor(256)), c)
    assert torch.equal(R.blend(c, f, torch.tensor(0)), f)
    mid = R.blend(c, f, torch.tensor(128))
    assert int(mid.min()) == 0 and int(mid.max()) == 255
    # through the reference: opacity 1 is the colour, opacity 0 the frame,
    # invalid pixels take invalid_opacity
    g = torch.Generator().manual_seed(5)
    v = R.planted((3, 5), seed=5)
    frame = torch.randint(0, 256, (3, 5, 3), generator=g, dtype=torch.uint8)
    valid = torch.rand(3, 5, generator=g) < 0.5
    colour = R.render_ref(v, lut(), 0.0, 1.0)
    assert torch.equal(R.render_ref(v, lut(), 0.0, 1.0, frame=frame), colour)
    assert torch.equal(R.render_ref(v, lut(), 0.0, 1.0, opacity=0.0, frame=frame), frame)
    both = R.render_ref(v, lut(), 0.0, 1.0, valid=valid, frame=frame)
    assert torch.equal(both[valid], colour[valid]) and torch.equal(both[~valid], frame[~valid])
    # no valid pixel: the range is (+inf, -inf) and the picture black
    r = R.value_range_ref(v, torch.zeros(3, 5, dtype=torch.bool))
    assert r.tolist() == [float('inf'), float('-inf')]
    assert not R.render_ref(v, lut(), r[0], r[1]).any()


def test_lut_errors():
    from umamd.render import lut
    t = lut('inferno')
    assert lut(t) is not None and torch.equal(lut(t), t)
    assert torch.equal(lut(t.numpy()), t)
    with pytest.raises(ValueError):
        lut('no_such_colour_map')
    with pytest.raises(ValueError, match='256'):
        lut('tab10')  # a 10-entry listed map
    with pytest.raises(ValueError, match=r'\[256, 3\]'):
        lut(t[:255])
    with pytest.raises(ValueError, match=r'\[256, 3\]'):
        lut(t.t().contiguous())
    with pytest.raises(TypeError, match='uint8'):
        lut(t.float())
    with pytest.raises(TypeError, match='uint8'):
        lut(t.numpy().astype(np.float32))
    for bad in (None, 3, [[0, 0, 0]] * 256):
        with pytest.raises(TypeError, match='colour map name'):
            lut(bad)


def test_lut_without_matplotlib(monkeypatch):
    """'inferno' needs no matplotlib; another name says that it does"""
    import sys
    from umamd.render import lut
    monkeypatch.setitem(sys.modules, 'matplotlib', None)
    monkeypatch.setitem(sys.modules, 'matplotlib.pyplot', None)
    assert tuple(lut('inferno').shape) == (256, 3)
    with pytest.raises(ImportError, match='matplotlib'):
        lut('viridis')


def test_colourise_errors_before_gpu_work():
    from umamd._lib import UmamdError
    from umamd.render import colourise
    v = torch.rand(4, 6)
    with pytest.raises(TypeError, match='f32'):
        colourise(v.double(), 0, 1)
    with pytest.raises(TypeError, match='f32'):
        colourise(v.numpy(), 0, 1)
    with pytest.raises(ValueError, match='contiguous'):
        colourise(v.t(), 0, 1)
    with pytest.raises(ValueError, match='go together'):
        colourise(v, lo=0.0)
    with pytest.raises(ValueError, match='go together'):
        colourise(v, hi=1.0)
    with pytest.raises(TypeError, match='number'):
        colourise(v, '0', 1)
    with pytest.raises(TypeError, match='number'):
        colourise(v, 0, 1, opacity='1')
    with pytest.raises(TypeError, match='valid'):
        colourise(v, 0, 1, valid=torch.ones(4, 6))
    with pytest.raises(ValueError, match='valid'):
        colourise(v, 0, 1, valid=torch.ones(6, 4, dtype=torch.bool))
    with pytest.raises(TypeError, match='frame'):
        colourise(v, 0, 1, frame=torch.zeros(4, 6, 3))
    with pytest.raises(ValueError, match='frame'):
        colourise(v, 0, 1, frame=torch.zeros(4, 6, dtype=torch.uint8))
    with pytest.raises(ValueError, match='frame'):
        colourise(v, 0, 1, frame=torch.zeros(3, 4, 6, dtype=torch.uint8))
    with pytest.raises(ValueError, match='out'):
        colourise(v, 0, 1, out=torch.zeros(4, 6, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        colourise(v, 0, 1, colour_map='no_such_colour_map')
    # well-formed, but on the host: the product path has no CPU fallback
    with pytest.raises(UmamdError, match='HIP device'):
        colourise(v, 0, 1, valid=torch.ones(4, 6, dtype=torch.bool),
                  frame=torch.zeros(4, 6, 3, dtype=torch.uint8))
    with pytest.raises(UmamdError, match='HIP device'):
        colourise(v)


def test_pipeline_render_argument_errors_without_gpu():
    from test_deploy_cpu import _cpu_model
    from umamd._lib import UmamdError
    from umamd.deploy import DepthPipeline
    m = _cpu_model()

    def build(**kw):
        return DepthPipeline(m, 150, 262, height=64, width=128, **kw)
    for bad in ('colour', 'valid', 'prediction', 1, True):
        with pytest.raises(ValueError, match='render='):
            build(render=bad)
    for bad in ('fixed', (0.0,), (0.0, 1.0, 2.0), 1.0, None):
        with pytest.raises(ValueError, match='render_range'):
            build(render='depth', render_range=bad)
    with pytest.raises(ValueError, match='go together'):
        build(render='depth', render_range=(0.0, None))
    with pytest.raises(TypeError, match='number'):
        build(render='depth', render_range=('0', '1'))
    with pytest.raises(ValueError):
        build(render='depth', colour_map='no_such_colour_map')
    with pytest.raises(TypeError, match='colour map name'):
        build(render='depth', colour_map=7)
    with pytest.raises(ValueError, match=r'\[256, 3\]'):
        build(render='depth', colour_map=torch.zeros(3, 256, dtype=torch.uint8))
    with pytest.raises(TypeError, match='opacity'):
        build(render='depth', opacity='half')
    with pytest.raises(TypeError, match='invalid_opacity'):
        build(render='depth', invalid_opacity=None)
    # well-formed: the first GPU work is what fails on this host
    with pytest.raises(UmamdError, match='HIP device'):
        build(render='depth', render_range=(0.0, 80.0), opacity=0.6)
    with pytest.raises(UmamdError, match='HIP device'):
        build(render='uncertainty', colour_map='viridis', inverse=True)
    assert not any(p.is_cuda for p in m.parameters())
