"""The deployment path without a GPU: the references of tests/_deploy_ref.py
against their own definitions and PIL, the three C-ABI entries in the header
and the binding, the resize gate, and DepthPipeline's argument errors (all
raised before any GPU work)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import _deploy_ref as R

ENTRIES = ('um_frame_prep_ok', 'um_frame_prep', 'um_depth_post')


def _pred(n, h, w, seed=5):
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(n, 2, h, w, generator=g) * 0.5
    s = torch.rand(n, 2, h, w, generator=g) * 0.3
    return torch.cat([d, s], 1)


def test_reference_identity_size():
    """source size = model size: up() is the identity, so disparity = d_L * W
    and uncertainty = sigma_L; depth and the mask follow their definitions"""
    p = _pred(2, 8, 16)
    for dt in (torch.float64, torch.float32):
        r = R.depth_post_ref(p, 8, 16, 100.0, 0.05 * 16, 0.15, 0.2 * 16, dt)
        assert torch.equal(r['disparity'], p[:, 0].to(dt) * 16)
        assert torch.equal(r['uncertainty'], p[:, 2].to(dt))
        far = r['disparity'] > 0.05 * 16
        assert torch.equal(r['depth'][far], 100.0 / r['disparity'][far])
        assert not r['depth'][~far].any()
        assert torch.equal(r['valid'], far & (r['uncertainty'] <= 0.15) &
                           (r['lr_error'] <= 0.2 * 16))
        assert 0 < int(r['valid'].sum()) < r['valid'].numel()
        assert float(r['lr_error'].min()) >= 0


def test_reference_lr_error_is_zero_for_consistent_disparities():
    """d_L = d_R = 0 is consistent wherever the warp stays inside: the
    left-right error is |0 - 0|"""
    p = torch.zeros(1, 4, 8, 16)
    r = R.depth_post_ref(p, 19, 37, 1.0, 1e-3, 1.0, 1.0)
    assert not r['lr_error'].any() and not r['depth'].any() and not r['valid'].any()


def test_frame_prep_ref_matches_pil():
    from PIL import Image
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    got = R.frame_prep_ref(torch.from_numpy(img), 16, 24)
    assert got.shape == (2, 3, 16, 24) and got.dtype == torch.float32
    for i in range(2):
        pil = np.asarray(Image.fromarray(img[i]).resize((24, 16), Image.BILINEAR))
        assert torch.equal(got[i], torch.from_numpy(pil.copy()).permute(2, 0, 1).float().div(255))


def test_entries_in_header_and_binding():
    from umamd import _lib
    src = open(os.path.join(REPO, 'include', 'umamd.h')).read()
    assert 'deployment ---' in src
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib._SIG, name
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name)


def _ks(n_in, n_out):
    from umamd.imageprep import resize_coeffs
    return resize_coeffs(n_in, n_out)[2]


def test_resize_gate():
    """every upscale and every downscale up to 8x per axis passes; the limit
    is the one the header states (vertical: ceil(7 Hs / Hd) + 1 + ks_v <= 512
    source rows; horizontal: ks_h <= 257)"""
    from umamd._lib import query

    def ok(hs, ws, hd, wd):
        return query('um_frame_prep_ok', hs, ws, hd, wd, _ks(ws, wd), _ks(hs, hd))
    for hs, ws, hd, wd in ((1024, 1280, 256, 512), (12, 20, 16, 24), (16, 24, 16, 24),
                           (2, 2, 2048, 4096), (2048, 4096, 256, 512), (8 * 352, 8 * 640, 352, 640),
                           (37, 53, 16, 24), (113, 256, 2, 2)):
        assert ok(hs, ws, hd, wd) == 1, (hs, ws, hd, wd)
        assert -(-7 * hs // hd) + 1 + _ks(hs, hd) <= 512 and _ks(ws, wd) <= 257
    assert ok(114, 256, 2, 2) == 0      # 399 + 1 + 115 = 515 rows
    assert ok(113, 258, 2, 2) == 0      # ks_h = 259
    assert ok(57 * 256, 512, 256, 512) == 0
    assert query('um_frame_prep_ok', 0, 4, 4, 4, 3, 3) == 0


def _cpu_model():
    import yaml
    import model as M
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)
    cfg['model']['encoder']['load_graph'] = os.path.join(REPO, cfg['model']['encoder']['load_graph'])
    return M.RandomlyConnectedModel(**cfg['model'])


def test_pipeline_argument_errors_without_gpu():
    from umamd._lib import UmamdError
    from umamd.deploy import DepthPipeline, _check_frames
    m = _cpu_model()
    with pytest.raises(ValueError, match='multiples of 32'):
        DepthPipeline(m, 150, 262, height=60, width=128)
    with pytest.raises(ValueError, match='multiples of 32'):
        DepthPipeline(m, 150, 262, height=64, width=100)
    with pytest.raises(ValueError, match='at least 2'):
        DepthPipeline(m, 1, 262, height=64, width=128)
    with pytest.raises(ValueError, match='at least 2'):
        DepthPipeline(m, 150, 1, height=64, width=128)
    with pytest.raises(ValueError, match=r'56x.*512 source rows.*64 KiB'):
        DepthPipeline(m, 57 * 64, 262, height=64, width=128)
    with pytest.raises(ValueError, match=r'ks_h <= 257'):
        DepthPipeline(m, 150, 129 * 128, height=64, width=128)
    with pytest.raises(UmamdError, match='HIP device'):
        DepthPipeline(m, 150, 262, height=64, width=128)
    # what __call__ checks before it touches the device
    shape = (2, 150, 262, 3)
    _check_frames(torch.zeros(shape, dtype=torch.uint8), shape)
    with pytest.raises(TypeError, match='uint8'):
        _check_frames(torch.zeros(shape, dtype=torch.float32), shape)
    with pytest.raises(TypeError, match='uint8'):
        _check_frames(np.zeros(shape, np.uint8), shape)
    for bad in ((1, 150, 262, 3), (2, 262, 150, 3), (2, 3, 150, 262), (2, 150, 262)):
        with pytest.raises(ValueError, match='built for frames'):
            _check_frames(torch.zeros(bad, dtype=torch.uint8), shape)
    assert not any(p.is_cuda for p in m.parameters())
