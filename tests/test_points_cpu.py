"""The point stage without a GPU: the reference of tests/_points_ref.py against
an f64 restatement on inputs where both are exact, the workspace query, the
three C-ABI entries in the header and the binding, and every error that
umamd.points and DepthPipeline(points=...) raise before any GPU work."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import _points_ref as R

ENTRIES = ('um_depth_backproject', 'um_depth_cloud_ws', 'um_depth_cloud')
TILE = 1024  # lattice sites of a tile (include/umamd.h)
INT_MAX = 2 ** 31 - 1


def test_entries_in_header_and_binding():
    from umamd import _lib
    src = open(os.path.join(REPO, 'include', 'umamd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib._SIG and hasattr(L, name), name
    assert os.path.isfile(os.path.join(REPO, 'uncertainty-model_amd', 'csrc', 'points.hip'))
    assert 'cx - 0.5' in src and 'unspecified' in src  # the two conventions a caller must know


def test_reference_equals_f64_on_exact_inputs():
    """integer depths up to 64, integer cx and cy, power-of-two focal lengths:
    u - cx, its product with Z (below 2^24) and the quotient are exact in f32
    and in f64, so the two restatements must agree to the bit"""
    g = torch.Generator().manual_seed(1)
    shape = (2, 19, 37)
    depth = torch.randint(1, 65, shape, generator=g).float()
    valid = (torch.rand(shape, generator=g) < 0.6).to(torch.uint8)
    unc = torch.randint(0, 9, shape, generator=g).float() / 8
    frame = torch.randint(0, 256, shape + (3,), generator=g, dtype=torch.uint8)
    intr = (512.0, 256.0, 18.0, 9.0)
    m32 = R.backproject_ref(depth, intr, valid)
    m64 = R.backproject_ref(depth, intr, valid, dtype=np.float64)
    assert m32.dtype == torch.float32 and m64.dtype == torch.float64
    assert torch.equal(m32.double(), m64)
    # spot values of the definition
    assert m32[1, 7, 30].tolist() == ([(30 - 18) * float(depth[1, 7, 30]) / 512,
                                       (7 - 9) * float(depth[1, 7, 30]) / 256,
                                       float(depth[1, 7, 30])] if valid[1, 7, 30] else [0, 0, 0])
    assert not m32[valid == 0].any() and bool((m32[valid != 0][:, 2] > 0).all())
    for stride in (1, 2, 3):
        a = R.cloud_ref(depth, intr, valid, unc, frame, stride)
        b = R.cloud_ref(depth, intr, valid, unc, frame, stride, dtype=np.float64)
        assert torch.equal(a[0].double(), b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[2], b[2])
        # the cloud is the organised map's lattice, in order
        lat_valid = valid[:, ::stride, ::stride] != 0
        assert torch.equal(a[0][:, :3], m32[:, ::stride, ::stride][lat_valid])
        assert torch.equal(a[0][:, 3], unc[:, ::stride, ::stride][lat_valid])
        assert torch.equal(a[1][:, :3], frame[:, ::stride, ::stride][lat_valid])
        assert bool((a[1][:, 3] == 255).all())
        assert a[2].tolist() == [0, int(lat_valid[0].sum()), int(lat_valid.sum())]
    x = R.cloud_ref(depth, intr)  # nothing optional: all kept, fourth value 0, no colours
    assert x[1] is None and len(x[0]) == depth.numel() and not x[0][:, 3].any()


def test_planted_inputs():
    depth, valid, unc, frame = R.planted((2, 67, 129), seed=3)
    bad = ~torch.isfinite(depth) | (depth < 0.5)
    assert int(torch.isnan(depth).sum()) > 100 and int(torch.isinf(depth).sum()) > 200
    assert int((depth < 0).sum()) > 200
    assert not bool((bad & (valid != 0)).any())
    assert 0.55 < float(valid.float().mean()) < 0.65
    ref = R.backproject_ref(depth, R.INTR, valid)
    assert bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(R.cloud_ref(depth, R.INTR, valid, unc, frame, 2)[0]).all())


def test_cloud_workspace_query():
    """4 bytes per tile of 1024 lattice sites, tiles counted per image;
    0 for what um_depth_cloud refuses"""
    from umamd._lib import query

    def ws(n, h, w, s=1):
        return query('um_depth_cloud_ws', n, h, w, s)
    assert ws(1, 1, 1) == 4 and ws(1, 3, 5) == 4 and ws(1, 32, 32) == 4
    assert ws(1, 32, 33) == 8  # 1056 sites
    assert ws(3, 33, 67) == 3 * 3 * 4  # 2211 sites an image: tiles do not span images
    assert ws(2, 67, 129, 2) == 2 * 3 * 4 and ws(2, 67, 129, 3) == 2 * 1 * 4  # 34 x 65, 23 x 43
    assert ws(8, 1080, 1920) == 8 * 2025 * 4
    prev = 0
    for h in range(1, 200, 7):  # monotone in the tile count
        tiles = -(-h * 129 // TILE)
        assert ws(2, h, 129) == 2 * tiles * 4 >= prev > -1
        prev = ws(2, h, 129)
    for bad in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (-1, 4, 4, 1),
                (1, 4, 4, -2)):
        assert ws(*bad) == 0, bad
    assert ws(2, 32768, 32768) == 0  # 2^31 sites
    assert ws(1, 32768, 65535) > 0 and ws(1, 32768, 65536) == 0
    assert ws(2, 65536, 65536, 2) == 0 and ws(1, 65536, 65536, 2) > 0
    assert ws(INT_MAX, 2, 1, 2) == 0  # N * Hs rows
    assert ws(INT_MAX, 1, 1, 1) == 4 * INT_MAX


def test_check_intrinsics():
    from umamd.points import check_intrinsics
    assert check_intrinsics((500, 501.5, 320, 240.25)) == (500.0, 501.5, 320.0, 240.25)
    assert check_intrinsics([-500.0, 500.0, 0, 0]) == (-500.0, 500.0, 0.0, 0.0)
    for bad in (None, 7.0, (1.0, 1.0, 0.0), (1.0, 1.0, 0.0, 0.0, 0.0), (),
                (0.0, 1.0, 0.0, 0.0), (1.0, 0, 0.0, 0.0),
                (float('nan'), 1.0, 0.0, 0.0), (1.0, float('inf'), 0.0, 0.0),
                (1.0, 1.0, float('-inf'), 0.0), (1.0, 1.0, 0.0, float('nan')),
                ('1', 1.0, 0.0, 0.0), (1.0, 1.0, None, 0.0), (True, 1.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match='intrinsics'):
            check_intrinsics(bad)
    with pytest.raises(ValueError, match='somebody: intrinsics'):
        check_intrinsics((0, 0, 0, 0), 'somebody')


def test_cloud_and_backproject_errors_before_gpu_work():
    from umamd._lib import UmamdError
    from umamd.points import backproject, cloud
    d = torch.rand(2, 4, 6) + 1
    k = (100.0, 100.0, 3.0, 2.0)
    ok = dict(valid=torch.ones(2, 4, 6, dtype=torch.bool), uncertainty=torch.rand(2, 4, 6),
              frame=torch.zeros(2, 4, 6, 3, dtype=torch.uint8))
    for fn in (backproject, cloud):
        with pytest.raises(TypeError, match='depth'):
            fn(d.double(), k)
        with pytest.raises(TypeError, match='depth'):
            fn(d.numpy(), k)
        with pytest.raises(ValueError, match='depth'):
            fn(d.transpose(1, 2), k)
        with pytest.raises(ValueError, match='depth'):
            fn(d[0, 0], k)
        with pytest.raises(ValueError, match='depth'):
            fn(d[:0], k)
        with pytest.raises(ValueError, match='intrinsics'):
            fn(d, (0.0, 100.0, 3.0, 2.0))
        with pytest.raises(ValueError, match='intrinsics'):
            fn(d, k[:3])
        with pytest.raises(TypeError, match='valid'):
            fn(d, k, valid=torch.ones(2, 4, 6))
        with pytest.raises(ValueError, match='valid'):
            fn(d, k, valid=torch.ones(2, 6, 4, dtype=torch.bool))
        with pytest.raises(UmamdError, match='HIP device'):
            fn(d, k, valid=ok['valid'])
    with pytest.raises(TypeError, match='uncertainty'):
        cloud(d, k, uncertainty=torch.rand(2, 4, 6).double())
    with pytest.raises(ValueError, match='uncertainty'):
        cloud(d, k, uncertainty=torch.rand(2, 4, 7))
    with pytest.raises(TypeError, match='frame'):
        cloud(d, k, frame=torch.zeros(2, 4, 6, 3))
    with pytest.raises(ValueError, match='frame'):
        cloud(d, k, frame=torch.zeros(2, 3, 4, 6, dtype=torch.uint8))
    for bad in (0, -1, 1.0, '2', None, True):
        with pytest.raises(ValueError, match='stride'):
            cloud(d, k, stride=bad)
    with pytest.raises(UmamdError, match='HIP device'):
        cloud(d, k, stride=2, **ok)
    with pytest.raises(UmamdError, match='HIP device'):
        cloud(d[0], k)


def test_pipeline_points_argument_errors_without_gpu():
    from test_deploy_cpu import _cpu_model
    from umamd._lib import UmamdError
    from umamd.deploy import DepthPipeline
    m = _cpu_model()
    k = (900.0, 900.0, 131.0, 75.0)

    def build(**kw):
        return DepthPipeline(m, 150, 262, **{**dict(height=64, width=128), **kw})
    for bad in ('xyz', 'points', 'depth', 1, True, ('map',)):
        with pytest.raises(ValueError, match='points='):
            build(points=bad, intrinsics=k)
    for mode in ('map', 'cloud', 'both'):
        with pytest.raises(ValueError, match='needs intrinsics'):
            build(points=mode)
    for bad in ((0.0, 900.0, 131.0, 75.0), (900.0, 0.0, 131.0, 75.0), k[:3], k + (1.0,), 900.0,
                (900.0, 900.0, float('nan'), 75.0), (900.0, float('inf'), 131.0, 75.0),
                ('900', 900.0, 131.0, 75.0)):
        with pytest.raises(ValueError, match='DepthPipeline: intrinsics'):
            build(points='cloud', intrinsics=bad)
    for bad in (0, -2, 1.5, '2', None):
        with pytest.raises(ValueError, match='point_stride'):
            build(points='cloud', intrinsics=k, point_stride=bad)
    with pytest.raises(ValueError, match=r"point_stride=2 with points='map'"):
        build(points='map', intrinsics=k, point_stride=2)
    # the point stage's errors come first, like the display stage's
    with pytest.raises(ValueError, match='points='):
        build(points='nope', intrinsics=k, height=60)
    # well-formed: the first GPU work is what fails on this host
    for kw in (dict(points='map'), dict(points='cloud', point_stride=2), dict(points='both'),
               dict(points='both', point_stride=3, render='depth')):
        with pytest.raises(UmamdError, match='HIP device'):
            build(intrinsics=k, **kw)
    with pytest.raises(UmamdError, match='HIP device'):
        build(intrinsics=k)  # intrinsics without points: ignored, as colour_map without render
    assert not any(p.is_cuda for p in m.parameters())
