"""The rectification stage without a GPU: the numpy restatement of
tests/_rectify_ref.py against its own f64 form and against cases with a known
answer (identity, translations, a half-pixel shift, a ramp, special
coordinates), the two C-ABI entries in the header and the binding,
umamd.rectify.Calibration / RemapTable, and every error that umamd.rectify and
DepthPipeline(rectify=...) raise before any GPU work."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import _rectify_ref as R

ENTRIES = ('um_frame_rectify', 'um_valid_and')
OUT = -2 ** 31


def test_entries_in_header_and_binding():
    from umamd import _lib
    src = open(os.path.join(REPO, 'include', 'umamd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib._SIG and hasattr(L, name), name
    assert os.path.isfile(os.path.join(REPO, 'uncertainty-model_amd', 'csrc', 'rectify.hip'))
    assert 'INT32_MIN' in src and 'own rounding' in src


@pytest.mark.parametrize('name', ['small', 'rational', 'full'])
def test_f32_coordinates_against_f64(name):
    """The f32 restatement against the f64 restatement of the same f32 block:
    the Q5 coordinates differ by at most 1 unit in at most 1 % of the pixels (a
    cap, not a measurement; the restatement reads no pixel for 'small', 0.05 %
    for 'rational', 0.25 % for 'full').  The inside share lies strictly between
    0.5 and 0.99, so both branches of the mask are exercised."""
    cal = R.calibration(name, size=None if name == 'full' else (41, 50))
    Hs, Ws = R.RAW[name]
    Hr, Wr = cal.out_size((Hs, Ws))
    q32 = [R.q5(c) for c in R.coords_ref(cal.block(), Hr, Wr, np.float32)]
    q64 = [R.q5(c) for c in R.coords_ref(cal.block(), Hr, Wr, np.float64)]
    assert not any((q == OUT).any() for q in q32 + q64)
    diff = np.maximum(np.abs(q32[0].astype(np.int64) - q64[0]),
                      np.abs(q32[1].astype(np.int64) - q64[1]))
    share = float((diff > 0).mean())
    inside = float(R.inside_ref(q32[0], q32[1], Hs, Ws).mean())
    print(f'{name}: max Q5 difference {int(diff.max())}, in {share:.4%} of the pixels; '
          f'inside {inside:.1%}')
    assert int(diff.max()) <= 1 and share <= 0.01
    assert 0.5 < inside < 0.99


def test_identity():
    """no distortion, R = I, P = K, the same size: q = (32 u, 32 v) exactly, the
    output is the input and every pixel is inside"""
    from umamd.rectify import Calibration
    for K in ((60.3, 58.9, 26.1, 18.4), (1035.3, 1034.9, 596.5, 520.4)):
        cal = Calibration(K, (0.0, 0.0, 0.0, 0.0))
        Hs, Ws = (37, 53) if K[0] < 100 else (130, 170)
        qx, qy = R.q_of(cal, (Hs, Ws))
        assert np.array_equal(qx, np.broadcast_to(32 * np.arange(Ws)[None, :], (Hs, Ws)))
        assert np.array_equal(qy, np.broadcast_to(32 * np.arange(Hs)[:, None], (Hs, Ws)))
        f = R.frames(2, Hs, Ws, seed=3)
        out, inside = R.rectify_ref(f, cal)
        assert torch.equal(out, f) and bool((inside == 1).all())


def _grid(Hr, Wr):
    v, u = np.meshgrid(np.arange(Hr, dtype=np.float32), np.arange(Wr, dtype=np.float32),
                       indexing='ij')
    return u, v


def test_table_translation():
    """a pure integer translation by (+3, -2): the shifted image with a zero
    border, and the exact rectangle as inside"""
    from umamd.rectify import RemapTable
    Hs, Ws = 11, 17
    f = R.frames(2, Hs, Ws, seed=4)
    u, v = _grid(Hs, Ws)
    out, inside = R.rectify_ref(f, RemapTable(u + 3, v - 2))
    want = torch.zeros_like(f)
    want[:, 2:, :Ws - 3] = f[:, :Hs - 2, 3:]
    rect = torch.zeros(Hs, Ws, dtype=torch.uint8)
    rect[2:, :Ws - 3] = 1
    assert torch.equal(out, want) and torch.equal(inside, rect)


def test_table_half_pixel_shift():
    """half a pixel to the right: (a + b + 1) >> 1 of the two neighbours; the
    last column blends with the border"""
    from umamd.rectify import RemapTable
    Hs, Ws = 9, 14
    f = R.frames(1, Hs, Ws, seed=5)
    u, v = _grid(Hs, Ws)
    out, inside = R.rectify_ref(f, RemapTable(u + 0.5, v))
    a = f.to(torch.int32)
    b = torch.cat([a[:, :, 1:], torch.zeros_like(a[:, :, :1])], 2)
    assert torch.equal(out, ((a + b + 1) >> 1).to(torch.uint8))
    assert bool((inside[:, :-1] == 1).all()) and bool((inside[:, -1] == 0).all())
    out, _ = R.rectify_ref(f, RemapTable(u, v + 0.5))
    b = torch.cat([a[:, 1:], torch.zeros_like(a[:, :1])], 1)
    assert torch.equal(out, ((a + b + 1) >> 1).to(torch.uint8))


@pytest.mark.parametrize('name', ['small', 'rational'])
def test_ramp(name):
    """Bilinear interpolation is exact on the ramp src[y][x] = (2x + y, x, y)
    (raw sizes below 128: nothing clips).  At an inside pixel the result is
    within 1 of round(2 mx + my), mx and my from the f64 map: the Q5 rounding
    moves each coordinate by at most 1/64 px, i.e. the value by at most 3/64, the
    f32 map by at most one more Q5 unit in a coordinate (2/32), and the final
    rounding by 1/2: below 1, so the integers differ by at most 1."""
    cal = R.calibration(name, size=(41, 50))
    Hs, Ws = R.RAW[name]
    y, x = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing='ij')
    ramp = np.stack([2 * x + y, x, y], -1).astype(np.uint8)[None]
    assert int((2 * x + y).max()) < 256
    out, inside = R.rectify_ref(ramp, cal)
    mx, my = R.coords_ref(cal.block(), 41, 50, np.float64)
    keep = inside.numpy() != 0
    assert 0.5 < keep.mean() < 0.99
    got = out.numpy()[0].astype(np.int64)
    for ch, want in enumerate((2 * mx + my, mx, my)):
        err = np.abs(got[..., ch] - np.rint(want))[keep]
        assert err.max() <= 1, (ch, err.max())


def test_special_coordinates():
    """q, the border blend and inside at NaN, +-inf, +-2^21, -0.5, Ws - 1 and
    Ws - 1 + 1/32"""
    from umamd.rectify import RemapTable, q5
    Hs, Ws = 4, 6
    inf, nan = float('inf'), float('nan')
    xs = np.array([nan, inf, -inf, 2.0 ** 21, -2.0 ** 21, -0.5, Ws - 1, Ws - 1 + 1 / 32, 2.0,
                   2.0 ** 20, 2.0 ** 20 - 1], np.float32)
    want_q = [OUT, OUT, OUT, OUT, OUT, -16, 32 * (Ws - 1), 32 * (Ws - 1) + 1, 64, OUT,
              32 * (2 ** 20 - 1)]
    assert R.q5(xs).tolist() == want_q and q5(xs).tolist() == want_q
    assert R.q5(xs.astype(np.float64)).tolist() == want_q
    assert R.q5(np.array([0.515625, 0.546875, -0.015625], np.float32)).tolist() == [16, 18, 0]
    f = R.frames(1, Hs, Ws, seed=6)
    mx = np.tile(xs[:, None], (1, 2)).T.copy()  # [2, 11]: every special x on rows y = 1 and y = nan
    my = np.stack([np.full(len(xs), 1.0, np.float32), np.full(len(xs), nan, np.float32)])
    out, inside = R.rectify_ref(f, RemapTable(mx, my))
    a = f[0].to(torch.int32)
    assert not out[0, 1].any() and not inside[1].any()  # y is OUT: black, outside
    assert inside[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0]
    for j in (0, 1, 2, 3, 4, 9, 10):
        assert not out[0, 0, j].any(), j
    # half of the first pixel, half border
    assert torch.equal(out[0, 0, 5], ((16 * 32 * a[1, 0] + 512) >> 10).to(torch.uint8))
    assert torch.equal(out[0, 0, 6], f[0, 1, Ws - 1])
    assert torch.equal(out[0, 0, 7], ((31 * 32 * a[1, Ws - 1] + 512) >> 10).to(torch.uint8))
    assert torch.equal(out[0, 0, 8], f[0, 1, 2])


def test_calibration_object():
    from umamd.rectify import Calibration, RemapTable
    K, P = (60.3, 58.9, 26.1, 18.4), (48.0, 47.0, 24.5, 20.0)
    c = Calibration(K, (-0.31, 0.12, 0.0011, -0.0007), P=P, baseline=4.5)
    assert c.intrinsics == P and c.focal_baseline == 48.0 * 4.5
    assert c.out_size((37, 53)) == (37, 53)
    assert Calibration(K, (0, 0, 0, 0), size=(41, 50)).out_size((37, 53)) == (41, 50)
    with pytest.raises(ValueError, match='baseline'):
        Calibration(K, (0, 0, 0, 0)).focal_baseline
    assert Calibration(K, (0, 0, 0, 0)).intrinsics == K  # P defaults to K
    b = c.block()
    assert b.dtype == np.float32 and b.shape == (24,) and not b[21:].any()
    assert b[:4].tolist() == [np.float32(x) for x in K]
    # 4, 5 and 8 coefficients with the extra ones zero: the same block
    d4 = (-0.31, 0.12, 0.0011, -0.0007)
    for d in (d4 + (0.0,), d4 + (0.0, 0.0, 0.0, 0.0)):
        assert np.array_equal(Calibration(K, d, P=P).block(), b)
    d8 = Calibration(K, d4 + (-0.02, 0.05, -0.01, 0.002)).block()
    assert d8[4:12].tolist() == [np.float32(x) for x in
                                 (-0.31, 0.12, 0.0011, -0.0007, -0.02, 0.05, -0.01, 0.002)]
    # matrices and tuples are the same camera; m = inv(K_new R) from f64
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    Pm = np.array([[P[0], 0, P[2], -200.0], [0, P[1], P[3], 0], [0, 0, 1, 0]])
    Rm = R.rot(0.015, -0.03, 0.02)
    c2 = Calibration(Km, d4, R=Rm, P=Pm)
    assert np.array_equal(c2.block(), Calibration(K, d4, R=Rm, P=P).block())
    assert c2.intrinsics == P
    assert np.array_equal(c2.block()[12:21],
                          np.linalg.inv(Pm[:, :3] @ Rm).astype(np.float32).reshape(-1))
    assert np.array_equal(Calibration(K, d4, P=torch.tensor(P, dtype=torch.float64)).block(), b)
    t = RemapTable(torch.zeros(5, 7), np.ones((5, 7))).table()
    assert t.dtype == torch.int32 and t.shape == (5, 7, 2)
    assert not t[..., 0].any() and bool((t[..., 1] == 32).all())


def test_calibration_and_table_errors():
    from umamd.rectify import Calibration, RemapTable
    K, d = (60.3, 58.9, 26.1, 18.4), (0.0, 0.0, 0.0, 0.0)
    nan, inf = float('nan'), float('inf')
    for bad in (None, 7.0, K[:3], K + (1.0,), (nan,) + K[1:], (60.3, inf, 1.0, 1.0), np.eye(4),
                ('a', 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match='Calibration: K'):
            Calibration(bad, d)
    for bad in ((0.0, 58.9, 26.1, 18.4), (60.3, 0.0, 26.1, 18.4)):
        with pytest.raises(ValueError, match='focal length'):
            Calibration(bad, d)
        with pytest.raises(ValueError, match='focal length'):
            Calibration(K, d, P=bad)
    for bad in (None, (), (0.0,) * 3, (0.0,) * 6, (0.0,) * 7, (0.0,) * 9, (0.0, nan, 0.0, 0.0),
                (0.0, 0.0, inf, 0.0, 0.0), 'abcd'):
        with pytest.raises(ValueError, match='Calibration: dist'):
            Calibration(K, bad)
    for bad in (np.eye(2), np.zeros((3, 4)), np.full((3, 3), nan), 'R'):
        with pytest.raises(ValueError, match='Calibration: R'):
            Calibration(K, d, R=bad)
    for bad in (np.zeros((3, 3)), np.ones((3, 3))):
        with pytest.raises(ValueError, match='not invertible'):
            Calibration(K, d, R=bad)
    with pytest.raises(ValueError, match='not invertible'):
        Calibration(K, d, P=np.array([[48.0, 0, 24], [0, 48.0, 20], [2 * 48.0, 0, 48]]))
    for bad in (np.zeros((4, 3)), K[:2], (48.0, nan, 1.0, 1.0)):
        with pytest.raises(ValueError, match='Calibration: P'):
            Calibration(K, d, P=bad)
    for bad in ((1, 5), (5, 1), (4.0, 5), 5, (4, 5, 6), (True, 5), "ab"):
        with pytest.raises(ValueError, match='size'):
            Calibration(K, d, size=bad)
    for bad in (nan, inf, 'b', (1.0, 2.0)):
        with pytest.raises(ValueError, match='baseline'):
            Calibration(K, d, baseline=bad)
    ok = np.zeros((4, 5), np.float32)
    with pytest.raises(TypeError, match='map_x'):
        RemapTable(ok.astype(np.int32), ok)
    with pytest.raises(TypeError, match='map_y'):
        RemapTable(ok, torch.zeros(4, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match='map_x'):
        RemapTable(ok[0], ok)
    with pytest.raises(ValueError, match='map_y'):
        RemapTable(ok, ok[:1])
    with pytest.raises(ValueError, match='differ'):
        RemapTable(ok, ok[:3])


def test_rectify_errors_before_gpu_work():
    from umamd._lib import UmamdError
    from umamd.rectify import RemapTable, rectify
    cal = R.calibration('small', size=(41, 51))
    f = R.frames(2, 37, 53, seed=1)
    with pytest.raises(TypeError, match='Calibration or a RemapTable'):
        rectify(f, cal.block())
    with pytest.raises(TypeError, match='frames'):
        rectify(f.float(), cal)
    with pytest.raises(TypeError, match='frames'):
        rectify(f.numpy(), cal)
    for bad in (f[0], f[..., :2], f.transpose(1, 2), f[:, :, ::2]):
        with pytest.raises(ValueError, match='frames'):
            rectify(bad, cal)
    with pytest.raises(ValueError, match='raw size'):
        rectify(f[:, :1].contiguous(), cal)
    with pytest.raises(ValueError, match='output pixels'):
        rectify(f[:0], cal)
    with pytest.raises(TypeError, match='out'):
        rectify(f, cal, out=torch.zeros(2, 41, 51, 3))
    with pytest.raises(ValueError, match='out'):
        rectify(f, cal, out=torch.zeros(2, 37, 53, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match='inside'):
        rectify(f, cal, inside=torch.zeros(41, 51, dtype=torch.bool))
    with pytest.raises(ValueError, match='inside'):
        rectify(f, cal, inside=torch.zeros(2, 41, 51, dtype=torch.uint8))
    # well-formed: the first GPU work is what fails on this host
    with pytest.raises(UmamdError, match='HIP device'):
        rectify(f, cal)
    with pytest.raises(UmamdError, match='HIP device'):
        rectify(f, RemapTable(np.zeros((5, 7), np.float32), np.zeros((5, 7), np.float32)),
                out=torch.zeros(2, 5, 7, 3, dtype=torch.uint8),
                inside=torch.zeros(5, 7, dtype=torch.uint8))


def test_pipeline_rectify_argument_errors_without_gpu():
    from test_deploy_cpu import _cpu_model
    from umamd._lib import UmamdError
    from umamd.deploy import DepthPipeline
    from umamd.rectify import RemapTable
    m = _cpu_model()
    cal = R.calibration('small', size=(64, 128))

    def build(hs=96, ws=160, **kw):
        return DepthPipeline(m, hs, ws, **{**dict(height=32, width=64), **kw})
    for bad in (cal.block(), 'small', (60.3, 58.9, 26.1, 18.4), True, 1):
        with pytest.raises(TypeError, match='DepthPipeline: rectify'):
            build(rectify=bad)
    with pytest.raises(ValueError, match='DepthPipeline: rectify: raw size'):
        build(hs=1, rectify=cal)
    with pytest.raises(ValueError, match='DepthPipeline: rectify: raw size'):
        build(ws=32768, rectify=cal)
    with pytest.raises(ValueError, match='output pixels'):
        build(rectify=R.calibration('small', size=(32768, 32768)), batch=2)
    # the later stages are built for the rectified size: its resize limit counts
    with pytest.raises(ValueError, match='source size 4000x128'):
        build(rectify=R.calibration('small', size=(4000, 128)))
    tab = RemapTable(np.zeros((64, 128), np.float32), np.zeros((64, 128), np.float32))
    # well-formed: the first GPU work is what fails on this host
    for kw in (dict(rectify=cal), dict(rectify=tab), dict(rectify=R.calibration('small')),
               dict(rectify=cal, render='depth', points='both', intrinsics=cal.intrinsics)):
        with pytest.raises(UmamdError, match='HIP device'):
            build(**kw)
    assert not any(p.is_cuda for p in m.parameters())
