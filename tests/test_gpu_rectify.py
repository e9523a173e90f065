"""The rectification stage on the GPU (csrc/rectify.hip, umamd/rectify.py,
DepthPipeline(rectify=...)): um_frame_rectify and um_valid_and against the
numpy restatement of tests/_rectify_ref.py.  Everything is integer output of a
definition fixed to the bit, so every comparison is torch.equal: no tolerance,
no pixel left out.  Outputs are pre-filled with a sentinel and the bytes around
them must stay untouched."""
import numpy as np
import pytest
import torch

import _rectify_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 0xA5
PAD = 64  # sentinel bytes kept behind (and, with an offset, in front of) every output
OUT = -2 ** 31

# B, raw (Hs, Ws), rectified (Hr, Wr): 15 pixels (the scalar tail only); 4182 = 4 k + 2
SHAPES = {'tail': (1, (5, 7), (3, 5)), 'blocks': (2, (37, 53), (41, 51))}
# a camera of the tail's size, so that its 15 pixels sample the frame
TINY = dict(K=(7.9, 7.7, 3.2, 2.1), dist=(-0.2, 0.05, 0.001, -0.002, 0.0),
            R=R.rot(0.02, -0.03, 0.02), P=(4.0, 4.0, 2.2, 1.1))


class Buf:
    """``size`` bytes ``off`` bytes into a sentinel-filled device allocation"""

    def __init__(self, size, off=0, fill=None):
        self.whole = torch.full((off + size + PAD,), SENT, dtype=torch.uint8, device=DEV)
        self.view = self.whole[off:off + size]
        self.off, self.size = off, size
        if fill is not None:
            self.view.copy_(fill.reshape(-1))
        assert self.view.data_ptr() % 4 == off % 4

    def around_untouched(self):
        w = self.whole.cpu()
        return bool((w[:self.off] == SENT).all()) and bool((w[self.off + self.size:] == SENT).all())


def _rectify(frames, hr, wr, cal=None, table=None, offs=(0, 0, 0), with_inside=True):
    """the raw entry -> (dst [B, hr, wr, 3], inside [hr, wr] or None) on the
    host, after checking the bytes around the outputs"""
    from umamd import _lib as L
    b, hs, ws, _ = frames.shape
    src = Buf(frames.numel(), offs[0], frames.to(DEV))
    dst = Buf(b * hr * wr * 3, offs[1])
    ins = Buf(hr * wr, offs[2])
    c = None if cal is None else torch.from_numpy(np.asarray(cal, np.float32)).to(DEV)
    t = None if table is None else table.to(DEV).contiguous()
    L.call('um_frame_rectify', L.ptr(src.view), b, hs, ws, hr, wr, L.ptr(c), L.ptr(t),
           L.ptr(dst.view), L.ptr(ins.view) if with_inside else None)
    torch.cuda.synchronize()
    assert src.around_untouched() and dst.around_untouched() and ins.around_untouched()
    assert torch.equal(src.view.cpu(), frames.reshape(-1))
    if not with_inside:
        assert bool((ins.view == SENT).all())
    return dst.view.cpu().view(b, hr, wr, 3), ins.view.cpu().view(hr, wr) if with_inside else None


def _case(shape, name):
    from umamd.rectify import Calibration
    b, raw, rect = SHAPES[shape]
    cal = Calibration(size=rect, **TINY) if name == 'tiny' else R.calibration(name, size=rect)
    return cal, R.frames(b, *raw, seed=len(name) + b), rect


# -------------------------------------------------------------- analytic --
@pytest.mark.parametrize('shape,name', [('tail', 'small'), ('tail', 'rational'), ('tail', 'tiny'),
                                        ('blocks', 'small'), ('blocks', 'rational')])
def test_analytic_equals_reference(shape, name):
    cal, frames, (hr, wr) = _case(shape, name)
    want, want_in = R.rectify_ref(frames, cal)
    if shape == 'blocks' or name == 'tiny':
        assert 0 < int(want_in.sum()) < want_in.numel() and bool(want.any())
    got, got_in = _rectify(frames, hr, wr, cal=cal.block())
    assert torch.equal(got_in, want_in)
    assert torch.equal(got, want)
    got, _ = _rectify(frames, hr, wr, cal=cal.block(), with_inside=False)  # inside NULL
    assert torch.equal(got, want)


# ----------------------------------------------------------------- table --
def _planted_table():
    """the f32 map of 'small' at 41 x 51 over a 37 x 53 frame with special
    coordinates planted over it"""
    from umamd.rectify import RemapTable
    hs, ws = 37, 53
    mx, my = R.coords_ref(R.calibration('small').block(), 41, 51, np.float32)
    mx, my = mx.copy(), my.copy()
    inf, nan = np.float32('inf'), np.float32('nan')
    specials = [(nan, 5.0), (5.0, nan), (inf, 5.0), (5.0, -inf), (2.0 ** 21, 5.0),
                (5.0, -2.0 ** 21), (-0.5, 5.0), (5.0, -0.5), (-1.0, -1.0), (-1.03125, 3.0),
                (-7.25, 4.5), (ws - 1, hs - 1), (ws - 1 + 1 / 32, hs - 1), (ws - 1, hs - 1 + 1 / 32),
                (ws - 0.5, hs - 0.5), (ws, 3.0), (3.0, hs), (0.0, 0.0), (2.0 ** 20 - 1, 1.0)]
    flat_x, flat_y = mx.reshape(-1), my.reshape(-1)
    for k, (x, y) in enumerate(specials * 6):  # spread over rows and over the lanes of a group
        flat_x[17 * k + 3] = x
        flat_y[17 * k + 3] = y
    flat_x[-1], flat_y[-1] = nan, 1.0  # the last pixel, in the scalar tail
    return RemapTable(mx, my)


def test_table_with_special_coordinates():
    tab = _planted_table()
    t = tab.table()
    assert int((t == OUT).sum()) >= 6 * 6 and int((t < 0).sum()) > 6 * 10
    frames = R.frames(2, 37, 53, seed=8)
    want, want_in = R.rectify_ref(frames, tab)
    assert 0.5 < float(want_in.float().mean()) < 0.99
    got, got_in = _rectify(frames, 41, 51, table=t)
    assert torch.equal(got_in, want_in)
    assert torch.equal(got, want)
    # the table is the analytic map where nothing was planted
    cal = R.calibration('small', size=(41, 51))
    ana, ana_in = _rectify(frames, 41, 51, cal=cal.block())
    qx, qy = R.q_of(cal, (37, 53))
    same = torch.from_numpy((qx == t[..., 0].numpy()) & (qy == t[..., 1].numpy()))
    assert 0.9 < float(same.float().mean()) < 1
    assert torch.equal(ana[:, same], got[:, same]) and torch.equal(ana_in[same], got_in[same])
    # the tail shape through a table
    u, v = np.meshgrid(np.arange(5, dtype=np.float32), np.arange(3, dtype=np.float32))
    from umamd.rectify import RemapTable
    tiny = RemapTable(u * 1.25 - 0.3, v * 1.5 + 0.2)
    f = R.frames(1, 5, 7, seed=9)
    want, want_in = R.rectify_ref(f, tiny)
    got, got_in = _rectify(f, 3, 5, table=tiny.table())
    assert torch.equal(got, want) and torch.equal(got_in, want_in) and bool(want_in.any())


# ------------------------------------------------------- unaligned bases --
@pytest.mark.parametrize('mode', ['analytic', 'table'])
def test_unaligned_bases(mode):
    """src, dst and inside one byte into a larger allocation, in turn and
    together: the same bytes, nothing around them changes (_rectify checks)"""
    cal, frames, (hr, wr) = _case('blocks', 'small')
    how = cal if mode == 'analytic' else _planted_table()
    kw = dict(cal=cal.block()) if mode == 'analytic' else dict(table=how.table())
    want, want_in = R.rectify_ref(frames, how)
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 2, 1)):
        got, got_in = _rectify(frames, hr, wr, offs=offs, **kw)
        assert torch.equal(got, want) and torch.equal(got_in, want_in), offs


# ---------------------------------------------------------- um_valid_and --
def _valid_and(valid, inside, off=0):
    from umamd import _lib as L
    n, hw = valid.shape[0], inside.numel()
    v = Buf(valid.numel(), off, valid.to(DEV))
    i = Buf(hw, off, inside.to(DEV))
    L.call('um_valid_and', L.ptr(v.view), L.ptr(i.view), n, hw)
    torch.cuda.synchronize()
    assert v.around_untouched() and i.around_untouched()
    assert torch.equal(i.view.cpu(), inside.reshape(-1))
    return v.view.cpu().view(valid.shape)


@pytest.mark.parametrize('shape', [(2, 41, 51), (1, 3, 5), (3, 8, 16)])
def test_valid_and(shape):
    """bytes other than 0 / 1 on both sides count as set and come out as 1; an
    odd image size (2091) makes the second image's dwords straddle the mask"""
    g = torch.Generator().manual_seed(shape[1])
    valid = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    valid[torch.rand(shape, generator=g) < 0.4] = 0
    inside = torch.randint(0, 256, shape[1:], generator=g, dtype=torch.uint8)
    inside[torch.rand(shape[1:], generator=g) < 0.4] = 0
    want = ((valid != 0) & (inside != 0)[None]).to(torch.uint8)
    assert 0.2 < float(want.float().mean()) < 0.5
    for off in (0, 1, 2):
        assert torch.equal(_valid_and(valid, inside, off), want), off


# -------------------------------------------------------- argument errors --
def test_argument_errors():
    """each returns UM_ERR_ARG (1) and writes nothing"""
    from umamd import _lib as L
    lib = L.lib()
    frames = R.frames(1, 5, 7, seed=1).to(DEV)
    cal = torch.from_numpy(R.calibration('small').block()).to(DEV)
    cal_off = torch.zeros(28, device=DEV)
    table = torch.zeros((3, 5, 2), dtype=torch.int32, device=DEV)
    dst, ins = Buf(3 * 5 * 3), Buf(3 * 5)
    s, d, i, c, t = (L.ptr(x) for x in (frames, dst.view, ins.view, cal, table))
    ok = dict(src=s, N=1, Hs=5, Ws=7, Hr=3, Wr=5, cal=c, map=None, dst=d, inside=i)
    bad = [dict(N=0), dict(Hs=1), dict(Ws=1), dict(Hr=1), dict(Wr=1), dict(Hs=32768),
           dict(Ws=32768), dict(N=2 ** 31 - 1), dict(Hr=32768, Wr=32768, N=2),
           dict(map=t), dict(cal=None), dict(src=None), dict(dst=None),
           dict(cal=cal_off.data_ptr() + 2), dict(cal=None, map=t + 1), dict(cal=None, map=t + 2)]
    for kw in bad:
        a = {**ok, **kw}
        rc = lib.um_frame_rectify(a['src'], a['N'], a['Hs'], a['Ws'], a['Hr'], a['Wr'], a['cal'],
                                  a['map'], a['dst'], a['inside'], L.stream())
        assert rc == 1, kw
        assert b'um_frame_rectify' in lib.um_last_error(), kw
    v = Buf(15)
    for args in ((None, i, 1, 15), (L.ptr(v.view), None, 1, 15), (L.ptr(v.view), i, 0, 15),
                 (L.ptr(v.view), i, 1, 0), (L.ptr(v.view), i, -1, 15)):
        assert lib.um_valid_and(*args, L.stream()) == 1, args
    torch.cuda.synchronize()
    for b in (dst, ins, v):
        assert bool((b.whole == SENT).all())
    with pytest.raises(L.UmamdError, match='exactly one of cal and map'):
        L.call('um_frame_rectify', s, 1, 5, 7, 3, 5, c, t, d, i)


# ------------------------------------------------------- umamd.rectify --
def test_rectify_module_on_device_tensors():
    from umamd.rectify import rectify
    cal, frames, (hr, wr) = _case('blocks', 'rational')
    for how in (cal, _planted_table()):
        want, want_in = R.rectify_ref(frames, how)
        out, inside = rectify(frames.to(DEV), how)
        assert out.dtype == torch.uint8 and out.shape == (2, hr, wr, 3) and out.is_cuda
        assert inside.dtype == torch.uint8 and inside.shape == (hr, wr)
        assert torch.equal(out.cpu(), want) and torch.equal(inside.cpu(), want_in)
        o = torch.full((2, hr, wr, 3), SENT, dtype=torch.uint8, device=DEV)
        m = torch.full((hr, wr), SENT, dtype=torch.uint8, device=DEV)
        o2, m2 = rectify(frames.to(DEV), how, out=o, inside=m)
        assert o2 is o and m2 is m
        assert torch.equal(o.cpu(), want) and torch.equal(m.cpu(), want_in)
    from umamd._lib import UmamdError
    with pytest.raises(UmamdError, match='frames on'):
        rectify(frames.to(DEV), cal, out=torch.zeros(2, hr, wr, 3, dtype=torch.uint8))


# ---------------------------------------------------------- DepthPipeline --
import test_gpu_deploy as TD  # noqa: E402  (its small model)

# raw 96x160 -> rectified 64x128 -> the model at 64x128: the smallest size that model runs at (at
# 32x64 its deepest level is one row high and um_conv2d_fwd refuses the reflect pad)
B, RAW, RECT, MODEL = 2, (96, 160), (64, 128), (64, 128)
CAM = dict(K=(150.5, 149.0, 81.3, 47.2), dist=(-0.28, 0.09, 0.001, -0.0008, -0.01),
           R=R.rot(0.01, -0.02, 0.015), P=(95.0, 95.0, 64.0, 32.0), size=RECT, baseline=4.0)
CAM2 = {**CAM, 'K': (148.0, 151.0, 78.5, 49.0), 'dist': (-0.2, 0.05, -0.001, 0.0005, 0.0),
        'R': R.rot(-0.01, 0.015, -0.02)}
PLAIN_KEYS = ['depth', 'disparity', 'lr_error', 'prediction', 'uncertainty', 'valid']
EXTRA = dict(render='depth', render_range=(0.5, 40.0), opacity=0.6, invalid_opacity=0.1,
             points='both')
EXTRA_KEYS = ['cloud_offsets', 'cloud_rgba', 'cloud_xyzu', 'render', 'xyz']


def _cam(kw=CAM):
    from umamd.rectify import Calibration
    return Calibration(**kw)


def _pipe(model, rectify=None, **kw):
    from umamd.deploy import DepthPipeline
    hs, ws = RAW if rectify is not None else RECT
    return DepthPipeline(model, hs, ws, batch=B, height=MODEL[0], width=MODEL[1], scale=0.3,
                         rectify=rectify, **kw)


@pytest.fixture(scope='module')
def model():
    return TD._model()


@pytest.fixture(scope='module')
def raw_frames():
    return R.frames(B, *RAW, seed=21)


def _plain(model, frames, cam, **kw):
    """what a pipeline without the stage computes for the reference's
    rectified frames, at gates inside its outputs' range -> (gates, outputs,
    rectified, inside)"""
    rect, inside = R.rectify_ref(frames, cam)
    assert 0.5 < float(inside.float().mean()) < 0.99
    pipe = _pipe(model, focal_baseline=cam.focal_baseline, intrinsics=cam.intrinsics, **kw)
    gates = TD._quartiles(pipe(rect))
    pipe.set_params(**gates)
    out = TD._clone(pipe(rect))
    assert 0.2 < float(out['valid'].float().mean()) < 0.8
    return gates, out, rect, inside


def _check_against_plain(out, base, rect, inside):
    assert sorted(out) == sorted(list(base) + ['frame', 'inside'])
    assert out['frame'].dtype == torch.uint8 and out['inside'].dtype == torch.bool
    assert torch.equal(out['frame'].cpu(), rect)
    assert torch.equal(out['inside'].cpu(), inside.bool())
    both = base['valid'] & inside.bool().to(DEV)[None]
    assert int(both.sum()) < int(base['valid'].sum())
    assert torch.equal(out['valid'], both)
    for k in ('disparity', 'depth', 'uncertainty', 'lr_error', 'prediction'):
        assert torch.equal(out[k], base[k]), k


def test_pipeline_rectify(model, raw_frames):
    cam = _cam()
    gates, base, rect, inside = _plain(model, raw_frames, cam)
    assert sorted(base) == PLAIN_KEYS  # rectify=None: exactly today's keys
    kw = dict(focal_baseline=cam.focal_baseline, **gates)
    pipe = _pipe(model, rectify=cam, **kw)
    assert pipe._graph is not None and pipe.src_shape == (B,) + RAW + (3,)
    out = TD._clone(pipe(raw_frames))
    for k in ('disparity', 'depth', 'uncertainty', 'lr_error', 'valid'):
        assert out[k].shape == (B,) + RECT, k
    _check_against_plain(out, base, rect, inside)
    for f in (raw_frames.to(DEV), raw_frames.pin_memory()):  # device and pinned host frames
        _check_against_plain(TD._clone(pipe(f)), base, rect, inside)
    eager = _pipe(model, rectify=cam, capture=False, **kw)
    assert eager._graph is None
    _check_against_plain(TD._clone(eager(raw_frames)), base, rect, inside)
    _check_against_plain(TD._clone(eager(raw_frames.to(DEV))), base, rect, inside)
    with pytest.raises(ValueError, match='built for frames'):
        pipe(rect)  # the rectified size is not what the call takes


@pytest.mark.parametrize('capture', [True, False])
def test_pipeline_rectify_with_render_and_points(model, raw_frames, capture):
    """the display and the point stage read the rectified frame and the
    combined mask: what a plain pipeline renders and packs for the reference's
    frame when its mask is the combined one"""
    import _points_ref as PR
    from umamd import render as UR
    cam = _cam()
    gates, base, rect, inside = _plain(model, raw_frames, cam)
    pipe = _pipe(model, rectify=cam, capture=capture, focal_baseline=cam.focal_baseline,
                 intrinsics=cam.intrinsics, **EXTRA, **gates)
    out = TD._clone(pipe(raw_frames))
    assert sorted(out) == sorted(PLAIN_KEYS + EXTRA_KEYS + ['frame', 'inside'])
    _check_against_plain({k: v for k, v in out.items() if k not in EXTRA_KEYS}, base, rect, inside)
    valid = out['valid']
    assert torch.equal(out['xyz'].cpu(), PR.backproject_ref(out['depth'], cam.intrinsics, valid))
    want = PR.cloud_ref(out['depth'], cam.intrinsics, valid, out['uncertainty'], rect, 1)
    k = int(want[2][-1])
    assert k == int(valid.sum()) > 0
    assert torch.equal(out['cloud_offsets'].cpu(), want[2])
    assert torch.equal(out['cloud_xyzu'][:k].cpu(), want[0])
    assert torch.equal(out['cloud_rgba'][:k].cpu(), want[1])  # colours of the rectified frame
    shown = UR.colourise(out['depth'], 0.5, 40.0, valid=valid, frame=rect.to(DEV), opacity=0.6,
                         invalid_opacity=0.1)
    assert torch.equal(out['render'], shown)
    assert not torch.equal(out['render'].cpu(), rect)


@pytest.mark.parametrize('mode', ['analytic', 'table'])
def test_set_calibration_without_recapture(model, raw_frames, mode):
    from umamd.rectify import RemapTable

    def how(kw):
        cam = _cam(kw)
        if mode == 'analytic':
            return cam
        mx, my = R.coords_ref(cam.block(), *RECT, np.float32)
        return RemapTable(mx, my)
    a, b = how(CAM), how(CAM2)
    pipe = _pipe(model, rectify=a)
    g = pipe._graph
    first = TD._clone(pipe(raw_frames))
    ra, ia = R.rectify_ref(raw_frames, a)
    assert torch.equal(first['frame'].cpu(), ra) and torch.equal(first['inside'].cpu(), ia.bool())
    pipe.set_calibration(b)
    second = TD._clone(pipe(raw_frames))
    assert pipe._graph is g and g is not None
    rb, ib = R.rectify_ref(raw_frames, b)
    assert not torch.equal(ra, rb) and not torch.equal(ia, ib)
    assert torch.equal(second['frame'].cpu(), rb) and torch.equal(second['inside'].cpu(), ib.bool())
    fresh = _pipe(model, rectify=b)(raw_frames)
    for k in second:
        assert torch.equal(second[k], fresh[k]), k
    other = _cam({**CAM, 'size': (64, 96)}) if mode == 'analytic' else \
        RemapTable(np.zeros((64, 96), np.float32), np.zeros((64, 96), np.float32))
    with pytest.raises(ValueError, match='rectified size'):
        pipe.set_calibration(other)
    with pytest.raises(ValueError, match='build another pipeline'):
        pipe.set_calibration(_cam() if mode == 'table' else RemapTable(
            np.zeros(RECT, np.float32), np.zeros(RECT, np.float32)))
    with pytest.raises(TypeError, match='Calibration or a RemapTable'):
        pipe.set_calibration(a.block() if mode == 'analytic' else a.table())
    third = pipe(raw_frames)  # the refused calls changed nothing
    for k in second:
        assert torch.equal(second[k], third[k]), k


def test_rectify_none_is_todays_pipeline(model):
    frames = R.frames(B, *RECT, seed=22)
    pipe = _pipe(model)
    pipe(frames)
    assert sorted(pipe.last()) == PLAIN_KEYS
    for attr in ('_raw', '_inside', '_rect'):
        assert not hasattr(pipe, attr), attr
    assert pipe._rect_stage is None  # where the stage's buffers live
    assert pipe.rectify is None and pipe.frame_shape == pipe.src_shape
    with pytest.raises(ValueError, match='rectify=None'):
        pipe.set_calibration(_cam())
