"""The point stage on the GPU (csrc/points.hip, umamd/points.py and
DepthPipeline(points=...)): um_depth_backproject and um_depth_cloud against the
numpy-f32 restatement of their definition in tests/_points_ref.py, bit for bit
-- every step of the definition is one exactly rounded f32 operation and the
order of the cloud is fixed, so there is no tolerance and no left-out pixel
anywhere in this file.  Outputs are pre-filled with a sentinel: what a call
must not write still holds it."""
import pytest
import torch

import _points_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SENT = -777.0  # float outputs
SENT_U8 = 7
SENT_I32 = -5
TILE = 1024  # lattice sites of a tile, SCAN the scan workgroup (include/umamd.h)
SCAN = 256
INT_MAX = 2 ** 31 - 1

SHAPES = {'tail': (1, 3, 5), 'blocks': (2, 67, 129)}  # 15 (scalar tail only); 17 286 = 4 k + 2


def _dev(t):
    return None if t is None else t.to(DEV)


def _intr(intr=R.INTR):
    return torch.tensor(intr, dtype=torch.float32, device=DEV)


# --------------------------------------------------- um_depth_backproject --
def _map(depth, valid, intr=R.INTR):
    from umamd import _lib as L
    n, h, w = depth.shape
    dd, dv, di = _dev(depth), _dev(valid), _intr(intr)
    out = torch.full((n, h, w, 3), SENT, device=DEV)
    L.call('um_depth_backproject', L.ptr(dd), L.ptr(dv), n, h, w, L.ptr(di), L.ptr(out))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('with_valid', [True, False])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_map_equals_reference(shape, with_valid):
    depth, valid, _, _ = R.planted(SHAPES[shape], seed=3)
    if not with_valid:  # every pixel is kept: no special values to hide
        depth, valid = depth.nan_to_num(1.5, 2.5, 3.5).abs(), None
    got = _map(depth, valid)
    assert torch.equal(got, R.backproject_ref(depth, R.INTR, valid))
    assert bool(torch.isfinite(got).all()) and not bool((got == SENT).any())
    if with_valid:
        hidden = ~torch.isfinite(depth)
        assert bool(hidden.any()) and not bool(got[valid == 0].any())  # exactly 0 over NaN / inf
        assert bool((got[valid != 0][:, 2] > 0).all())


def test_map_valid_bytes_other_than_one():
    depth, valid, _, _ = R.planted(SHAPES['blocks'], seed=4)
    valid = valid * torch.tensor([1, 2, 255, 128], dtype=torch.uint8).repeat(17286 // 4 + 1)[
        :17286].view(valid.shape)
    assert torch.equal(_map(depth, valid), R.backproject_ref(depth, R.INTR, valid))


def test_map_unaligned_bases():
    """depth, valid and xyz each one element into a larger allocation (4, 1
    and 4 bytes off): the scalar form, the same bytes, nothing around them"""
    from umamd import _lib as L
    n, h, w = SHAPES['blocks']
    cnt = n * h * w
    depth, valid, _, _ = R.planted((n, h, w), seed=5)
    want = _map(depth, valid)
    assert torch.equal(want, R.backproject_ref(depth, R.INTR, valid))
    bd = torch.zeros(cnt + 1, device=DEV)
    bm = torch.zeros(cnt + 1, dtype=torch.uint8, device=DEV)
    bo = torch.zeros(3 * cnt + 2, device=DEV)
    bd[1:].copy_(depth.view(-1))
    bm[1:].copy_(valid.view(-1))
    di = _intr()
    for which in ('all', 'depth', 'valid', 'xyz'):
        bo.fill_(SENT)
        pd = bd[1:] if which in ('all', 'depth') else bd[1:].clone()
        pm = bm[1:] if which in ('all', 'valid') else bm[1:].clone()
        po = bo[1:3 * cnt + 1] if which in ('all', 'xyz') else bo[:3 * cnt]
        if which != 'all':
            off = {'depth': pd, 'valid': pm, 'xyz': po}[which]
            assert off.data_ptr() % (4 if which == 'valid' else 16) != 0
        L.call('um_depth_backproject', L.ptr(pd), L.ptr(pm), n, h, w, L.ptr(di), L.ptr(po))
        torch.cuda.synchronize()
        assert torch.equal(po.cpu().view(want.shape), want), which
        rest = torch.cat([bo[:1], bo[3 * cnt + 1:]]) if which in ('all', 'xyz') else bo[3 * cnt:]
        assert bool((rest == SENT).all()), which


# ---------------------------------------------------------- um_depth_cloud --
def _cloud(depth, valid=None, unc=None, frame=None, stride=1, intr=R.INTR, colours=True):
    """um_depth_cloud on device copies -> (xyzu, rgba, offsets) WHOLE buffers
    on the host, sentinel where nothing was written"""
    from umamd import _lib as L
    n, h, w = depth.shape
    cap = n * -(-h // stride) * -(-w // stride)
    dd, dv, du, df, di = _dev(depth), _dev(valid), _dev(unc), _dev(frame), _intr(intr)
    nbytes = L.query('um_depth_cloud_ws', n, h, w, stride)
    assert nbytes == 4 * n * -(-(cap // n) // TILE)
    ws = torch.full((nbytes + 8,), SENT_U8, dtype=torch.uint8, device=DEV)
    xyzu = torch.full((cap + 1, 4), SENT, device=DEV)
    rgba = torch.full((cap + 1, 4), SENT_U8, dtype=torch.uint8, device=DEV) if colours else None
    offs = torch.full((n + 2,), SENT_I32, dtype=torch.int32, device=DEV)
    L.call('um_depth_cloud', L.ptr(dd), L.ptr(dv), L.ptr(du), L.ptr(df), n, h, w, stride,
           L.ptr(di), L.ptr(ws), L.ptr(xyzu), L.ptr(rgba), L.ptr(offs))
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == SENT_U8).all())  # nothing beyond the queried workspace
    assert int(offs[n + 1]) == SENT_I32
    return xyzu.cpu(), None if rgba is None else rgba.cpu(), offs[:n + 1].cpu()


def _check_cloud(got, want, written_rgba=True):
    """the rows below offsets[N] equal the reference, every row from there on
    (the spare one included) still holds the sentinel"""
    xyzu, rgba, offs = got
    wx, wr, wo = want
    assert torch.equal(offs, wo), (offs, wo)
    k = int(wo[-1])
    assert len(wx) == k
    assert torch.equal(xyzu[:k], wx)
    assert bool((xyzu[k:] == SENT).all())
    if rgba is not None:
        if written_rgba:
            assert torch.equal(rgba[:k], wr)
            assert bool((rgba[k:] == SENT_U8).all())
        else:
            assert bool((rgba == SENT_U8).all())
    return k


@pytest.mark.parametrize('shape', [(1, 3, 5), (3, 33, 67)])
def test_cloud_order_and_offsets(shape):
    """less than one tile; three tiles an image with a ragged last one (2211
    sites), so image 1 and 2 start inside the scan"""
    depth, valid, unc, frame = R.planted(shape, seed=6)
    k = _check_cloud(_cloud(depth, valid, unc, frame), R.cloud_ref(depth, R.INTR, valid, unc, frame))
    assert 0 < k < depth.numel()


def test_cloud_more_tiles_than_four_scan_turns():
    """1027 tiles of 1024 sites for a scan workgroup of 256 threads: the scan
    loop runs five turns, the last one ragged"""
    from umamd import _lib as L
    shape = (1, 1030, 1021)
    tiles = -(-1030 * 1021 // TILE)
    assert tiles > 4 * SCAN and L.query('um_depth_cloud_ws', *shape, 1) == 4 * tiles
    g = torch.Generator().manual_seed(7)
    depth = torch.rand(shape, generator=g) * 49.5 + 0.5
    valid = (torch.rand(shape, generator=g) < 0.6).to(torch.uint8)
    depth[valid == 0] = float('nan')
    got = _cloud(depth, valid, None, None, colours=False)
    _check_cloud(got, R.cloud_ref(depth, R.INTR, valid))
    # several images, every one of them more than a scan turn of tiles
    shape = (3, 530, 1021)
    assert 529 * 3 > 4 * SCAN and L.query('um_depth_cloud_ws', *shape, 1) == 4 * 3 * 529
    depth = torch.rand(shape, generator=g) * 49.5 + 0.5
    valid = (torch.rand(shape, generator=g) < 0.3).to(torch.uint8)
    valid[1] = 0
    _check_cloud(_cloud(depth, valid, None, None, colours=False), R.cloud_ref(depth, R.INTR, valid))


def _pattern(name, shape):
    n, h, w = shape
    sites = h * w
    flat = torch.zeros(n, sites, dtype=torch.uint8)
    s = torch.arange(sites)
    if name == 'all':
        flat[:] = 1
    elif name == 'none':
        pass
    elif name == 'middle_image_empty':
        flat[:] = (torch.rand(n, sites, generator=torch.Generator().manual_seed(8)) < 0.6)
        flat[1] = 0
    elif name == 'last_site_of_a_tile':
        flat[:, s % TILE == TILE - 1] = 1
        flat[:, -1] = 1  # and of the ragged tile
    elif name == 'first_lane_of_each_wave':  # a thread has 4 sites: a wave 256
        flat[:, s % 256 == 0] = 1
    elif name == 'empty_wave_between_full':
        flat[:, (s // 256) % 3 != 1] = 1
    elif name == 'random60':
        flat[:] = (torch.rand(n, sites, generator=torch.Generator().manual_seed(9)) < 0.6)
    elif name == 'bytes_2_255':
        keep = torch.rand(n, sites, generator=torch.Generator().manual_seed(10)) < 0.6
        flat[:] = keep * torch.tensor([2, 255, 1, 128], dtype=torch.uint8).repeat(sites)[:sites]
    else:
        raise KeyError(name)
    return flat.view(shape)


PATTERNS = ('all', 'none', 'middle_image_empty', 'last_site_of_a_tile',
            'first_lane_of_each_wave', 'empty_wave_between_full', 'random60', 'bytes_2_255')


@pytest.mark.parametrize('pattern', PATTERNS)
def test_cloud_valid_patterns(pattern):
    shape = (3, 33, 67)
    depth, _, unc, frame = R.planted(shape, seed=11, keep=2.0)  # clean depths
    valid = _pattern(pattern, shape)
    depth[valid == 0] = float('nan')
    got = _cloud(depth, valid, unc, frame)
    k = _check_cloud(got, R.cloud_ref(depth, R.INTR, valid, unc, frame))
    if pattern == 'all':
        assert k == depth.numel()  # the capacity
    elif pattern == 'none':
        assert got[2].tolist() == [0, 0, 0, 0] and k == 0
    elif pattern == 'middle_image_empty':
        assert got[2][1] == got[2][2] and 0 < got[2][1] < got[2][3]
    elif pattern == 'last_site_of_a_tile':
        assert k == 3 * 3
    elif pattern == 'first_lane_of_each_wave':
        assert k == 3 * 9
    else:
        assert 0 < k < depth.numel()


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_cloud_stride(stride):
    shape = SHAPES['blocks']  # 67 x 129: a multiple of neither 2 nor 3
    depth, valid, unc, frame = R.planted(shape, seed=12)
    got = _cloud(depth, valid, unc, frame, stride)
    k = _check_cloud(got, R.cloud_ref(depth, R.INTR, valid, unc, frame, stride))
    assert len(got[0]) == 2 * -(-67 // stride) * -(-129 // stride) + 1 and k > 0


@pytest.mark.parametrize('stride', [1, 2])
def test_cloud_optional_inputs(stride):
    shape = SHAPES['blocks']
    depth, valid, unc, frame = R.planted(shape, seed=13)
    clean = depth.nan_to_num(1.5, 2.5, 3.5).abs()
    # no uncertainty: the fourth value is exactly 0
    got = _cloud(depth, valid, None, frame, stride)
    k = _check_cloud(got, R.cloud_ref(depth, R.INTR, valid, None, frame, stride))
    assert not bool(got[0][:k, 3].any())
    # no frame / no rgba / neither: no colour is written
    for f, colours in ((None, True), (frame, False), (None, False)):
        got = _cloud(depth, valid, unc, f, stride, colours=colours)
        _check_cloud(got, R.cloud_ref(depth, R.INTR, valid, unc, None, stride), written_rgba=False)
    # valid=None: every site is kept
    got = _cloud(clean, None, unc, frame, stride)
    k = _check_cloud(got, R.cloud_ref(clean, R.INTR, None, unc, frame, stride))
    assert k == len(got[0]) - 1


def test_cloud_unaligned_bases():
    """depth, uncertainty, valid and frame each one element into a larger
    allocation: scalar loads, the same bytes"""
    from umamd import _lib as L
    n, h, w = SHAPES['blocks']
    cnt = n * h * w
    depth, valid, unc, frame = R.planted((n, h, w), seed=14)
    want = R.cloud_ref(depth, R.INTR, valid, unc, frame)
    k = _check_cloud(_cloud(depth, valid, unc, frame), want)
    bd = torch.zeros(cnt + 1, device=DEV)
    bu = torch.zeros(cnt + 1, device=DEV)
    bm = torch.zeros(cnt + 1, dtype=torch.uint8, device=DEV)
    bf = torch.zeros(3 * cnt + 1, dtype=torch.uint8, device=DEV)
    bd[1:].copy_(depth.view(-1))
    bu[1:].copy_(unc.view(-1))
    bm[1:].copy_(valid.view(-1))
    bf[1:].copy_(frame.view(-1))
    di = _intr()
    ws = torch.zeros(L.query('um_depth_cloud_ws', n, h, w, 1), dtype=torch.uint8, device=DEV)
    for which in ('all', 'depth', 'uncertainty', 'valid', 'frame'):
        pd = bd[1:] if which in ('all', 'depth') else bd[1:].clone()
        pu = bu[1:] if which in ('all', 'uncertainty') else bu[1:].clone()
        pm = bm[1:] if which in ('all', 'valid') else bm[1:].clone()
        pf = bf[1:] if which in ('all', 'frame') else bf[1:].clone()
        if which != 'all':
            off = {'depth': pd, 'uncertainty': pu, 'valid': pm, 'frame': pf}[which]
            assert off.data_ptr() % (16 if which in ('depth', 'uncertainty') else 4) != 0
        xyzu = torch.full((cnt, 4), SENT, device=DEV)
        rgba = torch.full((cnt, 4), SENT_U8, dtype=torch.uint8, device=DEV)
        offs = torch.full((n + 1,), SENT_I32, dtype=torch.int32, device=DEV)
        L.call('um_depth_cloud', L.ptr(pd), L.ptr(pm), L.ptr(pu), L.ptr(pf), n, h, w, 1,
               L.ptr(di), L.ptr(ws), L.ptr(xyzu), L.ptr(rgba), L.ptr(offs))
        torch.cuda.synchronize()
        _check_cloud((xyzu.cpu(), rgba.cpu(), offs.cpu()), want)


def test_cloud_in_a_replayed_graph():
    """captured once, replayed with other masks: no state from the last run"""
    from umamd import _lib as L
    n, h, w = 3, 33, 67
    depth, valid, unc, frame = R.planted((n, h, w), seed=15, keep=2.0)
    dd, du, df, di = _dev(depth), _dev(unc), _dev(frame), _intr()
    dv = torch.zeros((n, h, w), dtype=torch.uint8, device=DEV)
    ws = torch.zeros(L.query('um_depth_cloud_ws', n, h, w, 1), dtype=torch.uint8, device=DEV)
    xyzu = torch.zeros((n * h * w, 4), device=DEV)
    rgba = torch.zeros((n * h * w, 4), dtype=torch.uint8, device=DEV)
    offs = torch.zeros(n + 1, dtype=torch.int32, device=DEV)

    def run():
        L.call('um_depth_cloud', L.ptr(dd), L.ptr(dv), L.ptr(du), L.ptr(df), n, h, w, 1,
               L.ptr(di), L.ptr(ws), L.ptr(xyzu), L.ptr(rgba), L.ptr(offs))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    for name in ('random60', 'all', 'middle_image_empty', 'random60'):
        mask = _pattern(name, (n, h, w))
        dv.copy_(mask)
        xyzu.fill_(SENT)
        rgba.fill_(SENT_U8)
        graph.replay()
        torch.cuda.synchronize()
        _check_cloud((xyzu.cpu(), rgba.cpu(), offs.cpu()),
                     R.cloud_ref(depth, R.INTR, mask, unc, frame))


def test_argument_errors():
    from umamd import _lib as L
    d = torch.ones(2 * 4 * 6, device=DEV)
    i = _intr()
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    x = torch.zeros(48, 4, device=DEV)
    o = torch.zeros(3, dtype=torch.int32, device=DEV)
    m = torch.zeros(48, 3, device=DEV)

    def cloud(depth=d, n=2, h=4, w=6, stride=1, intr=i, work=ws, xyzu=x, offsets=o):
        L.call('um_depth_cloud', L.ptr(depth), None, None, None, n, h, w, stride, L.ptr(intr),
               L.ptr(work), L.ptr(xyzu), None, L.ptr(offsets))
    cloud()
    for s in (0, -1):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_cloud: stride=%d' % s):
            cloud(stride=s)
    for kw in (dict(n=0), dict(h=0), dict(w=-3)):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_cloud: N='):
            cloud(**kw)
    for k in ('depth', 'intr', 'work', 'xyzu', 'offsets'):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_cloud: null pointer'):
            cloud(**{k: None})
    # a capacity above INT_MAX: refused before any launch (nothing is that large here)
    for kw in (dict(n=2, h=32768, w=32768), dict(n=1, h=32768, w=65536),
               dict(n=INT_MAX, h=2, w=1, stride=2)):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_cloud: .*must not exceed'):
            cloud(**kw)
        assert L.query('um_depth_cloud_ws', kw['n'], kw['h'], kw['w'], kw.get('stride', 1)) == 0
    with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_cloud: .*4-byte aligned'):
        cloud(depth=d.view(torch.uint8)[1:])
    with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_cloud: xyzu must be 16-byte'):
        cloud(xyzu=x.view(-1)[1:])

    def bp(depth=d, n=2, h=4, w=6, intr=i, xyz=m):
        L.call('um_depth_backproject', L.ptr(depth), None, n, h, w, L.ptr(intr), L.ptr(xyz))
    bp()
    for kw in (dict(n=0), dict(h=-1), dict(w=0)):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_backproject: N='):
            bp(**kw)
    for k in ('depth', 'intr', 'xyz'):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_backproject: null pointer'):
            bp(**{k: None})
    with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_backproject: .*rows'):
        bp(n=65536, h=32768)
    with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_backproject: .*4-byte aligned'):
        bp(xyz=m.view(-1).view(torch.uint8)[2:])
    torch.cuda.synchronize()
    assert float(x.sum()) != 0 and bool((o.cpu() == torch.tensor([0, 24, 48])).all())


# ------------------------------------------------------------ umamd.points --
def test_points_module_on_device_tensors():
    from umamd import points as P
    shape = SHAPES['blocks']
    depth, valid, unc, frame = R.planted(shape, seed=16)
    dd, dv, du, df = _dev(depth), _dev(valid), _dev(unc), _dev(frame)
    xyz = P.backproject(dd, R.INTR, dv)
    assert xyz.shape == shape + (3,)
    assert torch.equal(xyz.cpu(), R.backproject_ref(depth, R.INTR, valid))
    assert torch.equal(P.backproject(dd, R.INTR, dv.bool()), xyz)
    one = P.backproject(dd[1], R.INTR, dv[1])  # a single [H, W] map
    assert torch.equal(one, xyz[1])
    for stride in (1, 2):
        want = R.cloud_ref(depth, R.INTR, valid, unc, frame, stride)
        xyzu, rgba, offs = P.cloud(dd, R.INTR, dv.bool(), du, df, stride)
        cap = 2 * -(-67 // stride) * -(-129 // stride)
        assert xyzu.shape == (cap, 4) and rgba.shape == (cap, 4) and offs.dtype == torch.int32
        assert torch.equal(offs.cpu(), want[2])
        k = int(offs[-1])
        assert torch.equal(xyzu[:k].cpu(), want[0]) and torch.equal(rgba[:k].cpu(), want[1])
        parts = P.split(xyzu, rgba, offs)
        assert len(parts) == 2 and sum(len(a) for a, _ in parts) == k
        o = want[2].tolist()
        for n, (a, c) in enumerate(parts):
            assert torch.equal(a.cpu(), want[0][o[n]:o[n + 1]])
            assert torch.equal(c.cpu(), want[1][o[n]:o[n + 1]])
            assert a.data_ptr() == xyzu[o[n]:].data_ptr()  # views, no copies
    xyzu, rgba, offs = P.cloud(dd, R.INTR, dv)
    assert rgba is None and not bool(xyzu[:int(offs[-1]), 3].any())
    assert [c for _, c in P.split(xyzu, rgba, offs)] == [None, None]
    assert torch.equal(xyzu[:int(offs[-1]), :3].cpu(), R.cloud_ref(depth, R.INTR, valid)[0][:, :3])


# ---------------------------------------------------------- DepthPipeline --
import test_gpu_deploy as TD  # noqa: E402  (its 64x128 model and 150x262 frames)

K = dict(intrinsics=(905.5, 903.25, 130.5, 74.75))
PLAIN_KEYS = ['depth', 'disparity', 'lr_error', 'prediction', 'uncertainty', 'valid']
CLOUD_KEYS = ['cloud_offsets', 'cloud_rgba', 'cloud_xyzu']


@pytest.fixture(scope='module')
def model():
    return TD._model()


@pytest.fixture(scope='module')
def frames():
    return TD._frames(TD.B, TD.HS, TD.WS, seed=11)


@pytest.fixture(scope='module')
def plain(model, frames):
    """a points=None pipeline's outputs at gates inside the outputs' range"""
    pipe = TD._pipe(model)
    gates = TD._quartiles(pipe(frames))
    pipe.set_params(**gates)
    out = TD._clone(pipe(frames))
    assert sorted(out) == PLAIN_KEYS and 0.2 < float(out['valid'].float().mean()) < 0.8
    for k in ('fx', 'fy', 'cx', 'cy'):
        with pytest.raises(TypeError, match='unknown'):
            pipe.set_params(**{k: 500.0})
    for attr in ('_intr', '_xyz', '_cloud_xyzu', '_cloud_rgba', '_cloud_offsets', '_cloud_ws'):
        assert not hasattr(pipe, attr), attr
    assert pipe._point_stage is None  # where the stage's buffers live
    from umamd._lib import UmamdError
    with pytest.raises(UmamdError, match='points=None'):
        pipe.cloud()
    return gates, out


def _check_pipeline_points(out, frames, intr, stride=1, map_too=True):
    """xyz and the cloud against the reference evaluated on the pipeline's own
    depth, valid, uncertainty and frames"""
    if map_too:
        assert out['xyz'].shape == (TD.B, TD.HS, TD.WS, 3)
        assert torch.equal(out['xyz'].cpu(), R.backproject_ref(out['depth'], intr, out['valid']))
    want = R.cloud_ref(out['depth'], intr, out['valid'], out['uncertainty'], frames, stride)
    k = int(want[2][-1])
    assert k == int(out['valid'][:, ::stride, ::stride].sum()) > 0
    assert torch.equal(out['cloud_offsets'].cpu(), want[2])
    assert torch.equal(out['cloud_xyzu'][:k].cpu(), want[0])
    assert torch.equal(out['cloud_rgba'][:k].cpu(), want[1])
    return k


def test_pipeline_points_both(model, frames, plain):
    gates, base = plain
    intr = K['intrinsics']
    pipe = TD._pipe(model, points='both', **K, **gates)
    out = TD._clone(pipe(frames))
    assert sorted(out) == sorted(PLAIN_KEYS + CLOUD_KEYS + ['xyz'])
    for k in base:  # the other outputs are a points=None pipeline's
        assert torch.equal(out[k], base[k]), k
    k = _check_pipeline_points(out, frames, intr)
    assert out['cloud_xyzu'].shape == (TD.B * TD.HS * TD.WS, 4)
    parts = pipe.cloud()
    assert len(parts) == TD.B and sum(len(a) for a, _ in parts) == k
    assert torch.equal(torch.cat([a for a, _ in parts]), out['cloud_xyzu'][:k])
    assert torch.equal(torch.cat([c for _, c in parts]), out['cloud_rgba'][:k])
    # capture=False: the same launches eagerly
    eager = TD._pipe(model, capture=False, points='both', **K, **gates)
    assert eager._graph is None and pipe._graph is not None
    oe = eager(frames)
    assert torch.equal(oe['xyz'], out['xyz']) and torch.equal(oe['cloud_offsets'],
                                                              out['cloud_offsets'])
    assert torch.equal(oe['cloud_xyzu'][:k], out['cloud_xyzu'][:k])
    assert torch.equal(oe['cloud_rgba'][:k], out['cloud_rgba'][:k])
    # other frames: what a fresh pipeline computes for them
    frames2 = TD._frames(TD.B, TD.HS, TD.WS, seed=12)
    o2 = TD._clone(pipe(frames2))
    k2 = _check_pipeline_points(o2, frames2, intr)
    fresh = TD._pipe(model, points='both', **K, **gates)(frames2)
    assert torch.equal(o2['xyz'], fresh['xyz'])
    assert torch.equal(o2['cloud_offsets'], fresh['cloud_offsets'])
    assert torch.equal(o2['cloud_xyzu'][:k2], fresh['cloud_xyzu'][:k2])
    assert torch.equal(o2['cloud_rgba'][:k2], fresh['cloud_rgba'][:k2])
    assert not torch.equal(o2['xyz'], out['xyz'])


def test_pipeline_points_set_params_without_recapture(model, frames, plain):
    gates, _ = plain
    fx, fy, cx, cy = K['intrinsics']
    pipe = TD._pipe(model, points='both', **K, **{**gates, 'max_uncertainty': float('inf')})
    g = pipe._graph
    a = TD._clone(pipe(frames))
    _check_pipeline_points(a, frames, (fx, fy, cx, cy))
    pipe.set_params(fx=450.25, cx=120.0)
    b = TD._clone(pipe(frames))
    assert pipe._graph is g and pipe.intrinsics == dict(fx=450.25, fy=fy, cx=120.0, cy=cy)
    _check_pipeline_points(b, frames, (450.25, fy, 120.0, cy))
    assert not torch.equal(b['xyz'][..., 0], a['xyz'][..., 0])  # X moved, Y and Z did not
    assert torch.equal(b['xyz'][..., 1:], a['xyz'][..., 1:])
    # a tighter gate: the cloud shrinks to the new mask over the lattice
    pipe.set_params(max_uncertainty=float(a['uncertainty'].median()))
    c = TD._clone(pipe(frames))
    assert pipe._graph is g
    assert int(c['cloud_offsets'][-1]) == int(c['valid'].sum()) < int(a['cloud_offsets'][-1])
    _check_pipeline_points(c, frames, (450.25, fy, 120.0, cy))
    with pytest.raises(ValueError, match='intrinsics'):
        pipe.set_params(fx=0.0)
    with pytest.raises(ValueError, match='intrinsics'):
        pipe.set_params(cy=float('nan'))
    assert pipe.intrinsics['fx'] == 450.25


def test_pipeline_points_stride2(model, frames, plain):
    gates, _ = plain
    pipe = TD._pipe(model, points='both', point_stride=2, **K, **gates)
    out = TD._clone(pipe(frames))
    assert out['cloud_xyzu'].shape == (TD.B * 75 * 131, 4)
    _check_pipeline_points(out, frames, K['intrinsics'], stride=2)


def test_pipeline_cloud_beside_render(model, frames, plain):
    gates, base = plain
    rkw = dict(render='depth', render_range=(0.0, 40.0), opacity=0.6)
    pic = TD._pipe(model, **rkw, **gates)(frames)['render'].clone()
    pipe = TD._pipe(model, points='cloud', **K, **rkw, **gates)
    out = TD._clone(pipe(frames))
    assert sorted(out) == sorted(PLAIN_KEYS + CLOUD_KEYS + ['render'])
    assert not hasattr(pipe._point_stage, '_xyz')
    assert torch.equal(out['render'], pic)
    for k in base:
        assert torch.equal(out[k], base[k]), k
    _check_pipeline_points(out, frames, K['intrinsics'], map_too=False)
    only_map = TD._pipe(model, points='map', **K, **gates)
    om = only_map(frames)
    assert sorted(om) == sorted(PLAIN_KEYS + ['xyz']) and \
        not hasattr(only_map._point_stage, '_cloud')
    assert torch.equal(om['xyz'].cpu(), R.backproject_ref(om['depth'], K['intrinsics'],
                                                          om['valid']))
