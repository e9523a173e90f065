"""The display stage on the GPU (csrc/render.hip, umamd/render.py and
DepthPipeline(render=...)): um_depth_render and um_value_range against the
f32 restatement of their definition in tests/_render_ref.py, byte for byte --
the definition is integer arithmetic after three exactly rounded f32
operations, so there is no tolerance anywhere in this file."""
import pytest
import torch

import _render_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SHAPES = {'tail': (3, 5), 'blocks': (2, 67, 129)}  # 15 (scalar tail only); 17 286 = 4 k + 2


def _lut(name='inferno'):
    from umamd.render import lut
    return lut(name)


def _frame(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, tuple(shape) + (3,), generator=g, dtype=torch.uint8)


def _valid(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < 0.6).to(torch.uint8)


def _render(value, valid, frame, table, rparams, rng, inverse):
    """um_depth_render on device copies of the host tensors -> host uint8"""
    from umamd import _lib as L
    dv = value.to(DEV)
    dm = None if valid is None else valid.to(DEV)
    df = None if frame is None else frame.to(DEV)
    dt = table.to(DEV)
    dp = torch.tensor(rparams, dtype=torch.float32, device=DEV)
    dr = None if rng is None else torch.as_tensor(rng, dtype=torch.float32).to(DEV)
    out = torch.full(tuple(value.shape) + (3,), 7, dtype=torch.uint8, device=DEV)
    L.call('um_depth_render', L.ptr(dv), L.ptr(dm), L.ptr(df), value.numel(), L.ptr(dt),
           L.ptr(dp), L.ptr(dr), int(inverse), L.ptr(out))
    torch.cuda.synchronize()
    return out.cpu()


# name: (lo, hi, opacity, invalid_opacity, valid?, frame?, inverse, range given?)
RENDER_CASES = {
    'plain': (0.0, 1.0, 1.0, 0.0, False, False, False, False),
    'inverse': (0.0, 1.0, 1.0, 0.0, False, False, True, False),
    'frame_opacity1': (0.0, 1.0, 1.0, 0.0, False, True, False, False),
    'overlay': (0.0, 1.0, 0.6, 0.0, True, True, False, False),
    'overlay_invalid_quarter': (0.25, 0.75, 0.6, 0.25, True, True, True, False),
    'opacity0': (0.0, 1.0, 0.0, 0.25, True, True, False, False),
    'valid_no_frame': (0.0, 1.0, 0.6, 0.25, True, False, False, False),
    'range_given': (-5.0, -4.0, 1.0, 0.0, True, True, False, True),
    'flat_range': (0.5, 0.5, 1.0, 0.0, False, True, False, False),
    'viridis': (0.0, 1.0, 1.0, 0.0, False, False, False, False),
}


@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('case', sorted(RENDER_CASES))
def test_render_equals_reference(case, shape):
    lo, hi, op, iop, with_valid, with_frame, inverse, with_range = RENDER_CASES[case]
    shp = SHAPES[shape]
    table = _lut('viridis' if case == 'viridis' else 'inferno')
    value = R.planted(shp, seed=len(case))
    if case == 'flat_range':
        value.view(-1)[::3] = 0.5  # (v - lo) / 0: NaN at v == lo, +-inf elsewhere
    valid = _valid(shp, 1) if with_valid else None
    frame = _frame(shp, 2) if with_frame else None
    # with a range the (lo, hi) of the block must be ignored
    rparams = (lo, hi, op, iop) if not with_range else (-5.0, -4.0, op, iop)
    rng = (0.1, 0.9) if with_range else None
    if with_range:
        lo, hi = rng
    got = _render(value, valid, frame, table, rparams, rng, inverse)
    want = R.render_ref(value, table, lo, hi, op, iop, valid, frame, inverse)
    assert got.shape == want.shape and torch.equal(got, want)
    assert bool(want.any()) and not bool((want == 7).all())


def test_render_unaligned_bases():
    """value, valid, frame and rgb each one element into a larger allocation
    (4, 1, 1 and 1 bytes off): the scalar form, the same bytes"""
    from umamd import _lib as L
    shp = SHAPES['blocks']
    n = shp[0] * shp[1] * shp[2]
    value, valid, frame = R.planted(shp, seed=9), _valid(shp, 1), _frame(shp, 2)
    table = _lut()
    rparams = (0.0, 1.0, 0.6, 0.25)
    want = _render(value, valid, frame, table, rparams, None, False)
    assert torch.equal(want, R.render_ref(value, table, 0.0, 1.0, 0.6, 0.25, valid, frame))
    bv = torch.zeros(n + 1, device=DEV)
    bm = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
    bf = torch.zeros(3 * n + 1, dtype=torch.uint8, device=DEV)
    bo = torch.zeros(3 * n + 2, dtype=torch.uint8, device=DEV)
    bv[1:].copy_(value.view(-1))
    bm[1:].copy_(valid.view(-1))
    bf[1:].copy_(frame.view(-1))
    dt, dp = table.to(DEV), torch.tensor(rparams, device=DEV)
    for which in ('all', 'value', 'valid', 'frame', 'rgb'):
        bo.zero_()
        pv = bv[1:] if which in ('all', 'value') else bv[1:].clone()
        pm = bm[1:] if which in ('all', 'valid') else bm[1:].clone()
        pf = bf[1:] if which in ('all', 'frame') else bf[1:].clone()
        po = bo[1:3 * n + 1] if which in ('all', 'rgb') else bo[:3 * n]
        if which != 'all':
            off = {'value': pv, 'valid': pm, 'frame': pf, 'rgb': po}[which]
            assert off.data_ptr() % 4 != 0 or which == 'value' and off.data_ptr() % 16 != 0
        L.call('um_depth_render', L.ptr(pv), L.ptr(pm), L.ptr(pf), n, L.ptr(dt), L.ptr(dp),
               None, 0, L.ptr(po))
        torch.cuda.synchronize()
        assert torch.equal(po.cpu().view(want.shape), want), which
        rest = torch.cat([bo[:1], bo[3 * n + 1:]]) if which in ('all', 'rgb') else bo[3 * n:]
        assert not bool(rest.any()), which  # nothing written around the picture


# ---------------------------------------------------------- um_value_range --
def _range(value, valid):
    from umamd.render import value_range
    dv = value.to(DEV).contiguous()
    dm = None if valid is None else valid.to(DEV)
    return value_range(dv, dm)


@pytest.mark.parametrize('count', [1, 15, 17286, 480 * 640])
def test_value_range_equals_masked_min_max(count):
    g = torch.Generator().manual_seed(count)
    value = torch.randn(count, generator=g) * 30
    valid = _valid((count,), 3)
    valid[count // 2] = 1
    for v, m in ((value, None), (value, valid)):
        got = _range(v, m)
        again = _range(v, m)
        assert torch.equal(got.cpu(), R.value_range_ref(v, m)), (count, m is None)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))  # identical bits
    # NaNs take no part, also where they are valid; the extremes at the ends
    # of the map (the scalar tail) and behind an invalid pixel
    nan = value.clone()
    nan[torch.rand(count, generator=g) < 0.3] = float('nan')
    nan[count // 2] = 1.0
    for m in (None, valid):
        assert torch.equal(_range(nan, m).cpu(), R.value_range_ref(nan, m))
    if count > 2:
        ends = value.clone()
        ends[-1], ends[0], ends[1] = 1e6, -1e6, float('-inf')
        m = valid.clone()
        m[-1], m[0], m[1] = 1, 1, 0
        assert _range(ends, m).tolist() == [-1e6, 1e6]
        assert _range(ends, None).tolist() == [float('-inf'), 1e6]


def test_value_range_unaligned_and_nothing_valid():
    n = 17286
    value = R.planted((n,), seed=6)
    buf = torch.zeros(n + 1, device=DEV)
    buf[1:].copy_(value)
    mb = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
    valid = _valid((n,), 3)
    mb[1:].copy_(valid)
    from umamd.render import colourise, value_range
    assert torch.equal(value_range(buf[1:], mb[1:]).cpu(), R.value_range_ref(value, valid))
    # no valid pixel, and no pixel that is a number: (+inf, -inf), a black picture
    none = torch.zeros(n, dtype=torch.uint8, device=DEV)
    r = value_range(value.to(DEV), none)
    assert r.tolist() == [float('inf'), float('-inf')]
    assert value_range(torch.full((n,), float('nan'), device=DEV)).tolist() == \
        [float('inf'), float('-inf')]
    frame = _frame((n,), 2).to(DEV)
    pic = colourise(value.to(DEV), valid=none, frame=frame)  # auto range, all background
    assert torch.equal(pic, frame)
    assert not bool(colourise(value.to(DEV), valid=none, invalid_opacity=1.0).any())


def test_value_range_in_a_replayed_graph():
    """captured once, replayed with other inputs: no state from the last run"""
    from umamd import _lib as L
    n = 480 * 640
    g = torch.Generator().manual_seed(8)
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g) * 0.01 + 3  # inside a's range on neither side
    value = torch.zeros(n, device=DEV)
    valid = torch.ones(n, dtype=torch.uint8, device=DEV)
    out = torch.zeros(2, device=DEV)
    ws = torch.zeros(L.query('um_value_range_ws', n), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.call('um_value_range', L.ptr(value), L.ptr(valid), n, L.ptr(out), L.ptr(ws))
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.call('um_value_range', L.ptr(value), L.ptr(valid), n, L.ptr(out), L.ptr(ws))
    torch.cuda.current_stream().wait_stream(side)
    for src in (a, b, a):
        value.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), R.value_range_ref(src)), out


def test_argument_errors():
    from umamd import _lib as L
    v = torch.zeros(16, device=DEV)
    t = torch.zeros(256, 3, dtype=torch.uint8, device=DEV)
    p = torch.zeros(4, device=DEV)
    o = torch.zeros(16, 3, dtype=torch.uint8, device=DEV)
    r = torch.zeros(2, device=DEV)
    ws = torch.zeros(8, dtype=torch.uint8, device=DEV)

    def render(value=v, count=16, lut=t, rparams=p, rgb=o):
        L.call('um_depth_render', L.ptr(value), None, None, count, L.ptr(lut), L.ptr(rparams),
               None, 0, L.ptr(rgb))
    render()
    for kw in (dict(count=0), dict(count=-4)):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_render: count'):
            render(**kw)
    for k in ('value', 'lut', 'rparams', 'rgb'):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_render: null pointer'):
            render(**{k: None})
    with pytest.raises(L.UmamdError, match=r'\(1\).*um_depth_render: .*pixels'):
        render(count=1024 * (2 ** 31))  # 2^31 workgroups: refused before any launch
    L.call('um_value_range', L.ptr(v), None, 16, L.ptr(r), L.ptr(ws))
    for count in (0, -1):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_value_range: count'):
            L.call('um_value_range', L.ptr(v), None, count, L.ptr(r), L.ptr(ws))
    for args in ((None, None, 16, L.ptr(r), L.ptr(ws)), (L.ptr(v), None, 16, None, L.ptr(ws)),
                 (L.ptr(v), None, 16, L.ptr(r), None)):
        with pytest.raises(L.UmamdError, match=r'\(1\).*um_value_range: null pointer'):
            L.call('um_value_range', *args)
    torch.cuda.synchronize()


# ---------------------------------------------------------- DepthPipeline --
import test_gpu_deploy as TD  # noqa: E402  (its 64x128 model and 150x262 frames)

FIXED = dict(render='depth', render_range=(0.0, 40.0), opacity=0.6)


@pytest.fixture(scope='module')
def model():
    return TD._model()


@pytest.fixture(scope='module')
def frames():
    return TD._frames(TD.B, TD.HS, TD.WS, seed=11)


@pytest.fixture(scope='module')
def plain(model, frames):
    """a render=None pipeline's outputs at gates inside the outputs' range"""
    pipe = TD._pipe(model)
    gates = TD._quartiles(pipe(frames))
    pipe.set_params(**gates)
    out = TD._clone(pipe(frames))
    assert 'render' not in out and 0.2 < float(out['valid'].float().mean()) < 0.8
    for k in ('render_lo', 'render_hi', 'opacity', 'invalid_opacity'):
        with pytest.raises(TypeError, match='unknown'):
            pipe.set_params(**{k: 0.5})
    assert not hasattr(pipe, '_render') and not hasattr(pipe, '_rparams')
    assert pipe._render_stage is None  # where the stage's buffers live
    return gates, out


def _ref_of(out, frames, key, lo, hi, opacity, invalid_opacity=0.0, inverse=False, table=None):
    return R.render_ref(out[key], _lut() if table is None else table, lo, hi, opacity,
                        invalid_opacity, out['valid'], frames, inverse)


def test_pipeline_render_fixed_range(model, frames, plain):
    gates, base = plain
    pipe = TD._pipe(model, **gates, **FIXED)
    out = TD._clone(pipe(frames))
    pic = out.pop('render')
    assert pic.dtype == torch.uint8 and pic.shape == (TD.B, TD.HS, TD.WS, 3)
    assert sorted(out) == sorted(base)
    for k in base:  # the other outputs are a render=None pipeline's
        assert torch.equal(out[k], base[k]), k
    assert torch.equal(pic.cpu(), _ref_of(out, frames, 'depth', 0.0, 40.0, 0.6))
    invalid = ~out['valid'].cpu()
    assert torch.equal(pic.cpu()[invalid], frames[invalid])  # the camera image shows through
    assert not torch.equal(pic.cpu(), frames)
    # capture=False: the same launches eagerly
    eager = TD._pipe(model, capture=False, **gates, **FIXED)
    assert eager._graph is None and pipe._graph is not None
    assert torch.equal(eager(frames)['render'], pic)
    # the standalone call draws the same picture from the same inputs
    from umamd.render import colourise
    alone = colourise(out['depth'], 0.0, 40.0, valid=out['valid'], frame=frames.to(DEV),
                      opacity=0.6)
    assert torch.equal(alone, pic)
    buf = torch.zeros_like(pic)
    assert colourise(out['depth'], 0.0, 40.0, valid=out['valid'], frame=frames.to(DEV),
                     opacity=0.6, out=buf) is buf and torch.equal(buf, pic)


def test_pipeline_render_set_params_without_recapture(model, frames, plain):
    gates, _ = plain
    pipe = TD._pipe(model, **gates, **FIXED)
    g = pipe._graph
    a = TD._clone(pipe(frames))
    pipe.set_params(opacity=1.0, render_hi=25.0)
    b = TD._clone(pipe(frames))
    assert pipe._graph is g and pipe.render_params['render_hi'] == 25.0
    assert torch.equal(b['depth'], a['depth']) and not torch.equal(b['render'], a['render'])
    assert torch.equal(b['render'].cpu(), _ref_of(b, frames, 'depth', 0.0, 25.0, 1.0))
    pipe.set_params(render_lo=5.0, invalid_opacity=0.25, max_uncertainty=float('inf'))
    c = TD._clone(pipe(frames))
    assert pipe._graph is g and int(c['valid'].sum()) > int(b['valid'].sum())
    assert torch.equal(c['render'].cpu(), _ref_of(c, frames, 'depth', 5.0, 25.0, 1.0, 0.25))
    with pytest.raises(TypeError, match='unknown'):
        pipe.set_params(render_range=(0, 1))
    with pytest.raises(TypeError, match='number'):
        pipe.set_params(opacity='1')


def test_pipeline_render_auto_range(model, frames, plain):
    from umamd.render import colourise
    gates, base = plain
    pipe = TD._pipe(model, **gates, render='lr_error', colour_map='viridis', inverse=True,
                    invalid_opacity=0.25)
    assert pipe.render_auto
    for fr in (frames, TD._frames(TD.B, TD.HS, TD.WS, seed=12)):  # the range is per call
        out = TD._clone(pipe(fr))
        lo, hi = R.value_range_ref(out['lr_error'], out['valid'])
        assert torch.equal(pipe._render_stage._range.cpu(), torch.stack([lo, hi])) and lo < hi
        want = _ref_of(out, fr, 'lr_error', lo, hi, 1.0, 0.25, True, _lut('viridis'))
        assert torch.equal(out['render'].cpu(), want)
        alone = colourise(out['lr_error'], valid=out['valid'], frame=fr.to(DEV),
                          colour_map='viridis', inverse=True, invalid_opacity=0.25)
        assert torch.equal(alone, out['render'])
    for k in base:
        assert torch.equal(pipe(frames)[k], base[k]), k
    eager = TD._pipe(model, capture=False, **gates, render='lr_error', colour_map='viridis',
                     inverse=True, invalid_opacity=0.25)
    assert torch.equal(eager(frames)['render'], pipe(frames)['render'])
    with pytest.raises(ValueError, match="'auto'"):
        pipe.set_params(render_hi=1.0)
    with pytest.raises(ValueError, match="'auto'"):
        pipe.set_params(render_lo=0.0, opacity=0.5)
    pipe.set_params(opacity=0.5)
    out = TD._clone(pipe(frames))
    lo, hi = R.value_range_ref(out['lr_error'], out['valid'])
    assert torch.equal(out['render'].cpu(),
                       _ref_of(out, frames, 'lr_error', lo, hi, 0.5, 0.25, True, _lut('viridis')))


def test_pipeline_render_uncertainty_bf16(frames):
    pipe = TD._pipe(TD._model('bf16'), render='uncertainty', render_range=(0.0, 0.3),
                    colour_map=_lut('viridis'), opacity=0.6)
    out = TD._clone(pipe(frames))
    pipe.set_params(**TD._quartiles(out))
    out = TD._clone(pipe(frames))
    assert 0.2 < float(out['valid'].float().mean()) < 0.8
    want = _ref_of(out, frames, 'uncertainty', 0.0, 0.3, 0.6, table=_lut('viridis'))
    assert torch.equal(out['render'].cpu(), want)
