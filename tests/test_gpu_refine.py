"""The refine stage on the GPU (csrc/refine.hip, umamd/refine.py):
um_disp_smooth and um_disp_fuse against the numpy-f32 restatement of
tests/_refine_ref.py, and DepthPipeline(refine=...) end to end.  Every
comparison is bit for bit (float maps through their int32 view, so NaN payloads
count too), no tolerance and no pixel left out; outputs are pre-filled with a
sentinel."""
import pytest
import torch

import _refine_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -777.0
# (1, 3, 5): the window is larger than the image, 15 pixels (fuse: the scalar
# tail only); (2, 37, 71): ragged 64 x 16 and 64 x 8 tiles, 5254 = 4 k + 2;
# (1, 17, 130): one row and two columns past the tiles (64 x 16: 2 x 3 tiles)
SHAPES = [(1, 3, 5), (2, 37, 71), (1, 17, 130)]
WINDOWS = [(1, 1), (2, 4), (3, 5)]          # (3, 5): halo 15, the 8-row tile
EPS = 1e-4
PARAMS = (100.0, 5.0, 0.3, 1.5)             # fb, min_disp, max_unc, max_lr
FP = (EPS, 2.0, 0.25, 0.05, 9.0, 0, 0, 0)   # eps, a, floor, q, g2 = 3^2


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _f32(values):
    return torch.tensor(values, dtype=torch.float32, device=DEV)


def _tables(radius, sigma_space=1.5, sigma_colour=30.0):
    from umamd.refine import tables
    return tables(radius, sigma_space, sigma_colour)


def _smooth(disp, unc, frame, radius, step, S, G, fp=FP, off=0):
    """um_disp_smooth on device copies ``off`` elements into their allocations
    -> (disp_out, unc_out, guards): outputs pre-filled with SENT, ``guards`` the
    elements in front of and behind each output"""
    from umamd import _lib as L
    n, h, w = disp.shape
    d, u, s, g = (torch.cat([torch.zeros(off), t.flatten()]).to(DEV)[off:]
                  for t in (disp, unc, S, G))
    f = torch.cat([torch.zeros(off, dtype=torch.uint8), frame.flatten()]).to(DEV)[off:]
    outs = [torch.full((off + n * h * w + 1,), SENT, device=DEV) for _ in range(2)]
    block = _f32(fp)
    L.call('um_disp_smooth', L.ptr(d), L.ptr(u), L.ptr(f), n, h, w, radius, step, L.ptr(s),
           L.ptr(g), L.ptr(block), *[L.ptr(o[off:]) for o in outs])
    torch.cuda.synchronize()
    guards = torch.cat([torch.cat([o[:off], o[-1:]]) for o in outs])
    return outs[0][off:-1].view(n, h, w), outs[1][off:-1].view(n, h, w), guards


# --------------------------------------------------------- um_disp_smooth --
@pytest.mark.parametrize('radius,step', WINDOWS)
@pytest.mark.parametrize('shape', SHAPES)
def test_smooth_bit_exact(shape, radius, step):
    disp, unc, frame, lone = R.planted(shape, 3, radius, step)
    S, G = _tables(radius)
    want = R.smooth_ref(disp, unc, frame, radius, step, S, G, EPS)
    for (n, y, x) in lone:  # the reference passes these through
        assert R.same_bits(want[0][n, y, x], disp[n, y, x])
        assert R.same_bits(want[1][n, y, x], unc[n, y, x])
    if shape != SHAPES[0]:  # (there a pixel has few taps but itself)
        assert not R.same_bits(want[0], disp)
    got = _smooth(disp, unc, frame, radius, step, S, G)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
    assert bool((got[2] == SENT).all())


def test_smooth_unaligned_bases_and_other_tables():
    """bases 4 bytes (the frame: 1 byte) off a 16-byte boundary, and tables
    that are no Gaussians: the kernel reads what it is given"""
    shape, (radius, step) = (2, 37, 71), (2, 4)
    disp, unc, frame, _ = R.planted(shape, 5, radius, step)
    g = torch.Generator().manual_seed(9)
    S, G = torch.rand(9, generator=g), torch.rand(768, generator=g)
    want = R.smooth_ref(disp, unc, frame, radius, step, S, G, 0.03)
    fp = (0.03,) + FP[1:]
    for off in (1, 3):
        got = _smooth(disp, unc, frame, radius, step, S, G, fp, off=off)
        assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1]), off
        assert bool((got[2] == SENT).all())


def test_smooth_argument_errors_leave_the_sentinel():
    from umamd import _lib as L
    n, h, w = 2, 9, 11
    d, u = torch.ones(n * h * w + 1, device=DEV), torch.ones(n * h * w + 1, device=DEV)
    f = torch.zeros(n * h * w * 3, dtype=torch.uint8, device=DEV)
    S, G = _dev(*_tables(3))
    fp = _f32(FP)
    outs = [torch.full((n * h * w + 1,), SENT, device=DEV) for _ in range(2)]
    p = L.ptr

    def args(**kw):
        a = dict(disp=p(d), unc=p(u), frame=p(f), N=n, Hs=h, Ws=w, R=2, step=2, S=p(S), G=p(G),
                 fp=p(fp), disp_out=p(outs[0]), unc_out=p(outs[1]))
        a.update(kw)
        return list(a.values())

    L.call('um_disp_smooth', *args())  # the base case is accepted
    torch.cuda.synchronize()
    assert not bool((outs[0][:-1] == SENT).any())
    for o in outs:
        o.fill_(SENT)
    bad = [dict(R=0), dict(R=4), dict(step=0), dict(R=3, step=6), dict(R=2, step=9), dict(N=0),
           dict(Hs=0), dict(Ws=0), dict(N=2 ** 20, Hs=2 ** 6, Ws=2 ** 5)]
    bad += [{k: None} for k in ('disp', 'unc', 'frame', 'S', 'G', 'fp', 'disp_out', 'unc_out')]
    bad += [{k: v + 2} for k, v in (('disp', p(d)), ('unc', p(u)), ('S', p(S)), ('fp', p(fp)),
                                    ('disp_out', p(outs[0])), ('unc_out', p(outs[1])))]
    for kw in bad:
        with pytest.raises(L.UmamdError, match=r'um_disp_smooth failed \(1\)'):
            L.call('um_disp_smooth', *args(**kw))
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs)


def test_smooth_wrapper():
    from umamd.refine import smooth
    shape = (2, 37, 71)
    disp, unc, frame, _ = R.planted(shape, 6, 2, 3)
    want = R.smooth_ref(disp, unc, frame, 2, 3, *_tables(2, 1.2, 45.0), 1e-3)
    d, u, f = _dev(disp, unc, frame)
    got = smooth(d, u, f, radius=2, step=3, sigma_space=1.2, sigma_colour=45.0, conf_eps=1e-3)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
    assert R.same_bits(d, disp) and R.same_bits(u, unc)  # the inputs are left alone
    one = smooth(d[0], u[0], f[0], radius=2, step=3, sigma_space=1.2, sigma_colour=45.0,
                 conf_eps=1e-3)
    assert R.same_bits(one[0], want[0][0])
    for out in ((d, torch.empty_like(u)), (torch.empty_like(d), d), (u, u)):
        with pytest.raises(ValueError, match='overlaps'):
            smooth(d, u, f, out=out)


# ----------------------------------------------------------- um_disp_fuse --
FUSE_OUT = ('disparity', 'uncertainty', 'depth', 'valid', 'disp_var')


def _fuse(d, u, lr, state=None, skip=(), off=0, inplace=False, params=PARAMS, fp=FP):
    """um_disp_fuse on device copies -> dict of the outputs (None if skipped),
    ``mean`` and ``var`` (the state after the call) and ``guards``.  ``off``:
    every buffer starts that many elements into its allocation; ``inplace``:
    disparity and uncertainty are written over the inputs"""
    from umamd import _lib as L
    count = d.numel()

    def buf(t, dtype=torch.float32):
        b = torch.full((off + count + 1,), SENT if dtype == torch.float32 else 7, dtype=dtype,
                       device=DEV)
        if t is not None:
            b[off:-1] = t.flatten().to(DEV)
        return b

    ins = [buf(t) for t in (d, u, lr)]
    st = [None, None] if state is None else [buf(t) for t in state]
    out = {k: None if k in skip else buf(None, torch.uint8 if k == 'valid' else torch.float32)
           for k in FUSE_OUT}
    if inplace:
        out['disparity'], out['uncertainty'] = ins[0], ins[1]

    def p(b):
        return None if b is None else L.ptr(b[off:])
    blocks = _f32(params), _f32(fp)
    L.call('um_disp_fuse', p(ins[0]), p(ins[1]), p(ins[2]), count, L.ptr(blocks[0]),
           L.ptr(blocks[1]), p(st[0]), p(st[1]), *[p(out[k]) for k in FUSE_OUT])
    torch.cuda.synchronize()
    every = [b for b in ins + st + list(out.values()) if b is not None]
    res = {k: None if b is None else b[off:-1].view(d.shape) for k, b in out.items()}
    res['guards'] = torch.cat([torch.cat([b[:off], b[-1:]]).float() for b in every])
    if state is not None:
        res['mean'], res['var'] = (b[off:-1].view(d.shape) for b in st)
    if not inplace:  # the inputs are only read
        assert R.same_bits(ins[0][off:-1].view(d.shape), d)
    return res


def _check_fuse(got, want, state, label, skip=()):
    for k in ('disparity', 'uncertainty', 'depth'):
        if k not in skip:
            assert R.same_bits(got[k], want[k]), (label, k)
    if 'valid' not in skip:
        assert torch.equal(got['valid'].cpu(), want['valid'].to(torch.uint8)), label
    if state:
        assert R.same_bits(got['mean'], want['mean']), label
        assert R.same_bits(got['var'], want['var']), label
        if 'disp_var' not in skip:
            assert R.same_bits(got['disp_var'], want['var']), label
    elif 'disp_var' not in skip:
        assert bool((got['disp_var'] == SENT).all()), label  # never written without state
    g = got['guards']
    assert bool(((g == SENT) | (g == 7)).all()), label


@pytest.mark.parametrize('shape', SHAPES[:2])
def test_fuse_sequence_bit_exact(shape):
    """four frames against the reference, state included; every branch occurs"""
    state = R.empty_state(shape)
    seen = {'keep': 0, 'reset': 0, 'stale': 0}
    for t, (d, u, lr) in enumerate(R.sequence(shape, 11)):
        want = R.fuse_ref(d, u, lr, PARAMS, FP, state)
        got = _fuse(d, u, lr, state)
        _check_fuse(got, want, True, (shape, t))
        for k in seen:
            seen[k] += int(want[k].sum())
        if t == 0:  # an empty state behind a NaN: D = d
            assert bool(torch.isnan(want['disparity']).any())
        state = (got['mean'].cpu(), got['var'].cpu())
    assert all(seen.values()), seen


def test_fuse_without_state_reproduces_depth_post():
    """on um_depth_post's own disparity, uncertainty and lr_error the finalise
    step gives that kernel's depth and mask, and passes the two maps on"""
    import test_gpu_deploy as TD
    hs, ws = 19, 37
    gates = (TD.FB, 0.05 * ws, TD.UNC, 0.2 * ws)
    post = TD._depth_post(TD._pred(2, 8, 16), hs, ws, gates)
    assert 0 < int(post['valid'].sum()) < post['valid'].numel()
    got = _fuse(post['disparity'].cpu(), post['uncertainty'].cpu(), post['lr_error'].cpu(),
                params=gates)
    assert R.same_bits(got['depth'], post['depth'])
    assert torch.equal(got['valid'], post['valid'])
    assert R.same_bits(got['disparity'], post['disparity'])
    assert R.same_bits(got['uncertainty'], post['uncertainty'])
    assert bool((got['disp_var'] == SENT).all())


@pytest.mark.parametrize('state', [False, True])
def test_fuse_in_place_null_outputs_and_unaligned_bases(state):
    shape = (2, 37, 71)
    seq = R.sequence(shape, 12)
    st = None
    if state:  # a state that holds a frame, so every branch is taken
        first = R.fuse_ref(*seq[0], PARAMS, FP, R.empty_state(shape))
        st = (first['mean'], first['var'])
    d, u, lr = seq[1]
    want = R.fuse_ref(d, u, lr, PARAMS, FP, st)
    if state:
        assert all(bool(want[k].any()) for k in ('keep', 'reset', 'stale'))
    _check_fuse(_fuse(d, u, lr, st, inplace=True), want, state, 'in place')
    for skip in (('disparity',), ('uncertainty', 'depth'), ('valid', 'disp_var'),
                 ('disparity', 'uncertainty', 'depth', 'valid', 'disp_var')):
        got = _fuse(d, u, lr, st, skip=skip)
        assert all(got[k] is None for k in skip)
        _check_fuse(got, want, state, skip, skip=skip)
    for off in (1, 2, 3):  # 4, 8 and 12 bytes off: the scalar form
        _check_fuse(_fuse(d, u, lr, st, off=off), want, state, f'off {off}')


def test_fuse_argument_errors_leave_the_sentinel():
    from umamd import _lib as L
    n = 64
    a = {k: torch.full((n + 1,), SENT, device=DEV) for k in
         ('disp_in', 'unc_in', 'lr_error', 'mean', 'var', 'disparity', 'uncertainty', 'depth',
          'disp_var')}
    a['valid'] = torch.full((n + 1,), 7, dtype=torch.uint8, device=DEV)
    params, fp = _f32(PARAMS), _f32(FP)
    order = ('disp_in', 'unc_in', 'lr_error', 'count', 'params', 'fp', 'mean', 'var', 'disparity',
             'uncertainty', 'depth', 'valid', 'disp_var')

    def args(**kw):
        v = {k: L.ptr(t) for k, t in a.items()}
        v.update(count=n, params=L.ptr(params), fp=L.ptr(fp))
        v.update(kw)
        return [v[k] for k in order]

    bad = [dict(count=0), dict(count=-4), dict(disp_in=None), dict(unc_in=None),
           dict(params=None), dict(fp=None), dict(lr_error=None), dict(mean=None),
           dict(var=None)]
    bad += [{k: L.ptr(a[k]) + 2} for k in a if k != 'valid']
    for kw in bad:
        with pytest.raises(L.UmamdError, match=r'um_disp_fuse failed \(1\)'):
            L.call('um_disp_fuse', *args(**kw))
    torch.cuda.synchronize()
    assert all(bool((t == (7 if k == 'valid' else SENT)).all()) for k, t in a.items())
    L.call('um_disp_fuse', *args(lr_error=None, valid=None))  # no mask: lr_error is not needed
    torch.cuda.synchronize()
    assert bool((a['valid'] == 7).all()) and not bool((a['depth'][:-1] == SENT).any())


def test_fuse_wrapper():
    from umamd.refine import fuse, new_state
    shape = (2, 37, 71)
    seq = R.sequence(shape, 13, frames=3)
    kw = dict(focal_baseline=PARAMS[0], min_disparity=PARAMS[1], max_uncertainty=PARAMS[2],
              max_lr_error=PARAMS[3], noise_scale=FP[1], var_floor=FP[2], process_noise=FP[3],
              gate=3.0)
    state = new_state(seq[0][0].to(DEV))
    ref_state = R.empty_state(shape)
    for d, u, lr in seq:
        want = R.fuse_ref(d, u, lr, PARAMS, FP, ref_state)
        got = fuse(*_dev(d, u, lr), state=state, **kw)
        ref_state = (want['mean'], want['var'])
        for k in ('disparity', 'uncertainty', 'depth', 'valid'):
            assert R.same_bits(got[k], want[k]), k
        assert R.same_bits(got['disparity_var'], want['var'])
        assert R.same_bits(state[0], want['mean']) and R.same_bits(state[1], want['var'])
    plain = fuse(*_dev(d, u), **kw)  # no state, no lr_error
    want = R.fuse_ref(d, u, torch.zeros(shape), PARAMS, FP)
    assert sorted(plain) == ['depth', 'disparity', 'uncertainty', 'valid']
    assert R.same_bits(plain['depth'], want['depth']) and R.same_bits(plain['valid'], want['valid'])


# ---------------------------------------------------------- DepthPipeline --
import test_gpu_deploy as TD  # noqa: E402  (its small model and sizes)

MAPS = ('disparity', 'uncertainty', 'depth', 'valid')
# every gate open but the disparity floor (a test narrows what it needs)
NOISE = dict(noise_scale=4.0, var_floor=0.25, process_noise=0.5, gate=2.0, min_disparity=1e-3,
             max_uncertainty=float('inf'), max_lr_error=float('inf'))


@pytest.fixture(scope='module')
def model():
    return TD._model()


def _frames(k):
    return TD._frames(TD.B, TD.HS, TD.WS, seed=11 + k)


def _reference(pipe, out, frames, state):
    """the four maps (and the new state) the definition gives for one call of
    ``pipe``, from its raw maps, its lr_error and the frame it filtered along"""
    st = pipe._refine_stage
    p, q = pipe.params, pipe.refine_params
    d, u = out['raw_disparity'].cpu(), out['raw_uncertainty'].cpu()
    if st.spatial:
        d, u = R.smooth_ref(d, u, frames, st.radius, st.step,
                            *_tables(st.radius, q['sigma_space'], q['sigma_colour']),
                            q['conf_eps'])
    fp = (q['conf_eps'], q['noise_scale'], q['var_floor'], q['process_noise'], q['gate'] ** 2)
    return R.fuse_ref(d, u, out['lr_error'].cpu(),
                      [p[k] for k in ('focal_baseline', 'min_disparity', 'max_uncertainty',
                                      'max_lr_error')], fp, state if st.temporal else None)


def _check_call(pipe, out, frames, state, label):
    want = _reference(pipe, out, frames, state)
    for k in MAPS:
        assert R.same_bits(out[k], want[k]), (label, k)
    if pipe._refine_stage.temporal:
        assert R.same_bits(out['disparity_var'], want['var']), label
        return want['mean'], want['var']
    assert 'disparity_var' not in out
    return None


@pytest.mark.parametrize('mode', ['spatial', 'temporal', 'both'])
def test_pipeline_refine(model, mode):
    from umamd import _lib as L
    shape = (TD.B, TD.HS, TD.WS)
    frames = [_frames(k) for k in range(3)]
    pipe = TD._pipe(model, refine=mode, **NOISE)
    eager = TD._pipe(model, refine=mode, capture=False, **NOISE)
    assert pipe._graph is not None and eager._graph is None
    assert pipe.refine_step == 2 and pipe.refine_radius == 2 and pipe.refine == mode
    plain = TD._pipe(model)
    # three frames: the first call starts from an empty state (the warm-up run
    # of the capture left nothing behind), replay == eager == the definition
    state, first = R.empty_state(shape), None
    for t, f in enumerate(frames):
        out = TD._clone(pipe(f))
        state = _check_call(pipe, out, f, state, (mode, t))
        oe = eager(f)
        assert sorted(oe) == sorted(out)
        for k in out:
            assert R.same_bits(out[k], oe[k]), (mode, t, k)
        po = plain(f)
        assert R.same_bits(out['raw_disparity'], po['disparity'])
        assert R.same_bits(out['raw_uncertainty'], po['uncertainty'])
        assert R.same_bits(out['lr_error'], po['lr_error'])  # stays raw
        if mode != 'temporal' or t > 0:  # the first frame of a stream is its own estimate
            assert not R.same_bits(out['disparity'], po['disparity'])
        first = first or out
    if mode != 'spatial':
        assert float(out['disparity_var'].min()) >= 0
    # reset_refine() and refresh() restart the sequence
    for restart in (pipe.reset_refine, pipe.refresh):
        restart()
        again = pipe(frames[0])
        for k in first:
            assert R.same_bits(again[k], first[k]), (mode, restart.__name__, k)
        pipe(frames[1])
    # set_params: a sigma and the gate, seen by the next call without recapture
    g = pipe._graph
    pipe.reset_refine()
    before = TD._clone(pipe(frames[2]))
    pipe.reset_refine()
    pipe.set_params(sigma_colour=400.0, sigma_space=0.8)
    after = TD._clone(pipe(frames[2]))
    assert pipe._graph is g and pipe.refine_params['sigma_colour'] == 400.0
    assert R.same_bits(after['disparity'], before['disparity']) == (mode == 'temporal')
    state = _check_call(pipe, after, frames[2], R.empty_state(shape), (mode, 'sigma'))
    gate = 0.5
    if state is not None:  # a gate that half of the next frame's raw pixels would pass
        po, q = plain(frames[1]), pipe.refine_params
        m = (q['noise_scale'] * po['uncertainty'].cpu()) ** 2 + q['var_floor']
        e = po['disparity'].cpu() - state[0]
        gate = float((e * e / (state[1] + q['process_noise'] + m)).median().sqrt())
    pipe.set_params(gate=gate, max_uncertainty=float(after['uncertainty'].median()))
    out = TD._clone(pipe(frames[1]))
    assert pipe._graph is g
    want = _reference(pipe, out, frames[1], state)
    _check_call(pipe, out, frames[1], state, (mode, 'gate'))
    assert 0 < int(out['valid'].sum()) < int(after['valid'].sum())
    if mode != 'spatial':  # the gate is felt: it lets some pixels through and restarts others
        assert bool(want['keep'].any()) and bool(want['reset'].any())
    with pytest.raises(ValueError, match='gate'):
        pipe.set_params(gate=-1.0)
    with pytest.raises(TypeError, match='unknown'):
        pipe.set_params(refine_radius=1)
    # the entries of one eager call, in order
    names = ('um_depth_post', 'um_disp_smooth', 'um_disp_fuse', 'um_valid_and')
    with L.Recorder(names) as rec:
        eager(frames[0])
    torch.cuda.synchronize()
    assert [i[0] for i in rec.items] == [n for n in names[:3] if mode != 'temporal' or
                                         n != 'um_disp_smooth']


def test_pipeline_render_and_points_consume_the_refined_maps(model):
    from umamd.points import backproject
    from umamd.render import colourise
    K = (900.0, 900.0, 131.0, 75.0)
    pipe = TD._pipe(model, refine='both', render='depth', render_range=(0.0, 40.0), opacity=0.7,
                    invalid_opacity=0.2, points='map', intrinsics=K, **NOISE)
    assert pipe.params['max_uncertainty'] == float('inf')
    for k in range(2):
        f = _frames(k)
        out = pipe(f)
        assert not R.same_bits(out['disparity'], out['raw_disparity'])
        assert torch.equal(out['xyz'], backproject(out['depth'], K, out['valid']))
        assert torch.equal(out['render'], colourise(out['depth'], 0.0, 40.0, out['valid'],
                                                    f.to(DEV), opacity=0.7, invalid_opacity=0.2))
    assert float(out['xyz'].abs().max()) > 0


def test_pipeline_rectify_still_restricts_valid_to_inside(model):
    import test_gpu_rectify as TR
    cam = TR._cam()
    frames = TR.R.frames(TR.B, *TR.RAW, seed=21)
    pipe = TR._pipe(model, rectify=cam, refine='both', focal_baseline=cam.focal_baseline,
                    **NOISE)
    shape = (TR.B,) + TR.RECT
    state = R.empty_state(shape)
    for t in range(2):
        out = TD._clone(pipe(frames))
        inside = out['inside'].cpu()
        assert 0 < int(inside.sum()) < inside.numel()
        want = _reference(pipe, out, out['frame'].cpu(), state)  # filtered along the rectified frame
        state = (want['mean'], want['var'])
        for k in MAPS[:3]:
            assert R.same_bits(out[k], want[k]), (t, k)
        assert torch.equal(out['valid'].cpu(), want['valid'] & inside)
        assert int(want['valid'].sum()) > int(out['valid'].sum()) > 0


def test_pipeline_without_refine_returns_no_new_key(model):
    pipe = TD._pipe(model)
    out = pipe(_frames(0))
    assert sorted(out) == ['depth', 'disparity', 'lr_error', 'prediction', 'uncertainty', 'valid']
    assert pipe.refine is None and pipe._refine_stage is None
    with pytest.raises(TypeError, match='unknown'):
        pipe.set_params(sigma_colour=10.0)
    with pytest.raises(TypeError, match='unknown'):
        pipe.set_params(gate=2.0)
    with pytest.raises(AttributeError):
        pipe.refine_params
    pipe.reset_refine()  # nothing to do
