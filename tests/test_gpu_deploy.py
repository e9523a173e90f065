"""The deployment path on the GPU (csrc/deploy.hip, umamd/deploy.py):
um_frame_prep bit for bit against PIL's resize and against um_stereo_prep,
um_depth_post against the f64 reference of tests/_deploy_ref.py, and
DepthPipeline end to end (capture, replay, set_params, refresh) and the entries
each of its configurations launches, in order.

Bars of the float fields: per field max|gpu - ref64| <= 4 x max(max|ref32 -
ref64|, 2^-23 max|ref64|), ref32 the same reference evaluated in f32 on the
CPU (the factor covers another summation order of the 16 taps and FMA
contraction); depth by the same rule on the relative error over disparity >
min_disp.  The mask must equal the f64 reference wherever no reference value
lies within its field's bar of a threshold (those pixels, at most 1 %, are left
out; the depth gate leaves out the same pixels around min_disp).

Measured on an MI355X, gpu error / max(ref32 error, 2^-23 max|ref64|) per
field (disparity, uncertainty, lr_error, depth; the bar is 4; also DESIGN
section 5):
  um_depth_post  8x16 -> 19x37    1.04  1.04  1.01  1.03  (9.2e-6 / 7.9e-6 px)
                 8x16 -> 8x16     0     0     0.87  0.48  (disparity, sigma exact)
                 8x16 -> 3x5      0.59  0.23  1.00  0.82
                 64x128 -> 150x262  1.00  1.00  1.00  1.00  (7.8e-4 / 7.0e-4 px)
  pipeline fp32  64x128 -> 150x262  1.00  0.99  0.90  1.03
  pipeline bf16  64x128 -> 150x262  1.00  1.00  0.66  0.97
  mask: pixels left out 0 (8x16), 1.5e-4 (150x262), 4.2e-4 / 6.0e-4 (pipeline
  fp32 / bf16, thresholds at the outputs' quartiles); no mismatch elsewhere.
The ratios sit at 1 because the dominant error is shared with ref32: the f32
scale (in - 1) / (out - 1) of the upsample and the f32 sample position.
"""
import numpy as np
import pytest
import torch

import _deploy_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---------------------------------------------------------- um_frame_prep --
def _frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))


def _frame_prep(frames, hd, wd, expect_ok=True):
    from umamd import _lib as L
    from umamd.imageprep import resize_coeffs
    n, hs, ws, _ = frames.shape
    bh, kh, ksh = resize_coeffs(ws, wd)
    bv, kv, ksv = resize_coeffs(hs, hd)
    assert L.query('um_frame_prep_ok', hs, ws, hd, wd, ksh, ksv) == int(expect_ok)
    t = [torch.from_numpy(a).to(DEV) for a in (bh, kh, bv, kv)]
    src = frames.to(DEV)
    out = torch.full((n, 3, hd, wd), -1.0, device=DEV)
    L.call('um_frame_prep', n, hs, ws, L.ptr(src), hd, wd, L.ptr(t[0]), L.ptr(t[1]), ksh,
           L.ptr(t[2]), L.ptr(t[3]), ksv, L.ptr(out))
    torch.cuda.synchronize()
    return out


def _largest_accepted():
    """the largest source the gate takes for a 2 x 2 destination"""
    from umamd import _lib as L
    from umamd.imageprep import resize_coeffs

    def ok(hs, ws):
        return L.query('um_frame_prep_ok', hs, ws, 2, 2, resize_coeffs(ws, 2)[2],
                       resize_coeffs(hs, 2)[2])
    hs = max(h for h in range(2, 400) if ok(h, 2))
    ws = max(w for w in range(2, 400) if ok(2, w))
    assert not ok(hs + 1, 2) and not ok(2, ws + 1)
    return hs, ws


@pytest.mark.parametrize('case', ['down', 'up', 'identity', 'largest'])
def test_frame_prep_bit_exact(case):
    from umamd.imageprep import stereo_prep
    if case == 'largest':
        src, dst = _largest_accepted(), (2, 2)
        assert src == (113, 256)
    else:
        src, dst = {'down': ((37, 53), (16, 24)), 'up': ((12, 20), (16, 24)),
                    'identity': ((16, 24), (16, 24))}[case]
    frames = _frames(3, *src, seed=src[0])
    got = _frame_prep(frames, *dst).cpu()
    assert torch.equal(got, R.frame_prep_ref(frames, *dst))
    prep = torch.zeros(3, 8)
    prep[:, 2:7] = 1
    sp = stereo_prep({'left': frames, 'right': frames, 'prep': prep}, dst, torch.device(DEV))
    assert torch.equal(got, sp['left'].cpu())


def test_frame_prep_refuses_past_the_limit():
    from umamd._lib import UmamdError
    hs, ws = _largest_accepted()
    with pytest.raises(UmamdError, match=r'resize limit.*at most 512.*64 KiB'):
        _frame_prep(_frames(1, hs + 1, 8, seed=1), 2, 2, expect_ok=False)
    with pytest.raises(UmamdError, match=r'ks_h at most 257'):
        _frame_prep(_frames(1, 8, ws + 2, seed=1), 2, 2, expect_ok=False)


# ---------------------------------------------------------- um_depth_post --
FB, UNC = 100.0, 0.15
FIELDS = ('disparity', 'depth', 'uncertainty', 'lr_error', 'valid')


def _pred(n, h, w, seed=5):
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(n, 2, h, w, generator=g) * 0.5
    s = torch.rand(n, 2, h, w, generator=g) * 0.3
    return torch.cat([d, s], 1)


def _depth_post(pred_nchw, hs, ws, gates, sp=4, sn_extra=0, skip=()):
    """pred -> NHWC device buffer with pixel stride ``sp`` and ``sn_extra``
    floats between images (filled with NaN: never read) -> outputs"""
    from umamd import _lib as L
    n, _, h, w = pred_nchw.shape
    sn = h * w * sp + sn_extra
    buf = torch.full((n * sn,), float('nan'), device=DEV)
    view = buf.as_strided((n, h, w, 4), (sn, w * sp, sp, 1))
    view.copy_(pred_nchw.permute(0, 2, 3, 1))
    params = torch.tensor(gates, dtype=torch.float32, device=DEV)
    out = {k: None if k in skip else
           torch.full((n, hs, ws), 7, dtype=torch.uint8 if k == 'valid' else torch.float32,
                      device=DEV) for k in FIELDS}
    L.call('um_depth_post', L.ptr(buf), sn, sp, n, h, w, hs, ws, L.ptr(params),
           *[L.ptr(out[k]) for k in FIELDS])
    torch.cuda.synchronize()
    if out['valid'] is not None:
        assert bool((out['valid'] <= 1).all())
    return out


POST_CASES = {
    'up_odd': ((8, 16), (19, 37), {}),
    'identity': ((8, 16), (8, 16), {}),
    'down': ((8, 16), (3, 5), {}),
    'large': ((64, 128), (150, 262), {}),
    'strided': ((8, 16), (19, 37), dict(sp=8, sn_extra=24)),
    'null_outputs': ((8, 16), (19, 37), dict(skip=('depth', 'lr_error'))),
    'only_disparity': ((8, 16), (19, 37), dict(skip=('depth', 'uncertainty', 'lr_error',
                                                     'valid'))),
}


@pytest.mark.parametrize('case', sorted(POST_CASES))
def test_depth_post_matches_f64_reference(case):
    (h, w), (hs, ws), kw = POST_CASES[case]
    pred = _pred(2, h, w)
    gates = (FB, 0.05 * ws, UNC, 0.2 * ws)
    out = _depth_post(pred, hs, ws, gates, **kw)
    for k in kw.get('skip', ()):
        assert out[k] is None
    R.check_post(out, pred, hs, ws, *gates, label=f'depth_post {case} {h}x{w}->{hs}x{ws}')
    if case == 'identity':  # to 1 ulp (here: exactly; x * 16 is exact)
        d, u = out['disparity'].cpu(), out['uncertainty'].cpu()
        ref_d = pred[:, 0] * w
        assert bool(((d - ref_d).abs() <= 2.0 ** -23 * ref_d.abs()).all())
        assert bool(((u - pred[:, 2]).abs() <= 2.0 ** -23 * pred[:, 2].abs()).all())


def test_depth_post_unaligned_outputs():
    """output pointers that are not 16-byte aligned take the scalar stores
    and give the same values"""
    from umamd import _lib as L
    pred = _pred(2, 8, 16)
    hs, ws = 19, 37
    gates = (FB, 0.05 * ws, UNC, 0.2 * ws)
    want = _depth_post(pred, hs, ws, gates)
    buf = pred.permute(0, 2, 3, 1).contiguous().to(DEV)
    params = torch.tensor(gates, dtype=torch.float32, device=DEV)
    n = 2 * hs * ws
    f = [torch.zeros(n + 1, device=DEV) for _ in range(4)]
    v = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
    L.call('um_depth_post', L.ptr(buf), 8 * 16 * 4, 4, 2, 8, 16, hs, ws, L.ptr(params),
           *[L.ptr(t[1:]) for t in f], L.ptr(v[1:]))
    torch.cuda.synchronize()
    for k, t in zip(FIELDS, f + [v]):
        assert torch.equal(t[1:].view(2, hs, ws), want[k]), k
        assert float(t[0]) == 0


def test_depth_post_argument_errors():
    from umamd import _lib as L
    buf = torch.zeros(2 * 8 * 16 * 4, device=DEV)
    params = torch.zeros(4, device=DEV)
    out = torch.zeros(2 * 19 * 37, device=DEV)
    for h, w, hs, ws in ((1, 16, 19, 37), (8, 1, 19, 37), (8, 16, 1, 37), (8, 16, 19, 1)):
        with pytest.raises(L.UmamdError, match='every size >= 2'):
            L.call('um_depth_post', L.ptr(buf), 8 * 16 * 4, 4, 2, h, w, hs, ws, L.ptr(params),
                   L.ptr(out), None, None, None, None)
    with pytest.raises(L.UmamdError, match='strides'):
        L.call('um_depth_post', L.ptr(buf), 8 * 16 * 4, 3, 2, 8, 16, 19, 37, L.ptr(params),
               L.ptr(out), None, None, None, None)


# ---------------------------------------------------------- DepthPipeline --
B, H, W, HS, WS = 2, 64, 128, 150, 262
GATES = dict(focal_baseline=FB, min_disparity=0.05 * WS, max_uncertainty=UNC,
             max_lr_error=0.2 * WS)


def _model(dtype='fp32'):
    import test_gpu_infer as TI
    return TI._model(TI._cfg(), dtype).eval()


@pytest.fixture(scope='module')
def model():
    return _model()


def _pipe(m, **kw):
    from umamd.deploy import DepthPipeline
    return DepthPipeline(m, HS, WS, batch=B, height=H, width=W, scale=0.3, **{**GATES, **kw})


def _clone(out):
    return {k: v.clone() for k, v in out.items()}


def _quartiles(out):
    """thresholds inside the range of the pipeline's own outputs: each gate
    alone passes three quarters of the pixels"""
    def q(k, f):
        return float(torch.quantile(out[k].flatten(), f))
    return dict(min_disparity=q('disparity', 0.25), max_uncertainty=q('uncertainty', 0.75),
                max_lr_error=q('lr_error', 0.75))


def _check_against_own_prediction(pipe, out, label):
    p = pipe.params
    R.check_post(out, out['prediction'].float(), HS, WS, p['focal_baseline'], p['min_disparity'],
                 p['max_uncertainty'], p['max_lr_error'], label=label)


def test_pipeline_stages_and_modes(model):
    from umamd._lib import UmamdError
    from umamd.infer import InferenceEngine
    frames = _frames(B, HS, WS, seed=11)
    pipe = _pipe(model)
    with pytest.raises(UmamdError, match='before the first call'):
        pipe.last()
    out = _clone(pipe(frames))
    assert out['valid'].dtype == torch.bool and out['prediction'].shape == (B, 4, H, W)
    for k in ('disparity', 'depth', 'uncertainty', 'lr_error', 'valid'):
        assert out[k].shape == (B, HS, WS), k
    # stage 1: the engine's static input is the PIL-resized frame
    assert torch.equal(pipe.infer._in.cpu(), R.frame_prep_ref(frames, H, W))
    # stage 2: the forward is the stand-alone engine's
    eng = InferenceEngine(model, B, H, W, 0.3, capture=False)
    d, u = eng(pipe.infer._in.clone())
    assert torch.equal(out['prediction'], torch.cat([d, u], 1))
    # stage 3: thresholds inside the outputs' range, then the bars
    pipe.set_params(**_quartiles(out))
    out = _clone(pipe(frames))
    assert 0.2 < float(out['valid'].float().mean()) < 0.8
    _check_against_own_prediction(pipe, out, 'pipeline fp32')
    # capture=False: the same launches eagerly
    eager = _pipe(model, capture=False, **pipe.params)
    assert eager._graph is None and pipe._graph is not None
    oe = eager(frames)
    for k in out:
        assert torch.equal(out[k], oe[k]), k
    assert all(torch.equal(a, b) for a, b in zip(pipe.last().values(), out.values()))
    # device frames == host frames == pinned host frames
    for f in (frames.to(DEV), frames.pin_memory()):
        od = pipe(f)
        for k in out:
            assert torch.equal(out[k], od[k]), k
    # other frames change the outputs: what a fresh pipeline computes for them
    frames2 = _frames(B, HS, WS, seed=12)
    o2 = _clone(pipe(frames2))
    assert not torch.equal(o2['disparity'], out['disparity'])
    fresh = _pipe(model, **pipe.params)(frames2)
    for k in o2:
        assert torch.equal(o2[k], fresh[k]), k
    with pytest.raises(ValueError, match='built for frames'):
        pipe(frames[:1])
    with pytest.raises(TypeError, match='uint8'):
        pipe(frames.float())


def test_pipeline_set_params_without_recapture(model):
    frames = _frames(B, HS, WS, seed=11)
    pipe = _pipe(model, max_uncertainty=float('inf'), max_lr_error=float('inf'),
                 min_disparity=1e-3)
    g = pipe._graph
    a = _clone(pipe(frames))
    pipe.set_params(max_uncertainty=float(a['uncertainty'].median()))
    b = _clone(pipe(frames))
    assert pipe._graph is g
    assert torch.equal(a['disparity'], b['disparity']) and torch.equal(a['depth'], b['depth'])
    assert int(b['valid'].sum()) < int(a['valid'].sum())
    assert torch.equal(b['valid'], a['valid'] & (a['uncertainty'] <= pipe.params['max_uncertainty']))
    pipe.set_params(focal_baseline=7.0, max_uncertainty=float('inf'))
    c = pipe(frames)
    assert pipe._graph is g and torch.equal(c['valid'], a['valid'])
    far = (a['depth'] > 0).cpu()
    disp = a['disparity'].cpu()[far]
    assert torch.equal(c['depth'].cpu()[far], torch.full_like(disp, 7.0) / disp)  # IEEE division
    with pytest.raises(TypeError, match='unknown'):
        pipe.set_params(baseline=1.0)


def test_pipeline_refresh():
    m = _model()
    frames = _frames(B, HS, WS, seed=11)
    pipe = _pipe(m)
    a = _clone(pipe(frames))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 4:
                p.mul_(1.05)
    assert torch.equal(pipe(frames)['prediction'], a['prediction'])  # until refresh()
    g = pipe._graph
    pipe.refresh()
    b = pipe(frames)
    assert pipe._graph is g  # in place: no parameter moved
    assert not torch.equal(b['prediction'], a['prediction'])
    assert bool(torch.isfinite(b['prediction']).all())


def test_pipeline_bf16():
    m = _model('bf16')
    frames = _frames(B, HS, WS, seed=11)
    pipe = _pipe(m)
    out = _clone(pipe(frames))
    for k in ('disparity', 'depth', 'uncertainty', 'lr_error', 'prediction'):
        assert bool(torch.isfinite(out[k]).all()), k
    pipe.set_params(**_quartiles(out))
    out = _clone(pipe(frames))
    assert 0.2 < float(out['valid'].float().mean()) < 0.8
    _check_against_own_prediction(pipe, out, 'pipeline bf16')


# which entries a configuration launches, and in which order
ENTRIES = ('um_frame_rectify', 'um_frame_prep', 'um_depth_post', 'um_valid_and', 'um_value_range',
           'um_depth_render', 'um_depth_backproject', 'um_depth_cloud')
K = (900.0, 900.0, 131.0, 75.0)
LAUNCHES = {
    'plain': ({}, 'frame_prep depth_post'),
    'render_fixed': (dict(render='depth', render_range=(0.0, 40.0)),
                     'frame_prep depth_post depth_render'),
    'render_auto': (dict(render='depth', render_range='auto'),
                    'frame_prep depth_post value_range depth_render'),
    'points_map': (dict(points='map', intrinsics=K), 'frame_prep depth_post depth_backproject'),
    'points_cloud': (dict(points='cloud', intrinsics=K), 'frame_prep depth_post depth_cloud'),
    'points_both': (dict(points='both', intrinsics=K),
                    'frame_prep depth_post depth_backproject depth_cloud'),
    'rectify': (dict(rectify=True), 'frame_rectify frame_prep depth_post valid_and'),
    'all': (dict(rectify=True, render='depth', render_range='auto', points='both'),
            'frame_rectify frame_prep depth_post valid_and value_range depth_render '
            'depth_backproject depth_cloud'),
}


@pytest.mark.parametrize('case', sorted(LAUNCHES))
def test_pipeline_launch_sequence(model, case):
    """one eager call launches exactly the deployment entries of its
    configuration, in the fixed order rectify -> prep -> (forward) -> post ->
    mask-and -> render -> points, and nothing of a stage that is off"""
    from umamd import _lib as L
    kw, want = LAUNCHES[case]
    if kw.get('rectify'):
        import test_gpu_rectify as TR
        cam = TR._cam()
        kw = {**kw, 'rectify': cam, 'focal_baseline': cam.focal_baseline}
        if 'points' in kw:
            kw['intrinsics'] = cam.intrinsics
        pipe = TR._pipe(model, capture=False, **kw)
        frames = TR.R.frames(TR.B, *TR.RAW, seed=21)
    else:
        pipe = _pipe(model, capture=False, **kw)
        frames = _frames(B, HS, WS, seed=11)
    assert pipe._graph is None
    with L.Recorder(ENTRIES) as rec:
        pipe(frames)
    torch.cuda.synchronize()
    assert [item[0] for item in rec.items] == ['um_' + name for name in want.split()]
