"""The refine stage without a GPU: the numpy restatements of tests/_refine_ref.py
against their f64 variants and against what the filters are for (edges kept,
flicker damped), the two C-ABI entries in the header and the binding, and the
argument errors of umamd.refine and DepthPipeline(refine=...), all raised
before any GPU work.

Bars of the f32-against-f64 comparisons, from the roundings of the definition
(u = 2^-24, the relative error of one f32 operation):
  smooth  every term of the sums is positive on the planted scene, so relative
          errors add: a weight carries 5 roundings (u*u, + eps, 1 /, S * G,
          * c), a term one more, a sum of T taps T - 1, the division 1:
          |out32 - out64| <= (2 T + 10) u |out64|, T = (2 R + 1)^2.
  fuse    mean' = mean + K * (d - mean) with 0 <= K <= 1: with M = max(|d|,
          |mean|), e costs 2 u M, K three roundings on a factor <= 2 M, the
          product and the sum 2 u M and u M: 11 u M; var' the same with M = p.
          The state carries its error on (damped by 1 - K, never amplified):
          11 (t + 1) u M after frame t.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import _refine_ref as R

ENTRIES = ('um_disp_smooth', 'um_disp_fuse')
U = 2.0 ** -24
PARAMS = (100.0, 5.0, 0.3, 1.5)             # fb, min_disp, max_unc, max_lr
FP = (1e-4, 2.0, 0.25, 0.05, 9.0, 0, 0, 0)  # eps, a, floor, q, g2 = 3^2


def _tables(radius, sigma_space=1.5, sigma_colour=30.0):
    from umamd.refine import tables
    return tables(radius, sigma_space, sigma_colour)


def test_tables_are_the_rounded_f64_gaussians():
    S, G = _tables(2, 1.5, 30.0)
    assert S.dtype == torch.float32 and S.shape == (9,) and G.shape == (768,)
    assert float(S[0]) == 1.0 and float(G[0]) == 1.0
    assert float(S[1 * 3 + 2]) == float(np.float32(math.exp(-5 / 4.5)))
    assert float(G[100]) == float(np.float32(math.exp(-10000 / 1800.0)))
    assert bool((G[1:] <= G[:-1]).all()) and float(G[767]) == 0.0


@pytest.mark.parametrize('radius,step', [(1, 1), (2, 4), (3, 5)])
def test_smooth_f32_within_its_bar_of_f64(radius, step):
    """on the planted inputs, with 1e12 in place of 1e30: u * u overflows in
    f32 there, the confidence is exactly 0 and the formats differ by
    definition.  Where all taps are skipped both pass the raw value through."""
    shape = (2, 37, 71)
    disp, unc, frame, lone = R.planted(shape, 3, radius, step)
    S, G = _tables(radius)
    u12 = torch.where(unc > 1e29, torch.tensor(1e12), unc)
    o32 = R.smooth_ref(disp, u12, frame, radius, step, S, G, FP[0])
    o64 = R.smooth_ref(disp, u12, frame, radius, step, S, G, FP[0], np.float64)
    bar = (2 * (2 * radius + 1) ** 2 + 10) * U
    for a, b, raw in zip(o32, o64, (disp, u12)):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        same = a.double().view(torch.int64) == b.view(torch.int64)  # the raw value, NaN included
        near = (a.double() - b).abs() <= bar * b.abs()
        assert bool((near | same).all())
        assert int(near.sum()) >= 0.9 * a.numel()
    # the two lone pixels of the planted inputs pass through, bit for bit
    o32 = R.smooth_ref(disp, unc, frame, radius, step, S, G, FP[0])
    for n, y, x in lone:
        assert R.same_bits(o32[0][n, y, x], disp[n, y, x])
        assert R.same_bits(o32[1][n, y, x], unc[n, y, x])
    assert math.isinf(float(o32[0][lone[0]])) and math.isfinite(float(o32[0][lone[1]]))
    assert float(o32[1][lone[0]]) == 0.125 and float(o32[1][lone[1]]) > 1e29


def test_smooth_keeps_a_constant_map():
    shape = (1, 19, 23)
    _, unc, frame = R.edge_scene(shape, 5)
    disp = torch.full(shape, 37.25)
    S, G = _tables(2)
    out, _ = R.smooth_ref(disp, unc, frame, 2, 3, S, G, FP[0])
    assert bool(((out - 37.25).abs() <= (2 * 25 + 10) * U * 37.25).all())
    # and a map nobody is confident about comes back as it was
    raw = R.smooth_ref(disp, torch.full(shape, 1e30), frame, 2, 3, S, G, FP[0])
    assert R.same_bits(raw[0], disp)


def test_smooth_follows_the_colour_edge():
    """sigma_colour far below the frame's step keeps the disparity jump within
    one pixel column; a huge sigma_colour (a plain Gaussian) smears it"""
    shape = (1, 21, 40)
    disp, unc, frame = R.edge_scene(shape, 7, noise=0.0)
    unc = torch.full(shape, 0.1)
    assert R.EDGE_STEP * 3 > 4 * 30.0  # the step, summed over the channels, against sigma_c
    edge = shape[2] // 2
    for step in (1, 2):
        sharp, _ = R.smooth_ref(disp, unc, frame, 2, step, *_tables(2, 1.5, 30.0), FP[0])
        blur, _ = R.smooth_ref(disp, unc, frame, 2, step, *_tables(2, 1.5, 1e6), FP[0])
        assert bool(((sharp[..., :edge] - R.D_LEFT).abs() < 1e-3).all())
        assert bool(((sharp[..., edge:] - R.D_RIGHT).abs() < 1e-3).all())
        mid = blur[..., edge - 1:edge + 1]
        assert bool(((mid < R.D_LEFT - 2) & (mid > R.D_RIGHT + 2)).all())
        assert bool(((blur[..., :edge - 2 * step] - R.D_LEFT).abs() <= 60 * U * R.D_LEFT).all())


def test_smooth_weights_by_confidence():
    """one confident tap among doubtful ones pulls the result to itself"""
    shape = (1, 5, 5)
    frame = torch.full(shape + (3,), 90, dtype=torch.uint8)
    disp = torch.full(shape, 10.0)
    unc = torch.full(shape, 1.0)
    disp[0, 2, 3], unc[0, 2, 3] = 30.0, 0.01
    out, unc_out = R.smooth_ref(disp, unc, frame, 1, 1, *_tables(1), FP[0])
    assert float(out[0, 2, 2]) > 29.9 and float(unc_out[0, 2, 2]) < 0.02
    assert abs(float(out[0, 0, 0]) - 10.0) <= 28 * U * 10.0  # out of the tap's reach


def _run_sequence(seq, dtype, shape):
    state = R.empty_state(shape)
    outs = []
    for d, u, lr in seq:
        o = R.fuse_ref(d, u, lr, PARAMS, FP, state, dtype)
        state = (o['mean'], o['var'])
        outs.append(o)
    return outs


def test_fuse_f32_within_its_bar_of_f64_and_takes_every_branch():
    shape = (2, 37, 71)
    seq = R.sequence(shape, 11)
    o32, o64 = _run_sequence(seq, np.float32, shape), _run_sequence(seq, np.float64, shape)
    for t, (a, b, (d, _, _)) in enumerate(zip(o32, o64, seq)):
        for k in ('keep', 'reset', 'stale'):
            assert torch.equal(a[k], b[k]), (t, k)  # no decision sits at a threshold
            assert bool(a[k].any()) or (t == 0 and k == 'keep'), (t, k)
        held = a['var'] >= 0
        M = torch.maximum(d.double().abs().nan_to_num(0.0, 0.0, 0.0), b['mean'].abs())
        assert bool((((a['mean'].double() - b['mean']).abs() <= 11 * (t + 1) * U * M) | ~held).all())
        assert bool((((a['var'].double() - b['var']).abs() <= 11 * (t + 1) * U * (b['var'] + FP[3]))
                     | ~held).all())
        assert torch.equal(a['valid'], b['valid'])
    a = o32[0]
    assert not a['keep'].any()                       # an empty state cannot keep
    assert R.same_bits(a['mean'][a['reset']], seq[0][0][a['reset']])
    assert bool((a['var'][a['stale']] == -1).all())  # still empty
    assert R.same_bits(a['disparity'][a['stale']], seq[0][0][a['stale']])  # D = d, NaN included


def test_fuse_reset_and_stale_branches():
    """a jump larger than the gate restarts the state at the measurement; a
    measurement that is not fresh leaves the state untouched and is hidden"""
    shape = (1, 1, 4)
    lr = torch.zeros(shape)
    u = torch.full(shape, 0.1)
    st = (torch.full(shape, 20.0), torch.full(shape, 0.2))
    m = np.float32(np.float32(np.float32(2.0) * np.float32(0.1)) ** 2 + np.float32(0.25))
    gate = 3 * math.sqrt(0.2 + 0.05 + float(m))
    d = torch.tensor([[[20.0 + 0.9 * gate, 20.0 + 1.1 * gate, float('nan'), 20.5]]])
    u[0, 0, 3] = float('inf')
    o = R.fuse_ref(d, u, lr, PARAMS, FP, st)
    assert o['keep'].flatten().tolist() == [True, False, False, False]
    assert o['reset'].flatten().tolist() == [False, True, False, False]
    assert o['stale'].flatten().tolist() == [False, False, True, True]
    assert float(o['mean'][0, 0, 1]) == float(d[0, 0, 1]) and float(o['var'][0, 0, 1]) == float(m)
    assert 20.0 < float(o['mean'][0, 0, 0]) < float(d[0, 0, 0])
    assert float(o['var'][0, 0, 0]) < min(0.25, float(m))
    for i in (2, 3):
        assert float(o['mean'][0, 0, i]) == 20.0 and float(o['var'][0, 0, i]) == float(st[1][0, 0, i])
        assert float(o['disparity'][0, 0, i]) == 20.0
    assert o['valid'].flatten().tolist() == [True, True, True, False]  # U = s = inf > max_unc


def test_fuse_variance_falls_to_its_fixed_point():
    shape = (1, 8, 8)
    g = torch.Generator().manual_seed(2)
    u = torch.full(shape, 0.15)
    a, floor, q = FP[1], FP[2], FP[3]
    m = (a * 0.15) ** 2 + floor
    fixed = (-q + math.sqrt(q * q + 4 * q * m)) / 2  # v = (v + q) m / (v + q + m)
    state, last = R.empty_state(shape), None
    for t in range(40):
        d = 25.0 + (torch.rand(shape, generator=g) - 0.5) * 0.4
        o = R.fuse_ref(d, u, torch.zeros(shape), PARAMS, FP, state)
        state = (o['mean'], o['var'])
        assert bool(o['keep'].all()) == (t > 0)
        if last is not None:  # strictly down while far from the fixed point, then to rounding
            assert bool((o['var'] < last).all() if t < 6 else (o['var'] <= last * (1 + 4 * U)).all())
        last = o['var']
        assert bool((o['var'] >= fixed * (1 - 1e-5)).all())
    assert bool(((last - fixed).abs() <= 1e-5 * fixed).all())
    assert bool(((o['disparity'] - 25.0).abs() < 0.2).all())


def test_fuse_without_state_is_the_gate_of_depth_post():
    shape = (2, 5, 7)
    d, u, lr = R.sequence(shape, 4, frames=1)[0]
    o = R.fuse_ref(d, u, lr, PARAMS, FP)
    assert R.same_bits(o['disparity'], d) and R.same_bits(o['uncertainty'], u)
    far = d > PARAMS[1]
    assert torch.equal(o['depth'][far], torch.full_like(d, PARAMS[0])[far] / d[far])
    assert not o['depth'][~far].any()
    assert torch.equal(o['valid'], far & (u <= PARAMS[2]) & (lr <= PARAMS[3]))


def test_entries_in_header_and_binding():
    from umamd import _lib
    src = open(os.path.join(REPO, 'include', 'umamd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib._SIG, name
        assert hasattr(_lib.lib(), name)


def test_refine_argument_errors_without_gpu():
    from umamd._lib import UmamdError
    from umamd.refine import RefineStage, fuse, smooth, tables

    def stage(refine='both', radius=2, step=2, **kw):
        v = dict(sigma_space=1.5, sigma_colour=30.0, conf_eps=1e-4, noise_scale=20.0,
                 var_floor=0.25, process_noise=1.0, gate=3.0)
        v.update(kw)
        return RefineStage(refine, radius, step, *v.values())

    assert stage().params['gate'] == 3.0 and stage(radius=3, step=5).step == 5
    for bad in ('bilateral', 'Spatial', True, 3):
        with pytest.raises(ValueError, match='refine='):
            stage(refine=bad)
    for radius, step, what in ((0, 1, 'radius'), (4, 1, 'radius'), (2.0, 1, 'radius'),
                               (2, 0, 'step'), (2, 1.5, 'step'), (2, True, 'step'),
                               (3, 6, 'radius \\* step'), (2, 9, 'radius \\* step')):
        with pytest.raises(ValueError, match=what):
            stage(radius=radius, step=step)
    for k, v in (('sigma_space', -1.0), ('sigma_colour', -30.0), ('sigma_colour', 0.0),
                 ('conf_eps', -1e-4), ('noise_scale', float('nan')), ('var_floor', float('inf')),
                 ('process_noise', -1.0), ('gate', 0.0), ('gate', '3')):
        with pytest.raises(ValueError, match=k):
            stage(**{k: v})
    assert stage(gate=float('inf')).params['gate'] == math.inf
    with pytest.raises(ValueError, match='sigma_space'):
        tables(2, -1.5, 30.0)
    with pytest.raises(ValueError, match='sigma_colour'):
        tables(2, 1.5, -30.0)
    with pytest.raises(ValueError, match='radius'):
        tables(4, 1.5, 30.0)
    with pytest.raises(ValueError, match='sigma_space'):
        stage().check_params(dict(sigma_space=-2.0))
    # the stand-alone functions check on the host too
    d = torch.zeros(2, 5, 7)
    f = torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='radius \\* step'):
        smooth(d, d.clone(), f, radius=3, step=6)
    with pytest.raises(TypeError, match='uint8'):
        smooth(d, d.clone(), f.float())
    with pytest.raises(ValueError, match='contiguous'):
        smooth(d, torch.zeros(2, 5, 8), f)
    with pytest.raises(UmamdError, match='HIP device'):
        smooth(d, d.clone(), f)
    with pytest.raises(ValueError, match='gate'):
        fuse(d, d.clone(), gate=-1.0)
    with pytest.raises(UmamdError, match='HIP device'):
        fuse(d, d.clone())


def test_pipeline_argument_errors_without_gpu():
    import test_deploy_cpu as TD
    from umamd._lib import UmamdError
    from umamd.deploy import DepthPipeline
    m = TD._cpu_model()
    kw = dict(height=64, width=128)
    with pytest.raises(ValueError, match='refine='):
        DepthPipeline(m, 150, 262, refine='bilateral', **kw)
    with pytest.raises(ValueError, match='radius'):
        DepthPipeline(m, 150, 262, refine='spatial', refine_radius=4, **kw)
    with pytest.raises(ValueError, match='step'):
        DepthPipeline(m, 150, 262, refine='spatial', refine_step=0, **kw)
    with pytest.raises(ValueError, match='radius \\* step'):
        DepthPipeline(m, 150, 262, refine='both', refine_radius=3, refine_step=6, **kw)
    with pytest.raises(ValueError, match='radius \\* step'):  # the default step: round(1280 / 128)
        DepthPipeline(m, 150, 1280, refine='both', **kw)
    with pytest.raises(ValueError, match='sigma_colour'):
        DepthPipeline(m, 150, 262, refine='temporal', sigma_colour=-1.0, **kw)
    with pytest.raises(UmamdError, match='HIP device'):  # all of it passed: the GPU comes next
        DepthPipeline(m, 150, 262, refine='both', **kw)
    # a pipeline without the stage knows none of its keys
    pipe = object.__new__(DepthPipeline)
    pipe._tunable, pipe._refine_stage = [], None
    for k in ('sigma_space', 'sigma_colour', 'conf_eps', 'noise_scale', 'var_floor',
              'process_noise', 'gate', 'refine_radius', 'refine_step'):
        with pytest.raises(TypeError, match='unknown'):
            pipe.set_params(**{k: 1.0})
    pipe.reset_refine()  # nothing to do
    assert not any(p.is_cuda for p in m.parameters())
