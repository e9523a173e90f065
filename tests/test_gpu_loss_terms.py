"""The standalone, differentiable loss terms on the HIP path (csrc/lossterms.hip
through umamd.lossterms and the modules of train/loss.py) against the f64 CPU
oracle and the reference's fixture (tests/golden/loss_terms.npz).

Bars are the fused loss's existing ones (test_gpu_loss_stack.py,
test_gpu_loss_pooling.py): loss scalars within 1e-4 relative (1e-5 absolute
floor where a bayesian NLL can cancel), the error map within 1e-4 absolute,
gradients within 4e-3 rel-norm (bilinear cell flips between f32 and f64).
Shapes (_loss_terms_ref.SHAPES): a 1x1 SSIM grid, 4x5, one row and six columns
past a 16x64 tile, two tile rows, more than three tiles wide; 2x2 too where a
term allows it.  Nothing that goes through the LDS scatter is compared bit for
bit between two runs.  Marked gpu."""
import functools
import os

import numpy as np
import pytest
import torch

import _loss_terms_ref as R
from conftest import GOLDEN
from oracle import loss as OL
from test_loss_pooling_cpu import loss_cfg

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GRAD_BAR = 4e-3


def _leaf(t, dev=DEV):
    return t.detach().clone().to(dev).requires_grad_(True)


def _leaf64(t):
    return t.detach().clone().double().requires_grad_(True)


def _grads_ok(what, got, ref):
    for name, g, r in zip(what, got, ref):
        assert g is not None and torch.isfinite(g).all(), name
        e = R.rel_norm(g, r)
        print(name, 'grad rel-norm', e)
        assert e < GRAD_BAR, (name, e)


class _Calls:
    """the entry names that pass through _lib.call from the loss modules"""

    def __init__(self, monkeypatch):
        from umamd import _lib, lossfn, lossterms
        self.names, self.args = [], []

        def call(name, *a, **k):
            if name != 'um_pyramid':
                self.names.append(name)
                self.args.append(a)
            return _lib.call(name, *a, **k)
        monkeypatch.setattr(lossfn, 'call', call)
        monkeypatch.setattr(lossterms, 'call', call)


# ------------------------------------------------------------ WSSIM --------
@functools.lru_cache(maxsize=None)
def _wssim_ref(shape, params):
    im, rc, _, gmap = R.inputs(*shape)
    a, b = _leaf64(im), _leaf64(rc)
    loss, emap = R.wssim(a, b, *params)
    ga, gb = torch.autograd.grad((emap * gmap.double()).sum() + 3.0 * loss, (a, b))
    return float(loss), emap.detach(), ga, gb


@pytest.mark.parametrize('params', R.WSSIM_PARAMS + [(0.0, 0.01, 0.03), (1.0, 0.02, 0.05)])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_wssim_vs_oracle(shape, params):
    """forward's scalar, the map (with history, from forward and from
    image_error) and the gradient w.r.t. both operands under a non-uniform
    upstream gradient of the map plus the scalar's own path"""
    from train.loss import WeightedSSIMLoss
    im, rc, _, gmap = R.inputs(*shape)
    ref_loss, ref_map, ref_ga, ref_gb = _wssim_ref(shape, params)
    m = WeightedSSIMLoss(*params)
    a, b = _leaf(im), _leaf(rc)
    loss = m(a, b)
    emap = m.previous_image_error
    assert emap.requires_grad and tuple(emap.shape) == (shape[0], 2, shape[1], shape[2])
    print(shape, params, float(loss), ref_loss)
    assert R.close(loss, ref_loss)
    d = float((emap.detach().double().cpu() - ref_map).abs().max())
    print('map', d)
    assert d < 1e-4
    ga, gb = torch.autograd.grad((emap * gmap.to(DEV)).sum() + 3.0 * loss, (a, b))
    _grads_ok(('images', 'recon'), (ga, gb), (ref_ga, ref_gb))
    # image_error alone: the same map, differentiable through one operand only
    e2 = m.image_error(im.to(DEV), b)
    assert torch.equal(e2.detach(), emap.detach())
    gb2, = torch.autograd.grad((e2 * gmap.to(DEV)).sum(), (b,))
    loss_only_b = torch.autograd.grad(m(im.to(DEV), b), (b,))[0]
    assert R.rel_norm(gb2 + 3.0 * loss_only_b, ref_gb) < GRAD_BAR


def test_wssim_constants_are_used():
    """(0.02, 0.05) moves the value by far more than the bar"""
    from train.loss import WeightedSSIMLoss
    im, rc, _, _ = R.inputs(2, 17, 70)
    a = float(WeightedSSIMLoss(0.85)(im.to(DEV), rc.to(DEV)))
    b = float(WeightedSSIMLoss(0.85, 0.02, 0.05)(im.to(DEV), rc.to(DEV)))
    assert abs(a - b) > 5e-3 * abs(a)


@pytest.mark.parametrize('params', R.WSSIM_PARAMS)
def test_wssim_constant_equal_images(params):
    """images == recon, constant: variance 0, DSSIM at the clamp's edge"""
    from train.loss import WeightedSSIMLoss
    im = torch.full((2, 6, 17, 70), 0.4, device=DEV)
    a, b = _leaf(im), _leaf(im)
    m = WeightedSSIMLoss(*params)
    loss = m(a, b)
    ga, gb = torch.autograd.grad(loss + m.previous_image_error.sum(), (a, b))
    assert abs(float(loss)) < 1e-6
    assert torch.isfinite(ga).all() and torch.isfinite(gb).all()


@pytest.mark.parametrize('alpha,k1,k2', R.WSSIM_PARAMS)
def test_wssim_vs_reference_fixture(alpha, k1, k2):
    from train.loss import WeightedSSIMLoss
    z, t = R.fixture(), R.wtag(alpha, k1, k2)
    m = WeightedSSIMLoss(alpha, k1, k2)
    a, b = _leaf(torch.from_numpy(z['images'])), _leaf(torch.from_numpy(z['recon']))
    loss = m(a, b)
    emap = m.image_error(a, b)
    assert R.close(loss, z[f'{t}_loss'])
    assert float((emap.detach().cpu() - torch.from_numpy(z[f'{t}_map'])).abs().max()) < 1e-4
    g = torch.autograd.grad((emap * torch.from_numpy(z['gmap']).to(DEV)).sum(), (a, b))
    _grads_ok(('images', 'recon'), g, (z[f'{t}_gimg'], z[f'{t}_grec']))


# ------------------------------------------- consistency / smoothness / NLL --
@pytest.mark.parametrize('with_images', [False, True])
@pytest.mark.parametrize('shape', R.SHAPES_2X2)
def test_consistency_vs_oracle(shape, with_images):
    from train.loss import ConsistencyLoss
    _, _, pred, _ = R.inputs(*shape)
    d, i = pred[:, 0:2], pred[:, 2:4]
    dc, ic = _leaf64(d), _leaf64(i)
    dg, ig = _leaf(d), _leaf(i)
    if with_images:
        ref, got = OL.consistency_loss(dc, ic), ConsistencyLoss()(dg, ig)
        wrt_c, wrt_g, names = (dc, ic), (dg, ig), ('disp', 'images')
    else:
        ref, got = OL.consistency_loss(dc), ConsistencyLoss()(dg)
        wrt_c, wrt_g, names = (dc,), (dg,), ('disp',)
    print(shape, with_images, float(got), float(ref))
    assert R.close(got, ref)
    _grads_ok(names, torch.autograd.grad(2.0 * got, wrt_g), torch.autograd.grad(2.0 * ref, wrt_c))


@pytest.mark.parametrize('shape', R.SHAPES_2X2)
def test_smoothness_vs_oracle(shape):
    from train.loss import SmoothnessLoss
    im, _, pred, _ = R.inputs(*shape)
    dc, dg = _leaf64(pred[:, 0:2]), _leaf(pred[:, 0:2])
    ref, got = OL.smoothness_loss(dc, im.double()), SmoothnessLoss()(dg, im.to(DEV))
    print(shape, float(got), float(ref))
    assert R.close(got, ref)
    _grads_ok(('disp',), torch.autograd.grad(got, (dg,)), torch.autograd.grad(ref, (dc,)))


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
@pytest.mark.parametrize('shape', R.SHAPES_2X2)
def test_nll_vs_oracle(shape, lt):
    from train.loss import ReprojectionErrorLoss
    _, _, pred, gmap = R.inputs(*shape)
    err = 0.3 * gmap
    uc, ug = _leaf64(pred[:, 2:4]), _leaf(pred[:, 2:4])
    ref = R.nll(uc, err.double(), lt)
    got = ReprojectionErrorLoss(lt).loss_function(ug, err.to(DEV).requires_grad_(True))
    print(shape, lt, float(got), float(ref))
    assert R.close(got, ref, 1e-5)
    _grads_ok(('uncertainty',), torch.autograd.grad(got, (ug,)), torch.autograd.grad(ref, (uc,)))


@pytest.mark.parametrize('pooling', [False, True])
@pytest.mark.parametrize('lt', R.LOSS_TYPES)
@pytest.mark.parametrize('shape', R.SHAPES[1:])
def test_error_loss_vs_oracle(shape, lt, pooling):
    """ReprojectionErrorLoss.forward: the error detached, the pool (ATen), the
    split, the NLL, the smoothness and the F5 consistency; the prediction is
    channels-last, as the model's are"""
    from train.loss import ReprojectionErrorLoss
    im, _, pred, gmap = R.inputs(*shape)
    err = 0.3 * gmap
    pc = _leaf64(pred)
    ref = OL.error_loss(pc, im.double(), err.double(), lt, 0.3, 0.5, pooling)
    pg = pred.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    eg = err.to(DEV).requires_grad_(True)
    got = ReprojectionErrorLoss(lt, 0.3, 0.5, pooling)(pg, im.to(DEV), eg)
    print(shape, lt, pooling, float(got), float(ref))
    assert R.close(got, ref, 1e-5)
    got.backward()
    assert eg.grad is None  # detached by definition
    _grads_ok(('predicted',), (pg.grad,), torch.autograd.grad(ref, (pc,)))


def test_terms_vs_reference_fixture():
    from train import loss as TL
    z = R.fixture()
    pred = torch.from_numpy(z['pred'])
    images = torch.from_numpy(z['images']).to(DEV)
    d = _leaf(pred[:, 0:2])
    loss = TL.ConsistencyLoss()(d)
    assert R.close(loss, z['cons_self_loss'])
    _grads_ok(('cons_self',), torch.autograd.grad(loss, (d,)), (z['cons_self_gdisp'],))
    d, i = _leaf(pred[:, 2:4]), _leaf(pred[:, 0:2])
    loss = TL.ConsistencyLoss()(d, i)
    assert R.close(loss, z['cons_img_loss'])
    _grads_ok(('cons_img disp', 'cons_img images'), torch.autograd.grad(loss, (d, i)),
              (z['cons_img_gdisp'], z['cons_img_gimg']))
    d = _leaf(pred[:, 0:2])
    loss = TL.SmoothnessLoss()(d, images)
    assert R.close(loss, z['smooth_loss'])
    _grads_ok(('smooth',), torch.autograd.grad(loss, (d,)), (z['smooth_gdisp'],))
    # the error map the reference fed its own error term (stored as the default
    # WSSIM case's map): a map recomputed here differs from it by ~1e-5, enough to
    # turn the sign of an |u - e| whose terms nearly meet
    err = torch.from_numpy(z[R.wtag(0.85, 0.01, 0.03) + '_map']).to(DEV)
    for lt in R.LOSS_TYPES:
        for pooling in (False, True):
            t = f'err_{lt}_p{int(pooling)}'
            p = _leaf(pred)
            loss = TL.ReprojectionErrorLoss(lt, 0.3, 0.5, pooling)(p, images, err)
            print(t, float(loss), float(z[f'{t}_loss']))
            assert R.close(loss, z[f'{t}_loss'], 1e-5)
            _grads_ok((t,), torch.autograd.grad(loss, (p,)), (z[f'{t}_gpred'],))


def test_tukra_blended_vs_reference_fixture(monkeypatch):
    import yaml
    from conftest import REPO
    from train.loss import TukraUncertaintyLoss
    z = R.fixture()
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)['loss']
    cfg['error_loss_config']['loss_type'] = 'bayesian'
    lf = TukraUncertaintyLoss(**cfg)
    pyr = [torch.from_numpy(z[k]).to(DEV) for k in ('images', 'images1')]
    rec = [torch.from_numpy(z[k]).to(DEV) for k in ('recon', 'recon1')]
    ps = [_leaf(torch.from_numpy(z[k])) for k in ('pred', 'pred1')]
    calls = _Calls(monkeypatch)
    dl, el = lf(pyr, ps, rec, 0, None)
    assert 'um_loss_fwd' not in calls.names and 'um_image_error_k' in calls.names
    assert R.close(dl, z['tukra_disp']) and R.close(el, z['tukra_error'], 1e-5)
    assert tuple(lf.wssim.previous_image_error.shape) == (2, 2, 10, 18)
    assert float(lf.last_terms[0]) == float(dl) and float(lf.last_terms[1]) == float(el)
    _grads_ok(('pred0', 'pred1'), torch.autograd.grad(dl + el, ps),
              (z['tukra_gpred0'], z['tukra_gpred1']))


# -------------------------------------------------------- strided inputs ----
def test_channel_slices_of_nhwc_without_a_copy(monkeypatch):
    """disp and uncertainty as channel slices of one NHWC [N,h,w,4] tensor:
    passed by pointer and strides, the gradient arrives in the parent, results
    as from contiguous copies"""
    from train import loss as TL
    N, H, W = 2, 17, 70
    im, _, pred, gmap = R.inputs(N, H, W)
    parent = pred.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)  # [N,h,w,4]
    logical = parent.permute(0, 3, 1, 2)
    disp, unc = logical[:, 0:2], logical[:, 2:4]
    err = (0.3 * gmap).to(DEV)
    calls = _Calls(monkeypatch)

    def total(d, u):
        return TL.ConsistencyLoss()(u, d) + TL.ConsistencyLoss()(d) + \
            TL.SmoothnessLoss()(d, im.to(DEV)) + TL.ReprojectionErrorLoss('bayesian').loss_function(u, err)
    got = total(disp, unc)
    # the first consistency: uncertainty = channels 2-3 of the parent, sampled = 0-1
    a = calls.args[calls.names.index('um_consistency_fwd')]
    assert a[0] == parent.data_ptr() + 8 and a[4] == parent.data_ptr()
    assert tuple(a[1:4]) == tuple(a[5:8]) == (H * W * 4, 1, 4)
    got.backward()
    pc = _leaf(pred)
    ref = total(pc[:, 0:2].contiguous(), pc[:, 2:4].contiguous())
    ref.backward()
    assert R.close(got, ref)
    assert R.rel_norm(parent.grad.permute(0, 3, 1, 2), pc.grad) < GRAD_BAR
    p64 = _leaf64(pred)
    d64, u64 = p64[:, 0:2], p64[:, 2:4]
    o = OL.consistency_loss(u64, d64) + OL.consistency_loss(d64) + \
        OL.smoothness_loss(d64, im.double()) + R.nll(u64, 0.3 * gmap.double(), 'bayesian')
    assert R.close(got, o)
    _grads_ok(('parent',), (parent.grad.permute(0, 3, 1, 2),), torch.autograd.grad(o, (p64,)))


# ---------------------------------------------------- shifts leaving the image
@pytest.mark.parametrize('with_images', [False, True])
def test_consistency_out_of_range_shifts(with_images):
    """shifts up to 1.5 image widths: those taps read zeros and scatter nothing"""
    from train.loss import ConsistencyLoss
    N, H, W = 1, 40, 72
    g = torch.Generator().manual_seed(31)
    d = 0.02 + 1.48 * torch.rand(N, 2, H, W, generator=g)
    i = R.smooth((N, 2, H, W), g)
    dc, ic, dg, ig = _leaf64(d), _leaf64(i), _leaf(d), _leaf(i)
    if with_images:
        ref, got = OL.consistency_loss(dc, ic), ConsistencyLoss()(dg, ig)
        wc, wg = (dc, ic), (dg, ig)
    else:
        ref, got = OL.consistency_loss(dc), ConsistencyLoss()(dg)
        wc, wg = (dc,), (dg,)
    assert np.isfinite(float(got)) and R.close(got, ref)
    _grads_ok(('disp', 'images'), torch.autograd.grad(got, wg), torch.autograd.grad(ref, wc))


# -------------------------------------------- reconstruct: the image gradient
@pytest.mark.parametrize('sign', [-1.0, 1.0])
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('shape', [(2, 17, 70), (1, 40, 72)])
def test_reconstruct_image_gradient(shape, C, sign):
    from umamd import lossfn as LF
    N, H, W = shape
    g = torch.Generator().manual_seed(5 + C)
    d = 0.02 + 0.3 * torch.rand(N, 1, H, W, generator=g)
    img = R.smooth((N, C, H, W), g)
    up = torch.randn(N, C, H, W, generator=g)
    dc, ic, dg, ig = _leaf64(d), _leaf64(img), _leaf(d), _leaf(img)
    ref = OL.reconstruct(sign * dc, ic)
    got = LF.reconstruct(dg, ig, sign)
    assert R.rel_norm(got.detach(), ref.detach()) < 1e-5
    gg = torch.autograd.grad((got * up.to(DEV)).sum(), (dg, ig))
    gr = torch.autograd.grad((ref * up.double()).sum(), (dc, ic))
    _grads_ok(('disp', 'image'), gg, gr)
    # image only: every element is written (no stale memory where nothing lands)
    gi, = torch.autograd.grad((LF.reconstruct(dg.detach(), ig, sign) * up.to(DEV)).sum(), (ig,))
    assert R.rel_norm(gi, gr[1]) < GRAD_BAR


def test_warp_bwd_img_width_limit():
    """a C*W past the LDS limit is an error return naming it, before any launch"""
    from umamd import _lib as L
    lim = L.query('um_warp_bwd_img_max_cw')
    W = lim // 3 + 1
    gout = torch.zeros(1, 3, 1, W, device=DEV)
    disp = torch.zeros(1, 1, 1, W, device=DEV)
    gimg = torch.full((1, 3, 1, W), 7.0, device=DEV)
    with pytest.raises(L.UmamdError, match=str(lim)):
        L.call('um_warp_bwd_img', gout.data_ptr(), 1, 3, 1, W, disp.data_ptr(), W, 1, 1.0,
               gimg.data_ptr())
    assert float(gimg.min()) == 7.0  # nothing ran
    # W = 1024 with C = 3 is inside it
    W = 1024
    gout = torch.ones(1, 3, 2, W, device=DEV)
    disp = torch.zeros(1, 1, 2, W, device=DEV)
    gimg = torch.empty(1, 3, 2, W, device=DEV)
    L.call('um_warp_bwd_img', gout.data_ptr(), 1, 3, 2, W, disp.data_ptr(), 2 * W, 1, 1.0,
           gimg.data_ptr())
    ic = torch.zeros(1, 3, 2, W, dtype=torch.float64, requires_grad=True)
    OL.reconstruct(torch.zeros(1, 1, 2, W, dtype=torch.float64), ic).sum().backward()
    assert R.rel_norm(gimg, ic.grad) < 1e-5


# --------------------------------------------- TukraUncertaintyLoss: two routes
def _tukra_inputs(N=2, H=32, W=64):
    g = torch.Generator().manual_seed(41)
    imgs = torch.rand(N, 6, H, W, generator=g)
    preds = [0.02 + 0.2 * torch.rand(N, 4, H >> i, W >> i, generator=g) for i in range(4)]
    return imgs, preds


@pytest.mark.parametrize('pooling', [False, True])
@pytest.mark.parametrize('lt', R.LOSS_TYPES)
def test_tukra_composed_equals_fused(lt, pooling, monkeypatch):
    """clones of reconstruct_pyramid's outputs lose the tag and take the
    per-level loop over the modules; the tagged recon takes the fused kernels"""
    import train.utils as u
    from train.loss import TukraUncertaintyLoss
    imgs, preds = _tukra_inputs()
    cfg = loss_cfg(lt, 0.3, 0.5, pooling)
    pyr = u.scale_pyramid(imgs.to(DEV), 4)
    calls = _Calls(monkeypatch)
    out = []
    for composed in (False, True):
        lf = TukraUncertaintyLoss(**cfg)
        pd = [_leaf(p) for p in preds]
        rec = u.reconstruct_pyramid(pd, pyr)
        if composed:
            rec = [r.clone() for r in rec]
        del calls.names[:]
        dl, el = lf(pyr, pd, rec, 0, None)
        fwd = list(calls.names)
        (dl + 0.5 * el).backward()
        out.append((dl, el, lf.last_terms, [p.grad for p in pd], lf.wssim.previous_image_error))
        if composed:
            assert not any(n.startswith('um_loss') for n in calls.names)
            assert fwd.count('um_image_error_k') == 4
        else:
            fused = 'um_loss_pool' if pooling else 'um_loss'
            assert fwd == [fused + '_fwd'] and calls.names == [fused + '_fwd', fused + '_bwd']
    (dl0, el0, t0, g0, e0), (dl1, el1, t1, g1, e1) = out
    print(lt, pooling, float(dl0), float(dl1), float(el0), float(el1))
    assert R.close(dl1, dl0) and R.close(el1, el0, 1e-5)
    for k in range(6):
        assert R.close(t1[k], t0[k], 1e-5 if k in (1, 5) else 0.0), k
    assert float((e1.detach() - e0).abs().max()) < 1e-4
    _grads_ok([f'level {i}' for i in range(4)], g1, g0)


def test_tukra_blended_recon_vs_oracle():
    import train.utils as u
    from train.loss import TukraUncertaintyLoss
    imgs, preds = _tukra_inputs()
    cfg = loss_cfg('bayesian', 0.3, 0.5, False)
    pyr = u.scale_pyramid(imgs.to(DEV), 4)
    pd = [_leaf(p) for p in preds]
    rec = [0.7 * r + 0.3 * im.flip(0) for r, im in zip(u.reconstruct_pyramid(pd, pyr), pyr)]
    dl, el = TukraUncertaintyLoss(**cfg)(pyr, pd, rec, 0, None)
    pyc = OL.scale_pyramid(imgs.double(), 4)
    pc = [_leaf64(p) for p in preds]
    rc = [0.7 * r + 0.3 * im.flip(0) for r, im in zip(OL.reconstruct_pyramid(pc, pyc), pyc)]
    dlc, elc, _ = OL.total_loss(pyc, pc, rc, dict(cfg))
    print(float(dl), float(dlc), float(el), float(elc))
    assert R.close(dl, dlc) and R.close(el, elc, 1e-5)
    _grads_ok([f'level {i}' for i in range(4)], torch.autograd.grad(dl + 0.5 * el, pd),
              torch.autograd.grad(dlc + 0.5 * elc, pc))


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
def test_tagged_path_stays_fused_and_composed_meets_the_reference(lt, monkeypatch):
    """tests/golden/loss.npz (the reference's TukraUncertaintyLoss on its own
    reconstruct_pyramid): the tagged recon still runs um_loss_fwd / um_loss_bwd
    and meets the fixture through the existing bars; so does the composed
    path on clones of the same recon"""
    import train.utils as u
    import yaml
    from conftest import REPO
    from train.loss import TukraUncertaintyLoss
    z = np.load(os.path.join(GOLDEN, 'loss.npz'))
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)['loss']
    cfg['error_loss_config']['loss_type'] = lt
    pyr = u.scale_pyramid(torch.from_numpy(z['images']).to(DEV), 4)
    calls = _Calls(monkeypatch)
    for composed in (False, True):
        lf = TukraUncertaintyLoss(**cfg)
        pd = [_leaf(torch.from_numpy(z[f'rough_pred{i}'])) for i in range(4)]
        rec = u.reconstruct_pyramid(pd, pyr)
        if composed:
            rec = [r.clone() for r in rec]
        del calls.names[:]
        dl, el = lf(pyr, pd, rec, 0, None)
        if not composed:
            assert calls.names == ['um_loss_fwd']
        assert abs(float(dl) / float(z[f'rough_{lt}_disp_loss']) - 1) < 1e-4
        assert abs(float(el) / float(z[f'rough_{lt}_error_loss']) - 1) < 1e-4
        terms = lf.last_terms.cpu()
        for k, name in ((2, 'wssim'), (3, 'consistency'), (4, 'smoothness'), (5, 'error')):
            assert abs(float(terms[k]) / float(z[f'rough_{lt}_term_{name}']) - 1) < 1e-4, name
        gd = torch.autograd.grad(dl, pd, retain_graph=True)
        ge = torch.autograd.grad(el, pd)
        if not composed:
            assert set(calls.names) == {'um_loss_fwd', 'um_loss_bwd'}
        _grads_ok([f'gdisp{i}' for i in range(4)], gd, [z[f'rough_{lt}_gdisp{i}'] for i in range(4)])
        _grads_ok([f'gerr{i}' for i in range(4)], ge, [z[f'rough_{lt}_gerr{i}'] for i in range(4)])


# ------------------------------------------------------------------ guards --
def test_guards_raise_before_any_launch(monkeypatch):
    import train.utils as u
    from train import loss as TL
    from umamd import lossfn as LF
    calls = _Calls(monkeypatch)
    z = lambda *s: torch.rand(*s, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match='2x7'):
        TL.WeightedSSIMLoss()(z(1, 6, 2, 7), z(1, 6, 2, 7))
    with pytest.raises(ValueError, match='3x2'):
        TL.WeightedSSIMLoss(0.5, 0.02, 0.05).image_error(z(1, 6, 3, 2), z(1, 6, 3, 2))
    with pytest.raises(ValueError, match='1x9'):
        TL.ConsistencyLoss()(z(1, 2, 1, 9))
    with pytest.raises(ValueError, match='5x1'):
        TL.SmoothnessLoss()(z(1, 2, 5, 1), z(1, 6, 5, 1))
    with pytest.raises(ValueError, match='3x13'):
        TL.ReprojectionErrorLoss('l1', pooling=True)(z(1, 4, 3, 13), z(1, 6, 3, 13), z(1, 2, 3, 13))
    with pytest.raises(NotImplementedError, match='images'):
        TL.SmoothnessLoss()(z(1, 2, 4, 4), z(1, 6, 4, 4).requires_grad_(True))
    assert calls.names == []
    # a deferred (unwritten) recon is only ever filled by the fused path
    imgs, preds = _tukra_inputs(1)
    pyr = u.scale_pyramid(imgs.to(DEV), 4)
    pd = [p.to(DEV) for p in preds]
    with LF.deferred_recon():
        rec = u.reconstruct_pyramid(pd, pyr)
    lf = TL.TukraUncertaintyLoss()
    del calls.names[:]
    with pytest.raises(ValueError, match='deferred'):
        lf(pyr, [p.clone() for p in pd], rec, 0, None)
    mixed = [rec[0]] + u.reconstruct_pyramid(pd, pyr)[1:]
    with pytest.raises(ValueError, match='partly deferred'):
        lf(pyr, pd, mixed, 0, None)
