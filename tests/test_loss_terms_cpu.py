"""The standalone loss terms without a GPU: the f64 CPU oracle (composed in
_loss_terms_ref.py) against what the reference's own modules computed
(tests/golden/make_loss_terms_golden.py -> loss_terms.npz), at 1e-4 relative
for the values, 1e-4 absolute for the error map and 1e-4 rel-norm for every
gradient; and the construction surface of the drop-in modules.  CPU only."""
import pytest
import torch

import _loss_terms_ref as R
from oracle import loss as OL


def _t(z, k, grad=False):
    t = torch.from_numpy(z[k]).double()
    return t.requires_grad_(True) if grad else t


def _check(name, got, ref, grads=()):
    print(name, float(got), float(ref))
    assert R.close(got, ref, 1e-5), name
    for gname, g, gref in grads:
        e = R.rel_norm(g, gref)
        print(name, gname, e)
        assert e <= 1e-4, (name, gname, e)


@pytest.mark.parametrize('alpha,k1,k2', R.WSSIM_PARAMS)
def test_oracle_matches_reference_wssim(alpha, k1, k2):
    z = R.fixture()
    t = R.wtag(alpha, k1, k2)
    im, rc = _t(z, 'images', True), _t(z, 'recon', True)
    loss, emap = R.wssim(im, rc, alpha, k1, k2)
    gi, gr = torch.autograd.grad((emap * _t(z, 'gmap')).sum(), (im, rc))
    d = float((emap.detach() - _t(z, f'{t}_map')).abs().max())
    print(t, 'map', d)
    assert d <= 1e-4
    _check(t, loss, z[f'{t}_loss'], (('gimg', gi, z[f'{t}_gimg']), ('grec', gr, z[f'{t}_grec'])))


def test_constants_matter_on_the_fixture():
    """(k1, k2) = (0.02, 0.05) against the defaults at equal alpha: a path
    that ignores the constants misses the 1e-4 bar by orders of magnitude"""
    z = R.fixture()
    a, _ = R.wssim(_t(z, 'images'), _t(z, 'recon'), 0.5, 0.01, 0.03)
    b, _ = R.wssim(_t(z, 'images'), _t(z, 'recon'), 0.5, 0.02, 0.05)
    print(float(a), float(b))
    assert abs(float(a) - float(b)) > 1e-2 * abs(float(b))


def test_oracle_matches_reference_consistency():
    z = R.fixture()
    d = _t(z, 'pred')[:, 0:2].clone().requires_grad_(True)
    loss = OL.consistency_loss(d)
    _check('cons_self', loss, z['cons_self_loss'],
           (('gdisp', torch.autograd.grad(loss, d)[0], z['cons_self_gdisp']),))
    d = _t(z, 'pred')[:, 2:4].clone().requires_grad_(True)
    im = _t(z, 'pred')[:, 0:2].clone().requires_grad_(True)
    loss = OL.consistency_loss(d, im)
    gd, gi = torch.autograd.grad(loss, (d, im))
    _check('cons_img', loss, z['cons_img_loss'],
           (('gdisp', gd, z['cons_img_gdisp']), ('gimg', gi, z['cons_img_gimg'])))


def test_oracle_matches_reference_smoothness():
    z = R.fixture()
    d = _t(z, 'pred')[:, 0:2].clone().requires_grad_(True)
    loss = OL.smoothness_loss(d, _t(z, 'images'))
    _check('smooth', loss, z['smooth_loss'],
           (('gdisp', torch.autograd.grad(loss, d)[0], z['smooth_gdisp']),))


@pytest.mark.parametrize('pooling', [False, True])
@pytest.mark.parametrize('lt', R.LOSS_TYPES)
def test_oracle_matches_reference_error_loss(lt, pooling):
    z = R.fixture()
    p = _t(z, 'pred', True)
    err = _t(z, R.wtag(0.85, 0.01, 0.03) + '_map')  # the map the reference fed its error term
    loss = OL.error_loss(p, _t(z, 'images'), err, lt, 0.3, 0.5, pooling)
    t = f'err_{lt}_p{int(pooling)}'
    _check(t, loss, z[f'{t}_loss'],
           (('gpred', torch.autograd.grad(loss, p)[0], z[f'{t}_gpred']),))


def test_oracle_matches_reference_tukra_blended():
    import yaml
    import os
    from conftest import REPO
    z = R.fixture()
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)['loss']
    cfg['error_loss_config']['loss_type'] = 'bayesian'
    pyr = [_t(z, 'images'), _t(z, 'images1')]
    ps = [_t(z, 'pred', True), _t(z, 'pred1', True)]
    dl, el, _ = OL.total_loss(pyr, ps, [_t(z, 'recon'), _t(z, 'recon1')], cfg)
    g = torch.autograd.grad(dl + el, ps)
    _check('tukra disp', dl, z['tukra_disp'])
    _check('tukra error', el, z['tukra_error'],
           (('gpred0', g[0], z['tukra_gpred0']), ('gpred1', g[1], z['tukra_gpred1'])))


def test_nll_helper_is_the_error_loss_without_weights():
    z = R.fixture()
    p = _t(z, 'pred')
    err = OL.image_error(_t(z, 'images'), _t(z, 'recon'))
    for lt in R.LOSS_TYPES:
        assert float(R.nll(p[:, 2:4], err, lt)) == \
            float(OL.error_loss(p, _t(z, 'images'), err, lt, 0.0, 0.0, False))


def test_wssim_holds_any_constants():
    from train.loss import WeightedSSIMLoss
    m = WeightedSSIMLoss(0.5, 0.02, 0.05)
    assert m.alpha == 0.5
    assert m.k1 == pytest.approx(4e-4, rel=1e-12) and m.k2 == pytest.approx(2.5e-3, rel=1e-12)
    d = WeightedSSIMLoss()
    assert (d.alpha, d.k1, d.k2) == (0.85, 0.01 ** 2, 0.03 ** 2)
    assert d.previous_image_error is None


def test_submodules_have_their_own_forward():
    """no sub-loss derives from a class whose forward raises: each defines
    forward itself, and the reference's helper methods exist"""
    import torch.nn as nn
    from train import loss as TL
    for cls in (TL.WeightedSSIMLoss, TL.ConsistencyLoss, TL.SmoothnessLoss,
                TL.ReprojectionErrorLoss):
        assert 'forward' in vars(cls), cls
        assert cls.__mro__[1] is nn.Module, cls.__mro__
    assert not hasattr(TL, '_FusedOnly')
    for name in ('ssim', 'dssim', 'l1_error', 'image_error'):
        assert callable(getattr(TL.WeightedSSIMLoss, name))
    assert callable(TL.ReprojectionErrorLoss('bayesian').loss_function)


def test_torch_composed_ssim_helpers_match_oracle():
    """ssim / dssim / l1_error are torch ops: they run anywhere, with the
    reference's shapes ([N,C,H-2,W-2])"""
    from train.loss import WeightedSSIMLoss
    im, rc, _, _ = R.inputs(2, 17, 70)
    m = WeightedSSIMLoss(0.5, 0.02, 0.05)
    x, y = im[:, 0:3].double(), rc[:, 0:3].double()
    assert tuple(m.ssim(x, y).shape) == (2, 3, 15, 68)
    assert torch.allclose(m.dssim(x, y), OL.dssim(x, y, 0.02 ** 2, 0.05 ** 2), rtol=0, atol=1e-12)
    assert torch.equal(m.l1_error(x, y), (x - y).abs())


def test_terms_refuse_cpu_tensors():
    from train import loss as TL
    from umamd._lib import UmamdError
    im, rc, pred, _ = R.inputs(1, 4, 5)
    with pytest.raises(UmamdError):
        TL.WeightedSSIMLoss()(im, rc)
    with pytest.raises(UmamdError):
        TL.WeightedSSIMLoss(0.5, 0.02, 0.05).image_error(im, rc)
    with pytest.raises(UmamdError):
        TL.ConsistencyLoss()(pred[:, 0:2])
    with pytest.raises(UmamdError):
        TL.SmoothnessLoss()(pred[:, 0:2], im)
    with pytest.raises(UmamdError):
        TL.ReprojectionErrorLoss('l1')(pred, im, torch.rand(1, 2, 4, 5))


def test_size_guards_need_no_device():
    from train import loss as TL
    with pytest.raises(ValueError, match='2x5'):
        TL.WeightedSSIMLoss()(torch.rand(1, 6, 2, 5), torch.rand(1, 6, 2, 5))
    with pytest.raises(ValueError, match='1x4'):
        TL.ConsistencyLoss()(torch.rand(1, 2, 1, 4))
    with pytest.raises(ValueError, match='3x1'):
        TL.SmoothnessLoss()(torch.rand(1, 2, 3, 1), torch.rand(1, 6, 3, 1))
    with pytest.raises(ValueError, match='3x9'):
        TL.ReprojectionErrorLoss('l1', pooling=True)(torch.rand(1, 4, 3, 9), torch.rand(1, 6, 3, 9),
                                                     torch.rand(1, 2, 3, 9))
    with pytest.raises(NotImplementedError, match='images'):
        TL.SmoothnessLoss()(torch.rand(1, 2, 4, 4), torch.rand(1, 6, 4, 4).requires_grad_(True))


def test_workspace_and_limit_queries():
    from umamd._lib import query
    assert query('um_warp_bwd_img_max_cw') == 16384 >= 3 * 1024
    # one f64 partial per workgroup: at least the elementwise cap, and every tile
    assert query('um_lossterm_ws', 1, 3, 3) == 8 * 1024
    assert query('um_lossterm_ws', 16, 256, 512) == 8 * 16 * 16 * 8
