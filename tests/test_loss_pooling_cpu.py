"""ReprojectionErrorLoss(pooling=True) without a GPU: the CPU oracle against
the fixture the reference computed (tests/golden/make_loss_pooling_golden.py)
and the drop-in modules' construction.  CPU only."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import loss as OL

LOSS_TYPES = ('l1', 'bayesian', 'log_bayesian')
WEIGHTS = ((0.0, 0.5), (0.3, 0.5), (0.3, 0.0))  # (esw, ecw) of the fixture


def tag(lt, esw, ecw):
    return f'{lt}_s{esw:g}_c{ecw:g}'


def loss_cfg(lt, esw, ecw, pooling=True):
    return {'wssim_weight': 1.0, 'consistency_weight': 1.0, 'smoothness_weight': 1.0,
            'adversarial_weight': 0.85, 'perceptual_weight': 0.05, 'predictive_error_weight': 1.0,
            'wssim_alpha': 0.85, 'perceptual_start': 5, 'adversarial_loss_type': 'mse',
            'error_loss_config': {'loss_type': lt, 'smoothness_weight': esw,
                                  'consistency_weight': ecw, 'pooling': pooling}}


def fixture():
    return np.load(os.path.join(GOLDEN, 'loss_pooling.npz'))


def rel_norm(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_fixture_matches_the_config_defaults():
    """the fixture was generated from config.yml's loss weights: the ones
    loss_cfg() writes out"""
    import yaml
    from conftest import REPO
    with open(os.path.join(REPO, 'config.yml')) as f:
        c = yaml.safe_load(f)['loss']
    want = loss_cfg('l1', 0.0, 0.5)
    for k in want:
        if k != 'error_loss_config':
            assert c[k] == want[k], k
    assert 'pooling' in c['error_loss_config']


@pytest.mark.parametrize('esw,ecw', WEIGHTS)
@pytest.mark.parametrize('lt', LOSS_TYPES)
def test_oracle_matches_reference_pooling(lt, esw, ecw):
    z = fixture()
    t = tag(lt, esw, ecw)
    pyr = OL.scale_pyramid(torch.from_numpy(z['images']), 4)
    preds = [torch.from_numpy(z[f'pred{i}']).clone().requires_grad_(True) for i in range(4)]
    dl, el, _ = OL.total_loss(pyr, preds, OL.reconstruct_pyramid(preds, pyr),
                              loss_cfg(lt, esw, ecw))
    for got, key in ((dl, 'disp_loss'), (el, 'error_loss')):
        ref = float(z[f'{t}_{key}'])
        print(t, key, float(got), ref)
        assert abs(float(got) - ref) <= 1e-4 * abs(ref) + 1e-5
    gd = torch.autograd.grad(dl, preds, retain_graph=True)
    ge = torch.autograd.grad(el, preds)
    for i in range(4):
        ed, ee = rel_norm(gd[i], z[f'gdisp{i}']), rel_norm(ge[i], z[f'{t}_gerr{i}'])
        print(t, i, ed, ee)
        assert ed <= 1e-4 and ee <= 1e-4
    # pooling is not a no-op on these inputs
    _, el0, _ = OL.total_loss(pyr, preds, OL.reconstruct_pyramid(preds, pyr),
                              loss_cfg(lt, esw, ecw, pooling=False))
    assert abs(float(el0) - float(el)) > 1e-2 * abs(float(el))


def test_pooling_constructs():
    import torch.nn as nn
    from train.loss import ReprojectionErrorLoss, TukraUncertaintyLoss
    lf = TukraUncertaintyLoss(error_loss_config={'pooling': True, 'loss_type': 'bayesian',
                                                 'smoothness_weight': 0.0,
                                                 'consistency_weight': 0.5})
    pool = lf.predictive_error.pool
    assert isinstance(pool, nn.AvgPool2d)
    assert (pool.kernel_size, pool.stride, pool.padding) == (3, 1, 0)
    assert lf._cfg()['pool'] is True
    off = TukraUncertaintyLoss(error_loss_config={'pooling': False})
    assert isinstance(off.predictive_error.pool, nn.Identity)
    assert off._cfg()['pool'] is False
    assert isinstance(ReprojectionErrorLoss().pool, nn.Identity)


def test_pooling_config_file_surface():
    """TukraUncertaintyLoss(**config['loss']) with the flag turned on, as a
    user's config.yml would"""
    import yaml
    from conftest import REPO
    from train.loss import TukraUncertaintyLoss
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)['loss']
    cfg['error_loss_config']['pooling'] = True
    assert TukraUncertaintyLoss(**cfg)._cfg()['pool'] is True


def test_pool_workspace_query():
    """um_loss_pool_ws is a host query: 0 for a geometry the pooled stage
    refuses (a level below 4x4), growing with the batch otherwise"""
    from umamd._lib import query
    assert query('um_loss_pool_ws', 4, 1, 24, 104) == 0  # coarsest level 3x13
    assert query('um_loss_pool_ws', 7, 1, 256, 512) == 0
    a, b = query('um_loss_pool_ws', 4, 1, 32, 64), query('um_loss_pool_ws', 4, 2, 32, 64)
    assert 0 < a < b
    # every pooled cell of every level: float4 + float2 + 6 floats + int4 = 64 bytes
    cells = sum((32 // 2 ** i - 2) * (64 // 2 ** i - 2) for i in range(4))
    assert a >= 64 * cells and a % 16 == 0
