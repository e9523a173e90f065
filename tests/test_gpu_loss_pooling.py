"""ReprojectionErrorLoss(pooling=True) on the HIP path (um_loss_pool_fwd /
um_loss_pool_bwd) against the f64 CPU oracle and the reference's fixture
(tests/golden/loss_pooling.npz): ragged shapes down to a 2x11 pooled grid,
shifts that leave the image, the size guard, the untouched pooling=False
path, the fused forward against the plain one, and the captured steps.

Bars are the fused loss's existing ones (test_gpu_loss_stack.py): loss
scalars within 1e-4 relative (error_loss with a 1e-5 floor: the bayesian NLL
can cancel to near zero), the gradient of dl + 0.5 el within 4e-3 rel-norm
per level (warp cell flips).  On these inputs error_loss with and
without pooling differs by 9-88 % and the per-level gradients by >= 3 %, so
a path that ignores the flag fails both.  Marked gpu."""
import numpy as np
import pytest
import torch

from oracle import loss as OL
from test_gpu_loss_stack import _smooth_preds
from test_loss_pooling_cpu import LOSS_TYPES, WEIGHTS, fixture, loss_cfg, rel_norm, tag

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(2, 64, 128), (1, 40, 72), (2, 32, 200), (3, 32, 104)]
CONFIGS = [(lt, esw, ecw) for lt in LOSS_TYPES for esw, ecw in ((0.3, 0.5), (0.0, 0.5))] + \
    [('l1', 0.3, 0.0)]


def _close(got, ref, floor=0.0):
    return abs(float(got) - float(ref)) <= 1e-4 * abs(float(ref)) + floor


def _hip(imgs, preds, cfg):
    """(lf, dl, el, prediction leaves) of the HIP loss under deferred_recon"""
    import train.utils as u
    from train.loss import TukraUncertaintyLoss
    from umamd import lossfn as LF
    lf = TukraUncertaintyLoss(**cfg)
    pyr = u.scale_pyramid(imgs.to(DEV), 4)
    pd = [p.to(DEV).requires_grad_(True) for p in preds]
    with LF.deferred_recon():
        rec = u.reconstruct_pyramid(pd, pyr)
    dl, el = lf(pyr, pd, rec, 0, None)
    return lf, dl, el, pd


def _oracle(imgs, preds, cfg):
    pyr = OL.scale_pyramid(imgs.double(), 4)
    pc = [p.double().requires_grad_(True) for p in preds]
    dl, el, _ = OL.total_loss(pyr, pc, OL.reconstruct_pyramid(pc, pyr), dict(cfg))
    return dl, el, pc


def _check_against_oracle(imgs, preds, cfg, what):
    lf, dl, el, pd = _hip(imgs, preds, cfg)
    dlc, elc, pc = _oracle(imgs, preds, cfg)
    print(what, 'disp', float(dl), float(dlc), 'error', float(el), float(elc))
    (dl + 0.5 * el).backward()
    (dlc + 0.5 * elc).backward()
    errs = [rel_norm(pd[i].grad.cpu(), pc[i].grad) for i in range(4)]
    print(what, 'grad rel-norm per level', errs)
    assert _close(dl, dlc) and _close(el, elc, 1e-5)
    for i in range(4):
        assert torch.isfinite(pd[i].grad).all()
        assert errs[i] < 4e-3, (i, errs[i])
    return lf


@pytest.mark.parametrize('lt,esw,ecw', CONFIGS)
@pytest.mark.parametrize('kind', ['uniform', 'smooth_noisy'])
@pytest.mark.parametrize('shape', SHAPES)
def test_pooling_vs_oracle_ragged(shape, kind, lt, esw, ecw):
    """forward and backward on shapes whose coarsest levels (8x16, 5x9, 4x25,
    4x13) give pooled grids down to 2x11, with partial tiles and strips"""
    N, H, W = shape
    g = torch.Generator().manual_seed(11)
    imgs = torch.rand(N, 6, H, W, generator=g)
    if kind == 'uniform':
        preds = [0.02 + 0.2 * torch.rand(N, 4, H >> i, W >> i, generator=g) for i in range(4)]
    else:
        preds = _smooth_preds(N, H, W, 12, noisy_right=True)
    lf = _check_against_oracle(imgs, preds, loss_cfg(lt, esw, ecw), (shape, kind, lt, esw, ecw))
    # previous_image_error stays the unpooled last-level map
    assert tuple(lf.wssim.previous_image_error.shape) == (N, 2, H >> 3, W >> 3)
    pyr = OL.scale_pyramid(imgs.double(), 4)
    pc = [p.double() for p in preds]
    e3 = OL.image_error(pyr[3], OL.reconstruct_pyramid(pc, pyr)[3], 0.85)
    # f32 against f64: the variances cancel to ~1e-7 absolute and sit over
    # denominators >= C2 = 9e-4, so ~1e-4 on a map of values in [0, 1] (the
    # pooled map differs from it by far more)
    assert float((lf.wssim.previous_image_error.double().cpu() - e3).abs().max()) < 1e-4
    # terms: out[1] / out[5] the pooled term, weight 1
    assert float(lf.last_terms[1]) == float(lf.last_terms[5])


@pytest.mark.parametrize('esw,ecw', WEIGHTS)
@pytest.mark.parametrize('lt', LOSS_TYPES)
def test_pooling_vs_reference_fixture(lt, esw, ecw):
    """values and both gradient sets at 2x32x64 (last level pooled to 2x6)
    against what the reference computed"""
    z = fixture()
    t = tag(lt, esw, ecw)
    imgs = torch.from_numpy(z['images'])
    preds = [torch.from_numpy(z[f'pred{i}']) for i in range(4)]
    _, dl, el, pd = _hip(imgs, preds, loss_cfg(lt, esw, ecw))
    print(t, 'disp', float(dl), float(z[f'{t}_disp_loss']), 'error', float(el),
          float(z[f'{t}_error_loss']))
    gd = torch.autograd.grad(dl, pd, retain_graph=True)
    ge = torch.autograd.grad(el, pd)
    ed = [rel_norm(gd[i].cpu(), z[f'gdisp{i}']) for i in range(4)]
    ee = [rel_norm(ge[i].cpu(), z[f'{t}_gerr{i}']) for i in range(4)]
    print(t, 'gdisp', ed, 'gerr', ee)
    assert _close(dl, z[f'{t}_disp_loss']) and _close(el, z[f'{t}_error_loss'], 1e-5)
    assert max(ed) < 4e-3 and max(ee) < 4e-3


@pytest.mark.parametrize('lt', ['l1', 'log_bayesian'])
def test_out_of_range_shifts(lt):
    """uncertainties up to 1.5: the consistency's sample row leaves the
    pooled image altogether; those taps read zeros (and scatter nothing)"""
    N, H, W = 1, 40, 72
    g = torch.Generator().manual_seed(31)
    imgs = torch.rand(N, 6, H, W, generator=g)
    preds = []
    for i in range(4):
        p = 0.02 + 0.2 * torch.rand(N, 4, H >> i, W >> i, generator=g)
        p[:, 2:] = 0.02 + 1.48 * torch.rand(N, 2, H >> i, W >> i, generator=g)
        preds.append(p)
    _check_against_oracle(imgs, preds, loss_cfg(lt, 0.3, 0.5), ('far', lt))


class _Calls:
    """the entry names that umamd.lossfn passes to _lib.call"""

    def __init__(self, monkeypatch):
        from umamd import _lib, lossfn
        self.names = []

        def call(name, *a, **k):
            if name != 'um_pyramid':  # the test's own image pyramid
                self.names.append(name)
            return _lib.call(name, *a, **k)
        monkeypatch.setattr(lossfn, 'call', call)


def test_size_guard(monkeypatch):
    """a level whose pooled grid would be below 2x2 raises before any launch"""
    N, H, W = 1, 24, 104  # coarsest level 3x13
    g = torch.Generator().manual_seed(5)
    imgs = torch.rand(N, 6, H, W, generator=g)
    preds = [0.02 + 0.2 * torch.rand(N, 4, H >> i, W >> i, generator=g) for i in range(4)]
    import train.utils as u
    from train.loss import TukraUncertaintyLoss
    from umamd import lossfn as LF
    lf = TukraUncertaintyLoss(**loss_cfg('l1', 0.3, 0.5))
    pyr = u.scale_pyramid(imgs.to(DEV), 4)
    pd = [p.to(DEV).requires_grad_(True) for p in preds]
    with LF.deferred_recon():
        rec = u.reconstruct_pyramid(pd, pyr)
    calls = _Calls(monkeypatch)
    with pytest.raises(ValueError, match=r'level 3 is 3x13'):
        lf(pyr, pd, rec, 0, None)
    assert calls.names == []
    # the same shape without pooling is served (test_gpu_loss_stack runs it)
    lf0 = TukraUncertaintyLoss(**loss_cfg('l1', 0.3, 0.5, pooling=False))
    lf0(pyr, pd, rec, 0, None)
    assert calls.names == ['um_loss_fwd']


def test_pooling_false_path_untouched(monkeypatch):
    N, H, W = 2, 64, 128
    g = torch.Generator().manual_seed(6)
    imgs = torch.rand(N, 6, H, W, generator=g)
    preds = [0.02 + 0.2 * torch.rand(N, 4, H >> i, W >> i, generator=g) for i in range(4)]
    calls = _Calls(monkeypatch)
    _, dl, el, pd = _hip(imgs, preds, loss_cfg('bayesian', 0.3, 0.5, pooling=False))
    (dl + el).backward()
    assert calls.names == ['um_loss_fwd', 'um_loss_bwd']
    del calls.names[:]
    _, dl, el, pd = _hip(imgs, preds, loss_cfg('bayesian', 0.3, 0.5))
    (dl + el).backward()
    # one forward entry, one backward entry; the error maps come from the
    # loss's own tile pass, not from um_image_error
    assert calls.names == ['um_loss_pool_fwd', 'um_loss_pool_bwd']


@pytest.mark.parametrize('lt', LOSS_TYPES)
def test_fused_matches_plain(lt):
    """the forward with gradient partials + the short backward against the
    no-grad forward + the full backward (a second backward through the same
    graph has no partials left), and linearity in the upstream scalars"""
    import train.utils as u
    N, H, W = 2, 64, 128
    g = torch.Generator().manual_seed(21)
    imgs = torch.rand(N, 6, H, W, generator=g)
    preds = _smooth_preds(N, H, W, 22, noisy_right=True)
    lf, dl, el, pd = _hip(imgs, preds, loss_cfg(lt, 0.3, 0.5))
    terms = lf.last_terms.clone()
    g_fused = torch.autograd.grad(dl + 0.5 * el, pd, retain_graph=True)
    g_plain = torch.autograd.grad(dl + 0.5 * el, pd, retain_graph=True)
    g_one = torch.autograd.grad(dl + el, pd, retain_graph=True)
    g_two = torch.autograd.grad(2.0 * dl + 2.0 * el, pd)
    with torch.no_grad():
        pyr = u.scale_pyramid(imgs.to(DEV), 4)
        pdd = [p.detach() for p in pd]
        dl0, el0 = lf(pyr, pdd, u.reconstruct_pyramid(pdd, pyr), 0, None)
    assert abs(float(dl) / float(dl0) - 1) < 1e-6
    assert abs(float(el) / float(el0) - 1) < 1e-6
    assert float((terms - lf.last_terms).abs().max() / lf.last_terms.abs().max()) < 1e-6

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    for a, b in zip(g_fused, g_plain):
        assert torch.isfinite(a).all()
        assert rel(a, b) < 1e-5
    for a, b in zip(g_one, g_two):
        assert rel(2.0 * a, b) < 1e-6


def _pool_model_cfg():
    from test_gpu_model import _cfg
    cfg = _cfg()
    cfg['loss']['error_loss_config'] = {'loss_type': 'l1', 'smoothness_weight': 0.3,
                                        'consistency_weight': 0.5, 'pooling': True}
    return cfg


def test_captured_step_matches_eager_pooling():
    """test_gpu_graph.test_captured_step_matches_eager's procedure and bars
    with pooling=True (B=2, 64x128, fp32)"""
    from test_gpu_graph import _adam_clone
    from test_gpu_model import _model, _uniform_pair
    from train.graph import CapturedTrainStep
    from train.loss import TukraUncertaintyLoss
    from train.train import train_step
    from umamd.optim import Adam
    cfg = _pool_model_cfg()
    left, right = _uniform_pair(2, 64, 128)
    left, right = left.to(DEV), right.to(DEV)
    lf = TukraUncertaintyLoss(**cfg['loss'])
    assert lf._cfg()['pool'] is True
    m_g = _model(cfg).train()
    opt_g = Adam(m_g.parameters(), 1e-4)
    cap = CapturedTrainStep(m_g, lf, opt_g, left, right, 0.3, warmup=2)
    for _ in range(2):
        cap()
    torch.cuda.synchronize()
    m_e = _model(cfg).train()
    m_e.load_state_dict(m_g.state_dict())
    opt_e = _adam_clone(opt_g, m_g, m_e)
    dl_e, el_e, _ = train_step(m_e, left, right, lf, opt_e, 0.3)
    dl_g, el_g = cap()
    torch.cuda.synchronize()
    for a, b in ((float(dl_e), float(dl_g)), (float(el_e), float(el_g))):
        print('eager', a, 'captured', b)
        assert abs(a - b) <= 1e-5 * abs(a) + 1e-7, (a, b)
    assert int(opt_g._dev[0]['step']) == int(opt_e._dev[0]['step']) == 3
    se, sg = m_e.state_dict(), m_g.state_dict()
    pnames = {k for k, _ in m_e.named_parameters()}
    for k in se:
        if k in pnames:
            d = float((se[k] - sg[k]).abs().max())
            assert d <= 6e-4, (k, d)
        elif se[k].is_floating_point():
            d = float((se[k] - sg[k]).abs().max())
            assert d <= 1e-4 * (float(se[k].abs().max()) + 1.0), (k, d)
        else:
            assert torch.equal(se[k], sg[k]), k


def test_captured_adversarial_step_pooling():
    """one adversarial captured step with the flag on runs and returns three
    finite losses"""
    from copy import deepcopy
    from test_gpu_adversarial import _disc, _pyr, _z
    from test_gpu_model import _model
    from train.graph import CapturedTrainStep
    from train.loss import TukraUncertaintyLoss
    from umamd.optim import Adam
    z = _z()
    cfg = _pool_model_cfg()
    m = _model(cfg).train()
    d = _disc(z, 'fp32')
    left, right, _ = _pyr(z)
    cap = CapturedTrainStep(m, TukraUncertaintyLoss(**cfg['loss']), Adam(m.parameters(), 1e-4),
                            left, right, 0.3, warmup=1, disc=d,
                            disc_optimiser=Adam(d.parameters(), 1e-4),
                            disc_loss_function=torch.nn.BCELoss(), disc_clone=deepcopy(d),
                            batch_size=2)
    out = cap(left, right, perceptual=True)
    torch.cuda.synchronize()
    assert len(out) == 3
    assert all(np.isfinite(float(t)) for t in out)
