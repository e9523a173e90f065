"""The adversarial training step as HIP graphs (train.graph.CapturedTrainStep
with a discriminator, train.train._GraphSteps) against the eager step
(train.train.train_step) and the reference goldens (adversarial.npz).

B=2, 64x128, the nodes_5_seed_42 graphs, formula weights.  As in
test_gpu_graph.py the comparison is per step from a shared state: captured
and eager differ by float-atomic summation order, which Adam turns into sign
noise on near-zero gradients.  Marked gpu."""
from copy import deepcopy

import numpy as np
import pytest
import torch

from test_gpu_adversarial import _disc, _pyr, _z
from test_gpu_graph import _adam_clone
from test_gpu_model import DEV, _cfg, _model

pytestmark = pytest.mark.gpu


def _setup(dtype='fp32', loss_type='l1', perceptual_start=None, warmup=2, capture=True):
    """model, discriminator, clone, loss, both Adams, inputs and (optionally)
    the captured step"""
    from train.graph import CapturedTrainStep
    from train.loss import TukraUncertaintyLoss
    from umamd.optim import Adam
    z = _z()
    cfg = _cfg()
    cfg['loss']['error_loss_config']['loss_type'] = loss_type
    if perceptual_start is not None:
        cfg['loss']['perceptual_start'] = perceptual_start
    s = {'z': z, 'cfg': cfg, 'dtype': dtype}
    s['m'] = _model(cfg, dtype).train()
    s['d'] = _disc(z, dtype)
    s['clone'] = deepcopy(s['d'])
    s['lf'] = TukraUncertaintyLoss(**cfg['loss'])
    s['dlf'] = torch.nn.BCELoss()
    s['opt'], s['dopt'] = Adam(s['m'].parameters(), 1e-4), Adam(s['d'].parameters(), 1e-4)
    s['left'], s['right'], _ = _pyr(z)
    if capture:
        s['cap'] = CapturedTrainStep(s['m'], s['lf'], s['opt'], s['left'], s['right'], 0.3,
                                     warmup=warmup, disc=s['d'], disc_optimiser=s['dopt'],
                                     disc_loss_function=s['dlf'], disc_clone=s['clone'],
                                     batch_size=2)
    return s


def _eager_copy(s):
    """fresh model / discriminator / clone / Adams holding a copy of s's state"""
    m = _model(s['cfg'], s['dtype']).train()
    m.load_state_dict(s['m'].state_dict())
    d = _disc(s['z'], s['dtype'])
    d.load_state_dict(s['d'].state_dict())
    clone = _disc(s['z'], s['dtype'])
    clone.load_state_dict(s['clone'].state_dict())
    return m, d, clone, _adam_clone(s['opt'], s['m'], m), _adam_clone(s['dopt'], s['d'], d)


def _compare_step(s, perceptual):
    """one eager train_step from a copy of s's state against one replay:
    the bars of test_gpu_graph.test_captured_step_matches_eager"""
    from train.train import train_step
    lf = s['lf']
    m, d, clone, opt, dopt = _eager_copy(s)
    before = int(s['opt']._dev[0]['step'])
    index = lf.perceptual_start if perceptual else lf.perceptual_start - 1
    assert index >= 0
    eager = train_step(m, s['left'], s['right'], lf, opt, 0.3, 4, index, d, clone, dopt,
                       s['dlf'], batch_size=2)
    graph = s['cap'](s['left'], s['right'], perceptual=perceptual)
    torch.cuda.synchronize()
    assert len(graph) == 3
    for name, a, b in zip(('disp', 'error', 'disc'), map(float, eager), map(float, graph)):
        print(f'{name} loss: eager {a!r} captured {b!r}')
        assert abs(a - b) <= 1e-5 * abs(a) + 1e-7, (name, a, b)
    for og, oe in ((s['opt'], opt), (s['dopt'], dopt)):
        assert int(og._dev[0]['step']) == int(oe._dev[0]['step']) == before + 1
    for net_e, net_g in ((m, s['m']), (d, s['d'])):
        se, sg = net_e.state_dict(), net_g.state_dict()
        pnames = {k for k, _ in net_e.named_parameters()}
        for k in se:
            if k in pnames:  # one Adam step from equal state, sign noise: 6 lr
                diff = float((se[k] - sg[k]).abs().max())
                assert diff <= 6e-4, (k, diff)
            elif se[k].is_floating_point():  # running stats: same forward
                diff = float((se[k] - sg[k]).abs().max())
                assert diff <= 1e-4 * (float(se[k].abs().max()) + 1.0), (k, diff)
            else:
                assert torch.equal(se[k], sg[k]), k


@pytest.mark.parametrize('perceptual', [False, True])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_captured_adversarial_step_matches_eager(dtype, perceptual):
    s = _setup(dtype)
    for _ in range(2):
        out = s['cap'](perceptual=perceptual)
    assert all(not t.requires_grad and t.dim() == 0 for t in out)
    torch.cuda.synchronize()
    assert int(s['opt']._dev[0]['step']) == int(s['dopt']._dev[0]['step']) == 2
    _compare_step(s, perceptual)


def test_perceptual_gate():
    """perceptual=False replays the step of a batch index below
    perceptual_start (the term contributes exact zeros), and the device
    gate follows the argument"""
    s = _setup('fp32')
    cap = s['cap']
    _compare_step(s, False)
    assert float(cap._gate) == 0.0
    with_term = [float(t) for t in cap(perceptual=True)]
    assert float(cap._gate) == 1.0
    cap(perceptual=False)
    assert float(cap._gate) == 0.0
    assert all(np.isfinite(with_term))


def test_captured_adversarial_step_matches_reference():
    """test_gpu_adversarial.test_adversarial_train_steps (bayesian,
    perceptual_start 1, lr 1e-4, BCELoss) through the captured step, with
    that test's bars: 1e-3 on the first step; 0.1 on the second, which
    follows one Adam step of an ill-conditioned bayesian NLL (see there)."""
    s = _setup('fp32', 'bayesian', perceptual_start=1)
    z = s['z']
    for i in range(2):
        got = [float(t) for t in s['cap'](s['left'], s['right'], perceptual=i >= 1)]
        if i % 10 == 0:
            s['clone'].load_state_dict(s['d'].state_dict())
        ref = [float(z[f'step_disp_{i}']), float(z[f'step_err_{i}']), float(z[f'step_disc_{i}'])]
        rel = [abs(a / b - 1) for a, b in zip(got, ref)]
        print(f'captured adversarial step {i}: got {got} ref {ref} rel {rel}')
        assert all(r < (1e-3 if i == 0 else 0.1) for r in rel), (i, got, ref)


def test_capture_restores_all_state():
    """the warm-up steps are undone: model, discriminator and clone are
    bit-equal to their state before construction, both Adams are at step 0
    with zero moments"""
    s = _setup('fp32', capture=False)
    from train.graph import CapturedTrainStep
    init = {n: {k: v.clone() for k, v in s[n].state_dict().items()}
            for n in ('m', 'd', 'clone')}
    CapturedTrainStep(s['m'], s['lf'], s['opt'], s['left'], s['right'], 0.3, warmup=2,
                      disc=s['d'], disc_optimiser=s['dopt'], disc_loss_function=s['dlf'],
                      disc_clone=s['clone'], batch_size=2)
    for n, sd in init.items():
        now = s[n].state_dict()
        assert list(now) == list(sd)
        for k, v in sd.items():
            assert torch.equal(now[k], v), (n, k)
    for opt in (s['opt'], s['dopt']):
        assert int(opt._dev[0]['step']) == 0
        assert opt.state and all(float(st[k].abs().max()) == 0 for st in opt.state.values()
                                 for k in ('exp_avg', 'exp_avg_sq'))


def test_clone_gradients_do_not_accumulate():
    """the clone is frozen: after three replays none of its parameters has a
    .grad, and the discriminator's own gradients exist"""
    s = _setup('fp32')
    for i in range(3):
        s['cap'](perceptual=i > 0)
    torch.cuda.synchronize()
    assert all(not p.requires_grad and p.grad is None for p in s['clone'].parameters())
    for k, p in s['d'].named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


class _Loader:
    """three full batches of 2 and a ragged one of 1 (seeded uniform);
    ``on_ragged`` runs when the loop asks for the ragged batch, i.e. after
    batch 2's step and clone refresh"""
    batch_size = 2

    def __init__(self, on_ragged=None):
        g = torch.Generator().manual_seed(99)
        self.batches = [{'left': torch.rand(n, 3, 64, 128, generator=g),
                         'right': torch.rand(n, 3, 64, 128, generator=g)} for n in (2, 2, 2, 1)]
        self.on_ragged = on_ragged

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            if b['left'].shape[0] == 1 and self.on_ragged is not None:
                self.on_ragged()
            yield b


def _two_epochs(check=None):
    """two train_one_epoch calls with one _GraphSteps from the formula
    weights -> the six epoch averages (+ what ``check`` collects)"""
    from train.train import _GraphSteps, train_one_epoch
    s = _setup('fp32', perceptual_start=1, capture=False)
    gs = _GraphSteps(s['m'], s['lf'], s['opt'], 4)
    seen = {}

    def on_ragged():
        seen['disc'] = {k: v.clone() for k, v in s['d'].state_dict().items()}
    out = []
    for epoch in range(2):
        out += list(train_one_epoch(s['m'], _Loader(on_ragged), s['lf'], s['opt'], 0.3, s['d'],
                                    s['dopt'], s['dlf'], epoch_number=epoch + 1, scales=4,
                                    perceptual_update_freq=2, device=DEV, no_pbar=True,
                                    graph_steps=gs))
        if check is not None:
            check(gs, seen, epoch)
    torch.cuda.synchronize()
    return out


# Three eager runs of _two_epochs from identical state, measured on MI355X:
# all six averages bit-equal between the runs (spread 0.0 -- at B=2 64x128 no
# float-atomic order noise reached the averages), and the captured run was
# bit-equal to them too.  The bar is 4 x that spread with the floor of 1e-4
# relative, which leaves room for the summation-order noise (turned into
# sign flips by Adam) that larger runs show (test_gpu_graph.py).
EAGER_SPREAD = 0.0
EPOCH_BAR = max(4 * EAGER_SPREAD, 1e-4)


def test_adversarial_epochs_captured_vs_eager(monkeypatch):
    """Two epochs of train_one_epoch (three full batches + a ragged one,
    perceptual_update_freq 2, perceptual_start 1) with one _GraphSteps: the
    step is captured once and replayed for the six full batches, the ragged
    batches step eagerly, the persistent clone holds the discriminator's
    state of the last refresh point, and the epoch averages track an eager
    run (UMAMD_ADV_GRAPH=0) from the same initial state.

    Bar: 4 x the spread of two EAGER runs from identical state, floor 1e-4
    relative.  Measured on MI355X: spread 0.0 (three eager runs bit-equal in
    all six averages; the captured run bit-equal to them), so the bar is the
    floor, 1e-4."""
    def check(gs, seen, epoch):
        assert gs.cap is not None and gs.captures == 1, 'captured once, reused by epoch 2'
        assert gs.replays == 3 * (epoch + 1) and gs.eager_steps == epoch + 1
        # every parameter of the refresh point.  (The BN running statistics
        # move on: the clone is in training mode, as the reference's deepcopy,
        # and the ragged batch's forwards after the refresh update them; in
        # training mode they do not enter any output.)
        clone = gs.disc_clone.state_dict()
        pnames = [k for k, _ in gs.disc_clone.named_parameters()]
        assert len(pnames) > 100
        for k in pnames:
            assert torch.equal(clone[k], seen['disc'][k]), k
        assert all(p.grad is None for p in gs.disc_clone.parameters())
    monkeypatch.delenv('UMAMD_ADV_GRAPH', raising=False)
    captured = _two_epochs(check)

    def no_graph(gs, seen, epoch):
        assert gs.cap is None and gs.captures == 0
    monkeypatch.setenv('UMAMD_ADV_GRAPH', '0')
    eager = _two_epochs(no_graph)
    assert len(captured) == len(eager) == 6
    assert all(np.isfinite(captured)) and all(np.isfinite(eager))
    rel = [abs(a / b - 1) for a, b in zip(captured, eager)]
    print(f'captured {captured}\neager {eager}\nrel {rel}')
    assert max(rel) <= EPOCH_BAR, (rel, EPOCH_BAR)
