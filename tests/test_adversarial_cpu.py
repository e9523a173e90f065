"""CPU-only checks of the adversarial glue's host side: which loss modules
dispatch to um_label_loss, and that nothing falls back silently on the CPU."""
import pytest
import torch


def test_label_loss_kind_is_exact():
    from umamd import discfn as DF
    from umamd._lib import LABEL_BCE, LABEL_MSE

    class MyMSE(torch.nn.MSELoss):
        pass
    assert DF.label_loss_kind(torch.nn.MSELoss()) == LABEL_MSE
    assert DF.label_loss_kind(torch.nn.BCELoss()) == LABEL_BCE
    for m in (MyMSE(), torch.nn.MSELoss(reduction='sum'), torch.nn.BCELoss(reduction='none'),
              torch.nn.BCELoss(weight=torch.ones(3)), torch.nn.L1Loss(), lambda p, y: p.mean()):
        assert DF.label_loss_kind(m) is None


def test_generator_loss_keeps_module_attribute():
    from train.loss import GeneratorLoss
    assert type(GeneratorLoss('mse').adversarial) is torch.nn.MSELoss
    assert type(GeneratorLoss('bce').adversarial) is torch.nn.BCELoss


def test_new_entries_raise_on_cpu_tensors():
    from umamd import discfn as DF
    from umamd._lib import LABEL_BCE, UmamdError
    with pytest.raises(UmamdError):
        DF.label_loss(torch.rand(4, 1), LABEL_BCE, 2)
    with pytest.raises(UmamdError):
        DF.image_pair_to_nhwc(torch.rand(1, 6, 8, 16), torch.rand(1, 6, 8, 16), torch.float32)


def test_graph_steps_decline_cpu_and_switch(monkeypatch):
    """_GraphSteps.usable: a CPU model or discriminator steps eagerly"""
    from train.train import _GraphSteps
    from train.loss import TukraUncertaintyLoss
    from umamd.optim import Adam
    m, d = torch.nn.Linear(2, 2), torch.nn.Linear(2, 1)
    lf = TukraUncertaintyLoss()
    opt, dopt = Adam(m.parameters(), 1e-4), Adam(d.parameters(), 1e-4)
    assert not _GraphSteps.usable(m, lf, opt, None)
    assert not _GraphSteps.usable(m, lf, opt, d, dopt)
    gs = _GraphSteps(m, lf, opt, 4)
    assert gs.bind_discriminator(None, None, None, 2) is None
    clone = gs.bind_discriminator(d, dopt, torch.nn.BCELoss(), 2)
    assert clone is not d and clone is gs.bind_discriminator(d, dopt, torch.nn.BCELoss(), 2)
    with torch.no_grad():
        d.weight.add_(1.0)
    assert not torch.equal(clone.weight, d.weight)
    gs.bind_discriminator(d, dopt, torch.nn.BCELoss(), 2)  # epoch start: refreshed in place
    assert torch.equal(clone.weight, d.weight)
