"""The two HIP entries of the adversarial glue (csrc/disc.hip):

* ``um_label_loss_fwd`` / ``_bwd`` (umamd.discfn.label_loss) against
  torch's MSELoss / BCELoss in f64 on the CPU with materialised labels;
* ``um_image_pair_to_nhwc`` (umamd.discfn.image_pair_to_nhwc) against the
  layout conversion of the concatenated batch, bit for bit.

Marked gpu."""
import pytest
import torch

from test_gpu_model import DEV

pytestmark = pytest.mark.gpu

G = 0.37  # upstream gradient of the loss (the adversarial weight's role)


def _probabilities(N, n_real, variant):
    """seeded probabilities with exact 0.0 and 1.0 in the real (label 1) and
    the fake (label 0) region: first / last element of each region; a region
    of one element takes 0.0 (variant 0) or 1.0 (variant 1)"""
    g = torch.Generator().manual_seed(100 * N + n_real)
    p = torch.rand(N, 1, generator=g) * 0.98 + 0.01
    sat = []
    for lo, hi in ((0, n_real), (n_real, N)):
        if hi - lo >= 2:
            a, b = (0.0, 1.0) if variant == 0 else (1.0, 0.0)
            p[lo, 0], p[hi - 1, 0] = a, b
            sat += [lo, hi - 1]
        elif hi - lo == 1:
            p[lo, 0] = float(variant)
            sat.append(lo)
    return p, sat


@pytest.mark.parametrize('N', [1, 2, 4, 16, 65, 300])
@pytest.mark.parametrize('kind', ['mse', 'bce'])
def test_label_loss_matches_torch_f64(kind, N):
    """loss and every dp element within 1e-6 relative + 1e-7 absolute of the
    f64 reference (f64 accumulation on the device: only single f32
    roundings differ), finite at saturated probabilities"""
    from umamd import discfn as DF
    module = torch.nn.MSELoss() if kind == 'mse' else torch.nn.BCELoss()
    code = DF.label_loss_kind(module)
    assert code is not None
    g32 = float(torch.tensor(G, dtype=torch.float32))
    for n_real in sorted({0, N // 2, N}):
        for variant in (0, 1):
            p, sat = _probabilities(N, n_real, variant)
            ref_p = p.double().requires_grad_(True)
            labels = torch.zeros_like(ref_p)
            labels[:n_real] = 1
            ref = module(ref_p, labels)
            (ref * g32).backward()
            dev_p = p.to(DEV).requires_grad_(True)
            got = DF.label_loss(dev_p, code, n_real)
            (got * G).backward()
            torch.cuda.synchronize()
            case = (kind, N, n_real, variant)
            a, b = float(got), float(ref)
            print(f'label loss {case}: got {a!r} ref {b!r}')
            assert abs(a - b) <= 1e-6 * abs(b) + 1e-7, case
            dp, dref = dev_p.grad.double().cpu(), ref_p.grad
            assert dp.shape == dref.shape
            err = (dp - dref).abs() - (1e-6 * dref.abs() + 1e-7)
            assert float(err.max()) <= 0, (case, int(err.argmax()), dp.flatten()[err.argmax()],
                                           dref.flatten()[err.argmax()])
            assert torch.isfinite(got).all() and torch.isfinite(dev_p.grad[sat]).all(), case


def test_label_loss_dispatch_keeps_other_modules():
    """only exactly MSELoss / BCELoss with mean reduction and no weight"""
    from umamd import discfn as DF
    from umamd._lib import LABEL_BCE, LABEL_MSE

    class MyBCE(torch.nn.BCELoss):
        pass
    assert DF.label_loss_kind(torch.nn.MSELoss()) == LABEL_MSE
    assert DF.label_loss_kind(torch.nn.BCELoss()) == LABEL_BCE
    for m in (torch.nn.MSELoss(reduction='sum'), torch.nn.BCELoss(reduction='none'),
              torch.nn.BCELoss(weight=torch.ones(1)), MyBCE(), torch.nn.L1Loss(),
              torch.nn.BCEWithLogitsLoss()):
        assert DF.label_loss_kind(m) is None, m
    # a module off the list still works through run_discriminator's ATen path
    import train.utils as u

    class Probe(torch.nn.Module):
        def forward(self, pyramid):
            return torch.sigmoid(pyramid[0].mean((1, 2, 3))).unsqueeze(1)
    img = [torch.rand(2, 6, 8, 16, device=DEV)]
    rec = [torch.rand(2, 6, 8, 16, device=DEV)]
    a = u.run_discriminator(img, rec, Probe(), torch.nn.BCELoss(), 2)
    b = u.run_discriminator(img, rec, Probe(), MyBCE(), 2)
    assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b)) + 1e-7


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('H,W', [(8, 16), (5, 7)])
@pytest.mark.parametrize('N', [1, 2])
def test_image_pair_to_nhwc_equals_cat(N, H, W, dtype):
    from umamd import discfn as DF
    from umamd import functional as U
    from umamd._lib import UmamdError
    g = torch.Generator().manual_seed(N * 1000 + H)
    a = torch.rand(N, 6, H, W, generator=g).to(DEV)
    b = torch.rand(N, 6, H, W, generator=g).to(DEV)
    got = DF.image_pair_to_nhwc(a, b, dtype)
    ref = U.image_to_nhwc(torch.cat((a, b), 0), dtype)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (2 * N, H, W, 8) and got.dtype == dtype
    assert torch.equal(got, ref)
    for x, y in ((a.clone().requires_grad_(True), b), (a, b.clone().requires_grad_(True))):
        with pytest.raises(UmamdError):
            DF.image_pair_to_nhwc(x, y, dtype)


def test_discriminator_takes_pairs():
    """RandomDiscriminator.forward on (image, recon) pairs per level equals
    its forward on the concatenated pyramid"""
    from test_gpu_adversarial import _disc, _pyr, _z
    z = _z()
    _, _, pyr = _pyr(z)
    other = [t.flip(0).contiguous() * 0.5 for t in pyr]
    d1, d2 = _disc(z), _disc(z)
    with torch.no_grad():
        got = d1(list(zip(pyr, other)))
        ref = d2([torch.cat((x, y), 0) for x, y in zip(pyr, other)])
    torch.cuda.synchronize()
    # same kernels on the same values after the (bit-equal) conversion; only the
    # BN statistics' f64 atomic order differs between two forwards
    assert got.shape == ref.shape == (4, 1)
    assert float((got - ref).abs().max()) <= 1e-6
