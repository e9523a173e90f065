"""f64 references for the standalone loss terms, composed from oracle.loss
(which is the yardstick and is not edited): the error map with run-time
``c1``/``c2`` (oracle.loss.image_error has them compiled in, oracle.loss.dssim
takes them), the NLL on its own, the shapes and the inputs the CPU and GPU
tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from oracle import loss as OL

# (N, H, W): a 1x1 SSIM grid; the smallest ragged one; one row and six columns
# past a 16x64 tile; two tile rows; more than three tiles wide
SHAPES = [(2, 3, 3), (1, 4, 5), (2, 17, 70), (1, 40, 72), (2, 32, 200)]
SHAPES_2X2 = [(1, 2, 2)] + SHAPES
WSSIM_PARAMS = [(0.85, 0.01, 0.03), (0.5, 0.02, 0.05)]
LOSS_TYPES = ('l1', 'bayesian', 'log_bayesian')


def fixture():
    return np.load(os.path.join(GOLDEN, 'loss_terms.npz'))


def wtag(alpha, k1, k2):
    return f'w_a{alpha:g}_k{k1:g}_{k2:g}'


def rel_norm(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def close(got, ref, floor=0.0):
    return abs(float(got) - float(ref)) <= 1e-4 * abs(float(ref)) + floor


def image_error(images, recon, alpha, k1, k2):
    """oracle.loss.image_error with c1 = k1^2, c2 = k2^2"""
    c1, c2 = k1 ** 2, k2 ** 2
    h, w = images.shape[-2:]
    l1 = (images - recon).abs()
    ss = torch.cat((OL.dssim(images[:, 0:3], recon[:, 0:3], c1, c2),
                    OL.dssim(images[:, 3:6], recon[:, 3:6], c1, c2)), 1)
    ss = F.interpolate(ss, size=(h, w), mode='bilinear', align_corners=True)
    tot = alpha * ss + (1 - alpha) * l1
    return torch.cat((tot[:, 0:3].mean(1, keepdim=True), tot[:, 3:6].mean(1, keepdim=True)), 1)


def wssim(images, recon, alpha, k1, k2):
    e = image_error(images, recon, alpha, k1, k2)
    return (e[:, 0:1] + e[:, 1:2]).mean(), e


def nll(unc, err, loss_type):
    """oracle.loss.error_loss with both weights off is the NLL alone"""
    pred = torch.cat((torch.zeros_like(unc), unc), 1)
    return OL.error_loss(pred, None, err, loss_type, 0.0, 0.0, False)


def smooth(shape, g, noise=0.01):
    """3x3-box-blurred (twice) U[0,1) noise stretched back to [0, 1], plus a
    little white noise: a map with the small neighbour differences of a
    disparity or an image.  The warp's gradient w.r.t. the shift is
    d(sample)/dx * W, which jumps where a sample position crosses an integer;
    f32 and the f64 oracle can land on either side of one (about one pixel in
    1e5 does), and on white noise a single such pixel is worth more than the
    4e-3 bar at 2x32x200 -- the f32 CPU oracle against the f64 one shows the
    same figure.  On a smooth sampled map the jump is small, as it is for the
    maps the loss sees in training (test_gpu_loss_stack._smooth_preds)."""
    x = torch.rand(*shape, generator=g)
    for _ in range(2):
        x = F.avg_pool2d(F.pad(x, (1, 1, 1, 1), mode='replicate'), 3, 1)
    lo, hi = x.amin(dim=(2, 3), keepdim=True), x.amax(dim=(2, 3), keepdim=True)
    return (x - lo) / (hi - lo).clamp_min(1e-6) + noise * torch.rand(*shape, generator=g)


def inputs(N, H, W, seed=7):
    """images, a recon that is no reconstruct_pyramid output (a blend of a
    perturbed image and the batch-flipped image), a smooth 4-channel
    prediction in (0.02, 0.22) and an upstream gradient for the map; all f32,
    CPU"""
    g = torch.Generator().manual_seed(seed + 1000 * N + 10 * H + W)
    images = torch.rand(N, 6, H, W, generator=g)
    noisy = (images + 0.1 * torch.randn(N, 6, H, W, generator=g)).clamp(0, 1)
    recon = 0.7 * noisy + 0.3 * images.flip(0).flip(3)
    pred = 0.02 + 0.2 * smooth((N, 4, H, W), g)
    gmap = torch.rand(N, 2, H, W, generator=g) + 0.1
    return images, recon, pred, gmap
