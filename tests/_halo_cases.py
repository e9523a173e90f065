"""Case tables, f64 references and acceptance criteria of the halo conv tests
(test infrastructure, shared by tests/test_gpu_halo_conv.py, which runs the
kernel, and the CPU tests, which check the tables and that the criteria have
teeth).  Nothing here needs a GPU.

Operands are rounded to bf16 ONCE; the kernel and the reference (f64 torch on
those rounded operands and the f32 bias) then compute the same exact-operand
convolution, so the only differences are the kernel's f32 accumulation and the
one rounding of a bf16 output.

Bars (derived, not measured):
  * f32 output: max|got - ref| <= 1e-5 * max|ref| -- the project's bar for f32
    accumulation of bf16 operands (test_glds_stage_depth, test_tappack);
  * bf16 output, per element: |got - ref| <= 2^-8 |ref| + 1e-5 max|ref| -- one
    round-to-nearest of the stored value (8 significant bits) plus the
    accumulation allowance; no max-norm;
  * statistics (partial rows or f64 slots, summed in f64 by the test): the sum
    within 1e-4 * sum|y| per channel, the sum of squares within 1e-4 relative,
    the slot count exactly N*P*Q (the bar of test_conv_fwd_up2_slots).
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

N = 2
TH, TW = 8, 32  # the kernel's output tile

F32_TOL = 1e-5
BF16_EPS = 2.0 ** -8
STAT_TOL = 1e-4

# (Cin, Cout, R, pad mode, H, W)
EXACT_CASES = [
    (32, 32, 3, 'zero', 8, 32),
    (32, 32, 3, 'zero', 16, 64),
    (32, 64, 3, 'reflect', 8, 64),
    (32, 32, 7, 'zero', 16, 32),
    (64, 64, 5, 'zero', 8, 64),
    (40, 48, 3, 'reflect', 8, 32),
    (8, 32, 3, 'reflect', 8, 64),
    (64, 16, 3, 'zero', 16, 32),
    (32, 8, 3, 'reflect', 8, 32),
    (64, 96, 3, 'zero', 8, 32),
    (168, 128, 3, 'reflect', 8, 32),
    (88, 160, 3, 'zero', 8, 32),
    (32, 88, 5, 'zero', 8, 32),
    (96, 72, 7, 'zero', 8, 32),
]
# (halo_pf2, halo_res_kb): tap rows streamed, two rows ahead, resident
WEIGHT_MODES = [(0, 0), (1, 0), (0, 48)]
# persistent workgroups over resident weights, 8 tiles each (the second ragged)
PERSIST_CASES = [
    (32, 32, 3, 'zero', 16, 64),
    (32, 32, 3, 'zero', 10, 40),
]
PERSIST_GRIDS = [1, 3]
RAGGED_CASES = [
    (32, 32, 3, 'zero', 10, 40),
    (32, 32, 3, 'reflect', 9, 17),
    (40, 48, 3, 'reflect', 13, 33),
    (64, 64, 5, 'zero', 12, 20),
    (32, 32, 7, 'zero', 5, 16),
    (64, 96, 3, 'zero', 9, 48),
]
# reflect shapes whose last tile's halo would need a second reflection
REFUSED_CASES = [
    (32, 32, 3, 'reflect', 8, 16),
    (32, 32, 3, 'reflect', 4, 32),
    (32, 32, 5, 'reflect', 8, 33),
]
EPILOGUE_CASES = [
    (32, 32, 3, 'zero', 10, 40),
    (64, 96, 3, 'reflect', 8, 32),
]
EPILOGUES = ['bias', 'residual', 'sigmoid', 'elu']
SIGMOID_SCALE = 0.3
# data gradient, zero pad, stride 1: (C, K, R, H, W, resident weights + halo_grid 3)
DGRAD_CASES = [
    (32, 32, 7, 16, 32, False),
    (64, 64, 5, 8, 64, False),
    (48, 32, 3, 10, 40, False),
    (160, 64, 3, 8, 32, False),
    (32, 32, 3, 16, 64, True),
]

OUT_GUARD = 8  # sentinel columns after the K output channels (ld_out = K + 8)
STAT_GUARD = 2  # sentinel rows after the larger of the two row counts


def ceil_div(a, b):
    return (a + b - 1) // b


def halo_stat_rows(P, Q, n=N):
    """partial rows the halo kernel writes: two per 8 x 32 tile"""
    return 2 * n * ceil_div(P, TH) * ceil_div(Q, TW)


def stat_buffer_rows(P, Q, parts, n=N):
    """rows of a guarded partial-statistics buffer: whichever kernel runs,
    with or without the tiling condition of halo_applicable, stays inside"""
    return max(halo_stat_rows(P, Q, n), parts) + STAT_GUARD


def reflect_slack(C, R, W):
    """elements before and after a reflect input inside its larger tensor (a
    multiple of 8: the view stays 16-byte aligned)"""
    return ceil_div((R - 1) * (W + 1) * C, 8) * 8


def reflect_needs_second(R, H, W):
    """some tile's halo reaches past one reflection (rows or columns): the
    last tile's origin t0 plus T - 1 + pad, against 2 (n - 1)"""
    pad = (R - 1) // 2
    return ((H - 1) // TH * TH + TH - 1 + pad > 2 * (H - 1) or
            (W - 1) // TW * TW + TW - 1 + pad > 2 * (W - 1))


def _q(t):
    return t.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def fwd_operands(case):
    """-> dict of CPU tensors: x, w (NCHW f32, bf16-exact), bias (f32),
    residual (NCHW f32, bf16-exact), ref / mut (f64 NCHW conv + bias of the
    operands / of the mutant: tap (0, R-1) of the last real input channel
    zeroed).  Computed once per case and shared; callers do not modify it."""
    C, K, R, mode, H, W = case
    pad = (R - 1) // 2
    g = torch.Generator().manual_seed(1000 * C + 10 * K + R + H * W)
    x = _q(torch.randn(N, C, H, W, generator=g)).float()
    w = _q((torch.rand(K, C, R, R, generator=g) - 0.5) * 0.2).float()
    bias = torch.randn(K, generator=g) * 0.5
    res = _q(torch.randn(N, K, H, W, generator=g)).float()
    wm = w.clone()
    wm[:, C - 1, 0, R - 1] = 0
    xp = F.pad(x.double(), (pad,) * 4, mode='reflect' if mode == 'reflect' else 'constant')
    ref = F.conv2d(xp, w.double(), bias.double())
    mut = F.conv2d(xp, wm.double(), bias.double())
    return dict(x=x, w=w, bias=bias, residual=res, ref=ref, mut=mut)


def epilogue_ref(y, op, epi):
    """f64 reference of an epilogue on the conv + bias ``y``"""
    if epi == 'residual':
        return y + op['residual'].double()
    if epi == 'sigmoid':
        return SIGMOID_SCALE * torch.sigmoid(y)
    if epi == 'elu':
        return F.elu(y)
    return y


@functools.lru_cache(maxsize=None)
def dgrad_operands(case):
    """-> dict: dy, w (bf16-exact f32), prev (the dx accumulated onto), ref /
    mut (f64 adjoint; the mutant zeroes tap (0, R-1) of the last channel the
    flipped conv reduces over, K - 1)"""
    C, K, R, H, W, _ = case
    pad = (R - 1) // 2
    g = torch.Generator().manual_seed(77 + 1000 * C + 10 * K + R + H * W)
    dy = _q(torch.randn(N, K, H, W, generator=g)).float()
    w = _q((torch.rand(K, C, R, R, generator=g) - 0.5) * 0.2).float()
    prev = _q(torch.randn(N, C, H, W, generator=g)).float()
    wm = w.clone()
    wm[K - 1, :, 0, R - 1] = 0
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w.double(), dy.double(), padding=pad)
    mut = torch.nn.grad.conv2d_input((N, C, H, W), wm.double(), dy.double(), padding=pad)
    return dict(dy=dy, w=w, prev=prev, ref=ref, mut=mut)


# ------------------------------------------------------------- criteria ----
def f32_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max())


def f32_ok(got, ref):
    return f32_err(got, ref) <= F32_TOL


def bf16_ratio(got, ref):
    """largest per-element error over its bound (<= 1 passes)"""
    got, ref = got.double(), ref.double()
    bound = BF16_EPS * ref.abs() + F32_TOL * ref.abs().max()
    return float(((got - ref).abs() / bound).max())


def bf16_ok(got, ref):
    return bf16_ratio(got, ref) <= 1.0


def stats_err(s1, s2, ref):
    """s1, s2: per-channel f64 sum and sum of squares; ref f64 NCHW ->
    (sum error over sum|y|, sum-of-squares relative error), worst channel"""
    r1, r2 = ref.sum(dim=(0, 2, 3)), (ref * ref).sum(dim=(0, 2, 3))
    scale = ref.abs().sum(dim=(0, 2, 3))
    return (float(((s1.double().cpu() - r1).abs() / scale).max()),
            float(((s2.double().cpu() - r2).abs() / r2).max()))


def stats_ok(s1, s2, ref):
    e1, e2 = stats_err(s1, s2, ref)
    return e1 <= STAT_TOL and e2 <= STAT_TOL
