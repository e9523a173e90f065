"""Deep-layer GEMM main loops: the LDS-DMA implicit GEMM's tap-outer issue
cursor (igemm.hip glds_tile) and the transposed-read weight gradient's
incremental operand addresses (wgrad_tr.hip), at the smallest shapes where
the cursors can go wrong: taps of 1, 2 and 3 k-steps, splits that begin
inside a tap, loops shorter than the stage count, out-of-range rows and
columns, rows that wrap inside a k-step.  Every result is compared with a
torch f64 convolution of the same bf16-rounded operands, with the tolerances
tests/test_gpu_ops.py uses for these entries, and the LDS-DMA path with the
register path (glds = 0) on the same inputs."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DT = torch.bfloat16
TOL_FWD = 1e-5   # f32 output of bf16 operands (test_glds_stage_depth)
TOL_DGRAD = 1e-2  # bf16 output (test_glds_stage_depth, test_dgrad_stride2_classes)
TOL_WGRAD = 1e-4  # f32 slabs (test_wgrad)


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw(x):
    return x.detach().permute(0, 3, 1, 2).float().cpu()


# split-K forced on (every grid below 256 tiles splits towards 512 blocks,
# >= minsteps k-steps per split) or off; the 1x1 cases have 1 or 2 k-steps, so
# only a one-step minimum splits them at all
def _split_knobs(split, R):
    if not split:
        return dict(glds_split_below=0, split_below=0)
    return dict(glds_split_below=256, glds_split_target=512, split_minsteps=4 if R > 1 else 1)


_REF = {}


def _fwd_dgrad_case(C, K, R, mode, N=2, H=9, W=7):
    """inputs and f64 references of one stride-1 case, computed once"""
    key = (C, K, R, mode, N, H, W)
    if key in _REF:
        return _REF[key]
    pad = (R - 1) // 2
    g = torch.Generator().manual_seed(1000 + C + 7 * K + R)
    w = (torch.rand(K, C, R, R, generator=g) - 0.5) * 0.2
    x = torch.randn(N, C, H, W, generator=g)
    dy = torch.randn(N, K, H, W, generator=g)
    wq, xq, dyq = (t.to(DT).double() for t in (w, x, dy))
    xr = xq.clone().requires_grad_(True)
    xp = F.pad(xr, (pad,) * 4, mode='reflect') if mode == 'reflect' and pad else \
        F.pad(xr, (pad,) * 4)
    ref_y = F.conv2d(xp, wq)
    ref_y.backward(dyq)
    _REF[key] = (w, x, dy, ref_y.detach(), xr.grad.detach())
    return _REF[key]


def _run_fwd_dgrad(C, K, R, mode, split, extra=None):
    from umamd import functional as U
    from umamd._lib import PAD_REFLECT, PAD_ZERO, tuning
    N, H, W = 2, 9, 7  # M = 126: the last 64-row tile has out-of-range rows
    w, x, dy, ref_y, ref_dx = _fwd_dgrad_case(C, K, R, mode)
    pad = (R - 1) // 2
    pm = PAD_REFLECT if mode == 'reflect' else PAD_ZERO
    wf, wT = U._pack(w.to(DEV), C, DT)
    outs = []
    for glds in (5, 0):  # LDS-DMA 8-wave 64x64 tiles, then the register path
        knobs = dict(halo=0, glds=glds, **_split_knobs(split, R))
        knobs.update(extra or {})
        with tuning(**knobs):
            y = U._conv_fwd(_nhwc(x).to(DT), wf, None, K, R, 1, pad, pm, out_dtype=torch.float32)
            dx = U._conv_dgrad(_nhwc(dy).to(DT), wT, (N, H, W, C), K, R, 1, pad, pm)
            torch.cuda.synchronize()
        outs.append((_nchw(y), _nchw(dx)))
        ey, ex = _rel(outs[-1][0], ref_y), _rel(outs[-1][1], ref_dx)
        print(f'C{C} K{K} R{R} {mode} split={split} glds={glds}: fwd {ey:.3e} dgrad {ex:.3e}')
        assert ey < TOL_FWD, ey
        assert ex < TOL_DGRAD, ex
    ey, ex = _rel(outs[0][0], outs[1][0]), _rel(outs[0][1], outs[1][1])
    print(f'  LDS-DMA vs register: fwd {ey:.3e} dgrad {ex:.3e}')
    assert ey < TOL_FWD, ey
    assert ex < TOL_DGRAD, ex


# K = 128 (NC > 64: the 64x64 tiles); C = 64/128/192: a tap lasts 1, 2 or 3
# k-steps (a tap boundary on every step; an odd count), so the prefetch runs
# across taps; K = 136: B rows past NC; 1x1 with C = 64/128: 1 and 2 k-steps,
# fewer than the stage count, so only the draining tail runs
FWD_CASES = [(64, 128, 3, 'zero'), (128, 128, 3, 'zero'), (192, 128, 3, 'zero'),
             (64, 128, 3, 'reflect'), (128, 128, 3, 'reflect'), (192, 128, 3, 'reflect'),
             (128, 136, 3, 'zero'), (64, 128, 1, 'zero'), (128, 128, 1, 'zero')]


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('case', FWD_CASES)
def test_glds_cursor_fwd_dgrad(case, split):
    C, K, R, mode = case
    _run_fwd_dgrad(C, K, R, mode, split)


def test_glds_cursor_six_stages():
    """the unsplit 3x3 C = 64 case on the 6-stage loop (9 k-steps: 3 steady, 6 draining)"""
    _run_fwd_dgrad(64, 128, 3, 'zero', False, extra=dict(glds_deep=6, glds_deep_blocks=1024))


@pytest.mark.parametrize('split', [False, True])
def test_glds_cursor_stride2_classes(split):
    """stride-2 data gradient, C = K = 64 on 8x8 -> 16x16: the four parity
    classes as one launch of LDS-DMA tiles (1, 2, 2 and 4 one-step taps)"""
    from umamd import functional as U
    from umamd._lib import PAD_ZERO, tuning
    C = K = 64
    N, H, W, R, pad = 2, 16, 16, 3, 1
    g = torch.Generator().manual_seed(17)
    w = (torch.rand(K, C, R, R, generator=g) - 0.5) * 0.2
    dy = torch.randn(N, K, 8, 8, generator=g)
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w.to(DT).double(), dy.to(DT).double(),
                                     stride=2, padding=pad)
    _, wT = U._pack(w.to(DEV), C, DT, wf=False)
    outs = []
    for cls_glds in (3, 0):  # LDS-DMA tiles, then the 256-row register tiles
        knobs = dict(cls4=1, cls_glds=cls_glds, **_split_knobs(split, 1))
        with tuning(**knobs):
            dx = U._conv_dgrad(_nhwc(dy).to(DT), wT, (N, H, W, C), K, R, 2, pad, PAD_ZERO)
            torch.cuda.synchronize()
        outs.append(_nchw(dx))
        err = _rel(outs[-1], ref)
        print(f'stride-2 classes split={split} cls_glds={cls_glds}: {err:.3e}')
        assert err < TOL_DGRAD, err
    assert _rel(outs[0], outs[1]) < TOL_DGRAD


# Weight gradient on the transposed-read kernel (bf16, K > 32, shapes the
# halo-tiled kernel does not take: Q < 32, 1x1, or more than 32 16x16 tiles
# per tap).  Maps: 8x16 (Q divides the 32-pixel k-step: whole rows per step),
# 5x7 (Q does not divide 32, M = 70 is no multiple of 32, rows wrap inside a
# step), 3x40 (Q > 32).  The >= 256 pixels per split of the split plan leave
# these N = 2 maps one split; the larger-N cases below reach 3 splits, whose
# later splits start inside an image.
def _wgrad_check(N, C, K, R, st, mode, H, W, want_splits=None):
    from umamd import functional as U
    from umamd._lib import PAD_REFLECT, PAD_ZERO, query
    pad = (R - 1) // 2
    g = torch.Generator().manual_seed(7)
    x = torch.rand(N, C, H, W, generator=g) - 0.5
    P = (H + 2 * pad - R) // st + 1
    Q = (W + 2 * pad - R) // st + 1
    dy = torch.randn(N, K, P, Q, generator=g)
    xb, dyb = x.to(DT), dy.to(DT)
    xpb = F.pad(xb.double(), (pad,) * 4, mode='reflect' if mode == 'reflect' and pad else 'constant')
    ref = torch.nn.grad.conv2d_weight(xpb, (K, C, R, R), dyb.double(), stride=st)
    pm = PAD_REFLECT if mode == 'reflect' else PAD_ZERO
    splits = query('um_conv_wgrad_splits', 1, N, H, W, C, C, K, R, st, pad, pm, P, Q, K)
    got = U._conv_wgrad(_nhwc(xb), _nhwc(dyb), K, K, C, R, st, pad, pm)
    torch.cuda.synchronize()
    err = _rel(got, ref)
    print(f'wgrad N{N} C{C} K{K} R{R} s{st} {mode} {H}x{W}: splits {splits} rel {err:.3e}')
    if want_splits is not None:
        assert splits == want_splits, splits
    assert err < TOL_WGRAD, err


@pytest.mark.parametrize('hw', [(8, 16), (5, 7), (3, 40)])
@pytest.mark.parametrize('rmode', [(1, 'zero'), (3, 'zero'), (3, 'reflect')])
@pytest.mark.parametrize('ck', [(64, 64), (72, 128)])
def test_wgrad_tr_addresses(ck, rmode, hw):
    C, K = ck
    R, mode = rmode
    _wgrad_check(2, C, K, R, 1, mode, *hw)


def test_wgrad_tr_stride2():
    """16x32 -> 8x16 outputs: whole output rows per k-step, source rows two apart"""
    _wgrad_check(2, 64, 64, 3, 2, 'zero', 16, 32)


@pytest.mark.parametrize('case', [(6, 64, 64, 3, 'zero', 8, 16), (16, 72, 128, 3, 'reflect', 5, 7),
                                  (6, 72, 128, 1, 'zero', 3, 40)])
def test_wgrad_tr_three_splits(case):
    """M = 768, 560 and 720 pixels: 3 splits of 256, 192 and 256 pixels, the
    later ones starting inside an image (and, for 5x7, inside a row)"""
    N, C, K, R, mode, H, W = case
    _wgrad_check(N, C, K, R, 1, mode, H, W, want_splits=3)
