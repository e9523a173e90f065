"""The halo-tiled direct conv (csrc/halo_conv.hip) against f64 torch on the
same bf16-rounded operands: every weight mode, column-block width, epilogue
arm, ragged edge tile and the flipped data gradient, with the kernel forced on
(tuning halo_min_tiles=1) and ``um_conv_halo_ok`` asserting that it is the halo
kernel that runs.  Tables, references and bars: tests/_halo_cases.py (the CPU
suite checks there that every bar rejects a one-tap mutant).

Every buffer the kernel writes is guarded: outputs have ld_out = K + 8 with
sentinel columns, partial-statistics buffers have sentinel rows past
um_conv_stats_parts, and inputs sit inside a larger NaN-filled tensor, so a
stray read that reaches a real output, or any stray write, fails the test
instead of landing in a neighbouring allocation.  Marked gpu."""
import pytest
import torch

import _halo_cases as HC

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = -1984.0  # exact in bf16
BF16, F32 = torch.bfloat16, torch.float32


def _pm(mode):
    from umamd._lib import PAD_REFLECT, PAD_ZERO
    return PAD_REFLECT if mode == 'reflect' else PAD_ZERO


def _epi_code(epi):
    from umamd import _lib as L
    return {'bias': L.EPI_NONE, 'residual': L.EPI_RESIDUAL, 'sigmoid': L.EPI_SIGMOID_SCALE,
            'elu': L.EPI_ELU, 'stats': L.EPI_STATS, 'slots': L.EPI_STAT_SLOTS}[epi]


def _halo_ok(case, epi='bias'):
    from umamd._lib import UM_BF16, query
    C, K, R, mode, H, W = case
    return query('um_conv_halo_ok', UM_BF16, HC.N, H, W, C, K, R, 1, (R - 1) // 2, _pm(mode), H, W,
                 _epi_code(epi), 0)


def _guarded_nhwc(t, R):
    """NCHW f32 (bf16-exact) -> NHWC bf16 device view inside a NaN-filled
    tensor with reflect_slack elements before and after it"""
    n, c, h, w = t.shape
    slack = HC.reflect_slack(c, R, w)
    big = torch.full((2 * slack + t.numel(),), float('nan'), dtype=BF16, device=DEV)
    v = big[slack:slack + t.numel()].view(n, h, w, c)
    v.copy_(t.permute(0, 2, 3, 1).to(BF16))
    return v


def _nchw(y):
    return y.detach().permute(0, 3, 1, 2).double().cpu()


class _Fwd:
    """one case on the device: packed weights, guarded input, launches"""

    def __init__(self, case):
        from umamd import functional as U
        self.case = case
        C, K, R, mode, H, W = case
        self.op = HC.fwd_operands(case)
        self.x = _guarded_nhwc(self.op['x'], R)
        self.wf, _ = U._pack(self.op['w'].to(DEV), C, BF16, wT=False)
        self.bias = self.op['bias'].to(DEV)
        res = torch.full((HC.N, H, W, K + HC.OUT_GUARD), SENT, dtype=BF16, device=DEV)
        res[..., :K] = self.op['residual'].permute(0, 2, 3, 1).to(BF16)
        self.residual = res  # ldr = K + 8

    def run(self, out_dtype, epi='bias', stats=None):
        """-> the K real output channels, NCHW f64 on the CPU; the output goes
        through ``out=`` into a buffer of ld_out = K + 8 whose padding columns
        must keep their sentinel"""
        from umamd import functional as U
        C, K, R, mode, H, W = self.case
        buf = torch.full((HC.N, H, W, K + HC.OUT_GUARD), SENT, dtype=out_dtype, device=DEV)
        U._conv_fwd(self.x, self.wf, self.bias, K, R, 1, (R - 1) // 2, _pm(mode),
                    out_dtype=out_dtype, epi=_epi_code(epi), epi_scale=HC.SIGMOID_SCALE,
                    residual=self.residual if epi == 'residual' else None, stats=stats, out=buf)
        torch.cuda.synchronize()
        assert bool((buf[..., K:] == SENT).all()), 'output padding columns written'
        return _nchw(buf[..., :K])

    def check_outputs(self, tag, epi='bias'):
        """f32 output against the f32 bar; bf16 output unstaged and staged,
        bit-equal, against the per-element bar.  Prints the observed maxima."""
        from umamd._lib import tuning
        ref = HC.epilogue_ref(self.op['ref'], self.op, epi)
        e32 = HC.f32_err(self.run(F32, epi), ref)
        with tuning(halo_staged=0):
            y0 = self.run(BF16, epi)
        with tuning(halo_staged=1):
            y1 = self.run(BF16, epi)
        rb = HC.bf16_ratio(y0, ref)
        print(f'halo_conv {tag} {self.case} {epi}: f32 rel {e32:.3e} bf16 err/bound {rb:.3f}')
        assert e32 <= HC.F32_TOL, e32
        assert rb <= 1.0, rb
        assert torch.equal(y0, y1), 'staged and unstaged bf16 outputs differ'


# exact tiles: weight modes x column-block widths
@pytest.mark.parametrize('mode', HC.WEIGHT_MODES)
@pytest.mark.parametrize('case', HC.EXACT_CASES)
def test_exact_tiles(case, mode):
    from umamd._lib import tuning
    pf2, res = mode
    with tuning(halo_min_tiles=1, halo_pf2=pf2, halo_res_kb=res):
        assert _halo_ok(case) == 1
        _Fwd(case).check_outputs(f'exact pf2={pf2} res={res}')


# persistent workgroups over resident weights: 8 tiles on 1 or 3 workgroups
@pytest.mark.parametrize('grid', HC.PERSIST_GRIDS)
@pytest.mark.parametrize('case', HC.PERSIST_CASES)
def test_persistent_tiles(case, grid):
    from umamd._lib import tuning
    with tuning(halo_min_tiles=1, halo_pf2=0, halo_res_kb=48, halo_grid=grid):
        assert _halo_ok(case) == 1
        _Fwd(case).check_outputs(f'persist grid={grid}')


# ragged edge tiles through the forward pass
@pytest.mark.parametrize('case', HC.RAGGED_CASES)
def test_ragged_outputs(case):
    from umamd._lib import tuning
    with tuning(halo_min_tiles=1):
        assert _halo_ok(case) == 1
        _Fwd(case).check_outputs('ragged')


def _check_stats(tag, case, s1, s2, ref):
    e1, e2 = HC.stats_err(s1, s2, ref)
    print(f'halo_conv {tag} {case}: sum err {e1:.3e} sumsq err {e2:.3e}')
    assert e1 <= HC.STAT_TOL, e1
    assert e2 <= HC.STAT_TOL, e2


@pytest.mark.parametrize('case', HC.RAGGED_CASES)
def test_ragged_stat_slots(case):
    """f64 slots take any tiling: the halo kernel, its statistics and count"""
    from umamd import _lib as L
    from umamd._lib import tuning
    C, K, R, mode, H, W = case
    nslot = L.STAT_SLOTS * K * 2
    slots = torch.zeros(nslot + 1 + 8, dtype=torch.float64, device=DEV)
    slots[nslot + 1:] = SENT
    with tuning(halo_min_tiles=1):
        assert _halo_ok(case, 'slots') == 1
        f = _Fwd(case)
        y = f.run(F32, 'slots', stats=slots)
    ref = f.op['ref']
    e32 = HC.f32_err(y, ref)
    print(f'halo_conv slots {case}: f32 rel {e32:.3e}')
    assert e32 <= HC.F32_TOL, e32
    st = slots[:nslot].view(L.STAT_SLOTS, K, 2).sum(0)
    _check_stats('slots', case, st[:, 0], st[:, 1], ref)
    assert float(slots[nslot]) == HC.N * H * W
    assert bool((slots[nslot + 1:] == SENT).all())


def _partial_rows(f, case, halo):
    """UM_EPI_STATS into a guarded buffer -> (y, s1, s2); asserts the path
    and that no row past um_conv_stats_parts is written"""
    from umamd._lib import query
    C, K, R, mode, H, W = case
    parts = query('um_conv_stats_parts', HC.N * H * W, K)
    rows = HC.stat_buffer_rows(H, W, parts)
    st = torch.full((rows, K, 2), float('nan'), dtype=F32, device=DEV)
    st[parts:] = SENT
    assert _halo_ok(case, 'stats') == halo
    y = f.run(F32, 'stats', stats=st)
    assert bool((st[parts:] == SENT).all()), 'statistics rows past um_conv_stats_parts written'
    s = st[:parts].double().sum(0)
    return y, s[:, 0], s[:, 1]


@pytest.mark.parametrize('case', HC.RAGGED_CASES)
def test_ragged_partial_rows(case):
    """partial-row statistics on a ragged tiling: two rows per tile would
    overrun the um_conv_stats_parts rows, so the halo kernel is not taken;
    output and statistics are right on the path that runs and the rows past
    the buffer the callers size stay untouched"""
    from umamd._lib import tuning
    with tuning(halo_min_tiles=1):
        f = _Fwd(case)
        y, s1, s2 = _partial_rows(f, case, halo=0)
    e32 = HC.f32_err(y, f.op['ref'])
    print(f'halo_conv ragged-stats {case}: f32 rel {e32:.3e}')
    assert e32 <= HC.F32_TOL, e32
    _check_stats('ragged-stats', case, s1, s2, f.op['ref'])


def test_exact_partial_rows():
    """partial-row statistics on the halo kernel (exact tiling; small=0 keeps
    the 128-row layout at 96 output channels)"""
    from umamd._lib import tuning
    case = HC.EPILOGUE_CASES[1]
    assert case[4] % HC.TH == 0 and case[5] % HC.TW == 0
    with tuning(halo_min_tiles=1, small=0):
        f = _Fwd(case)
        y, s1, s2 = _partial_rows(f, case, halo=1)
    e32 = HC.f32_err(y, f.op['ref'])
    print(f'halo_conv exact-stats {case}: f32 rel {e32:.3e}')
    assert e32 <= HC.F32_TOL, e32
    _check_stats('exact-stats', case, s1, s2, f.op['ref'])


@pytest.mark.parametrize('case', HC.REFUSED_CASES)
def test_refused_reflect(case):
    """reflect shapes whose last tile would reflect twice (and read before
    the tensor) are not taken by the halo kernel; results are right"""
    from umamd._lib import tuning
    with tuning(halo_min_tiles=1):
        assert _halo_ok(case) == 0
        _Fwd(case).check_outputs('refused')


@pytest.mark.parametrize('epi', HC.EPILOGUES)
@pytest.mark.parametrize('case', HC.EPILOGUE_CASES)
def test_epilogues(case, epi):
    """bias, bf16 residual (ldr = K + 8), sigmoid-scale and ELU arms, on a
    ragged 32-column block and an exact 96-column reflect block"""
    from umamd._lib import tuning
    with tuning(halo_min_tiles=1):
        assert _halo_ok(case, epi) == 1
        _Fwd(case).check_outputs('epilogue', epi)


# zero-pad stride-1 data gradient (FLIP arm), bf16 dx of ld = C + 8
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', HC.DGRAD_CASES)
def test_dgrad(case, accumulate):
    from umamd import functional as U
    from umamd._lib import PAD_ZERO, UM_BF16, EPI_NONE, call, ptr, query, tuning
    C, K, R, H, W, resident = case
    pad = (R - 1) // 2
    op = HC.dgrad_operands(case)
    dy = _guarded_nhwc(op['dy'], R)
    _, wT = U._pack(op['w'].to(DEV), C, BF16, wf=False)
    ldx = C + HC.OUT_GUARD
    dx = torch.full((HC.N, H, W, ldx), SENT, dtype=BF16, device=DEV)
    ref = op['ref']
    if accumulate:
        dx[..., :C] = op['prev'].permute(0, 2, 3, 1).to(BF16)
        ref = ref + op['prev'].double()
    keys = dict(halo_min_tiles=1)
    if resident:
        keys.update(halo_pf2=0, halo_res_kb=48, halo_grid=3)
    with tuning(**keys):
        assert query('um_conv_halo_ok', UM_BF16, HC.N, H, W, C, K, R, 1, pad, PAD_ZERO, H, W,
                     EPI_NONE, 1) == 1
        wsb = query('um_conv_dgrad_ws_pad', UM_BF16, HC.N, H, W, C, R, K, 1, pad, PAD_ZERO)
        ws = torch.empty((wsb // 4,), dtype=F32, device=DEV) if wsb else None
        call('um_conv2d_dgrad', UM_BF16, HC.N, H, W, C, ldx, ptr(dx), accumulate, ptr(wT), K, R, 1,
             pad, PAD_ZERO, H, W, ptr(dy), K, ptr(ws), wsb)
        torch.cuda.synchronize()
    assert bool((dx[..., C:] == SENT).all()), 'dx padding columns written'
    rb = HC.bf16_ratio(_nchw(dx[..., :C]), ref)
    print(f'halo_conv dgrad {case} accumulate={accumulate}: bf16 err/bound {rb:.3f}')
    assert rb <= 1.0, rb
