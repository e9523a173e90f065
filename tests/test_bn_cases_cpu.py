"""The acceptance criteria of tests/test_gpu_bn.py have teeth, and its tables
reach every arm they name.  No GPU: each bar is evaluated with the f64
reference in the kernel's place (rounded the way the kernel stores it: must
pass) and against deliberately wrong references, each of which must fail on
every case of its table:
  the last row dropped from a sum; the last 8-channel group zeroed; rows of a
  straddling block given the first image's add_nc; ELU' taken at z of the
  neighbouring channel; biased instead of unbiased running variance; count off
  by one; slot 15 ignored; momentum applied to the old value; one merge source
  skipped; one column-reduction part row skipped; SE ReLU gate ignored.
The reach test uses the library's host queries (no device needed) and the
documented plan of bn_slices, so a later change of a plan constant that moves
a case out of its arm fails here instead of the coverage silently shrinking.
"""
import pytest
import torch

import _bn_cases as B
from umamd._lib import query, tuning

BN_CASES = sorted(set(B.PLAIN_CASES + B.SE_CASES + B.ROWS_MAX_CASES))


def _bf16(t):
    return t.to(torch.bfloat16).double()


def _zero_last_group(t):
    t = t.clone()
    t[..., -8:] = 0
    return t


def _ids(c):
    return '-'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('case', BN_CASES + [B.COND_CASE + ('cond',)], ids=_ids)
def test_forward_bar(case, mode):
    """forward a, f32 and bf16 stores, ELU on and off; pool sums of the stored a"""
    op = B.bn_operands(case[:4], mode, len(case) == 5)
    for elu in (1, 0):
        ref = B.fwd_ref(op['y'], op['scale'], op['shift'], elu)
        for bf16, stored in ((False, ref.float().double()), (True, _bf16(ref))):
            bound = B.fwd_bound(op['y'], op['scale'], op['shift'], ref, bf16)
            assert B.ok(stored, ref, bound), (case, elu, bf16)
            assert not B.ok(_zero_last_group(stored), ref, bound), (case, elu, bf16)
            # per-image sums of the stored a: a dropped row is seen
            R = B.fwd_rows_c(op['M'], op['HW'], op['C'])
            sums, sb = B.image_sums(stored, op), B.image_sum_bound(stored, op, R)
            short = stored.clone()
            short[-1] = 0
            assert B.ok(sums, sums, sb)
            assert not B.ok(B.image_sums(short, op), sums, sb), (case, elu, bf16)


def _bwd(op, use_add, elu, R, **mut):
    """sums and dy of the backward (k1..k3 from the unmutated sums, as f32)"""
    good = B.bwd_sums_ref(op, use_add, elu, R)
    k, _ = B.bwd_coeffs_ref(good['s0'], good['s1'], op['M'], op['gamma'], op['invstd'])
    k = {n: v.float() for n, v in k.items()}
    r = B.bwd_sums_ref(op, use_add, elu, R, **mut) if mut else good
    good_dy = B.dy_ref(op, good['dz'], k['k1'], k['k2'], k['k3'])
    r['dy'] = B.dy_ref(op, r['dz'], k['k1'], k['k2'], k['k3'])
    r['dyb'] = lambda bf16: B.dy_bound(op, good['dz'], good['dzb'], k['k1'], k['k2'], k['k3'],
                                       good_dy, bf16)
    return r


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('case', BN_CASES + [B.COND_CASE + ('cond',)], ids=_ids)
def test_backward_bars(case, mode):
    """dz sums and dy: the reference passes; a dropped last row, a zeroed last
    channel group and ELU' of the neighbouring channel fail"""
    op = B.bn_operands(case[:4], mode, len(case) == 5)
    R = B.bwd_rows(op['M'])
    for use_add in (0, 1):
        for elu in (1, 0):
            g = _bwd(op, use_add, elu, R)
            assert B.ok(g['s0'], g['s0'], g['b0']) and B.ok(g['s1'], g['s1'], g['b1'])
            d = _bwd(op, use_add, elu, R, drop_last=True)
            assert not B.ok(d['s0'], g['s0'], g['b0']), (case, use_add, elu)
            assert not B.ok(d['s1'], g['s1'], g['b1']), (case, use_add, elu)
            assert not B.ok(_zero_last_group(g['s0']), g['s0'], g['b0'])
            assert not B.ok(_zero_last_group(g['s1']), g['s1'], g['b1'])
            for bf16, stored in ((False, g['dy'].float().double()), (True, _bf16(g['dy']))):
                bound = g['dyb'](bf16)
                assert B.ok(stored, g['dy'], bound), (case, use_add, elu, bf16)
                assert not B.ok(_zero_last_group(stored), g['dy'], bound)
                # sum dy of the stored values (the conv-bias gradient partials)
                sb = B.stored_sum_bound(stored, R)
                assert not B.ok(stored[:-1].sum(0), stored.sum(0), sb), (case, bf16)
                if elu:
                    n = _bwd(op, use_add, elu, R, z_shift=1)
                    stored_n = _bf16(n['dy']) if bf16 else n['dy'].float().double()
                    assert not B.ok(stored_n, g['dy'], bound), (case, use_add, bf16)
            if elu:
                n = _bwd(op, use_add, elu, R, z_shift=1)
                assert not B.ok(n['s0'], g['s0'], g['b0']), (case, use_add)
                assert not B.ok(n['s1'], g['s1'], g['b1']), (case, use_add)


STRADDLING = [(c, r) for c in sorted(set(B.SE_CASES + B.ROWS_MAX_CASES))
              for r in sorted({B.bwd_rows(c[0] * c[1] * c[2]),
                               B.bwd_rows(c[0] * c[1] * c[2], B.ROWS_MAX_KNOB),
                               B.bwd_rows_c(c[0] * c[1] * c[2], c[3], True)})
              if B.straddles(c[0] * c[1] * c[2], c[1] * c[2], r)]


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('case,rows', STRADDLING, ids=_ids)
def test_straddling_block_with_first_images_vector_fails(case, rows, mode):
    """add_nc with one_img == false: rows of a block that straddles two images
    given the first image's SE vector fail the sums and the dy bars"""
    op = B.bn_operands(case, mode)
    wrong = B.add_rows(op, 1, first_image_rows=rows)
    assert not torch.equal(wrong, B.add_rows(op, 1))
    for elu in (1, 0):
        g = _bwd(op, 1, elu, rows)
        w = _bwd(op, 1, elu, rows, ad=wrong)
        assert not B.ok(w['s0'], g['s0'], g['b0']), (case, rows, elu)
        assert not B.ok(w['s1'], g['s1'], g['b1']), (case, rows, elu)
        assert not B.ok(w['dy'].float(), g['dy'], g['dyb'](False)), (case, rows, elu)
        assert not B.ok(_bf16(w['dy']), g['dy'], g['dyb'](True)), (case, rows, elu)


def _coeff_mutants(s0, s1, count, gamma, beta, rm, rv, slots):
    """(name, coefficients) of the wrong statistics"""
    m0, m1 = B.slot_sums(slots, s0.numel())
    return [('biased', B.coeffs_ref(s0, s1, count, gamma, beta, rm, rv, biased=True)),
            ('count', B.coeffs_ref(s0, s1, count + 1, gamma, beta, rm, rv)),
            ('slot15', B.coeffs_ref(m0, m1, count, gamma, beta, rm, rv)),
            ('momentum', B.coeffs_ref(s0, s1, count, gamma, beta, rm, rv, mom_on_old=True))]


@pytest.mark.parametrize('mode', ['f32', 'bf16y'])
@pytest.mark.parametrize('case', BN_CASES, ids=_ids)
def test_coefficient_bars(case, mode):
    """mean / invstd / scale / shift and the running statistics from the
    slots: the f32 rounding passes; biased running variance, count off by
    one, slot 15 ignored and momentum on the old value fail"""
    op = B.bn_operands(case, mode)
    yd = op['y'].double()
    for count in (op['M'], op['M'] + 19):  # the second: a count read after the slots
        slots = B.make_slots(yd, yd * yd, count)
        s0, s1 = B.slot_sums(slots, op['C'])
        co = B.coeffs_ref(s0, s1, count, op['gamma'], op['beta'], op['rm'], op['rv'])
        cb = B.coeffs_bounds(co)
        for k in cb:
            assert B.ok(co[k].float(), co[k], cb[k]), (case, k)
            assert not B.ok(_zero_last_group(co[k].float()), co[k], cb[k]), (case, k)
        if count == op['M']:  # the clamp's channel
            assert float(co['var'][B.CONST_CH]) < 1e-12
            assert abs(float(co['invstd'][B.CONST_CH]) * B.EPS ** 0.5 - 1) < 1e-6
        short = B.make_slots(yd, yd * yd, count, skip=15)
        assert bool((slots[:-1].reshape(16, -1).abs().sum(1) > 0).all()), case
        for name, mu in _coeff_mutants(s0, s1, count, op['gamma'], op['beta'], op['rm'], op['rv'],
                                       short):
            keys = ('rv',) if name == 'biased' else ('rm', 'rv') if name == 'momentum' else cb
            bad = [k for k in keys if not B.ok(mu[k].float(), co[k], cb[k])]
            assert bad and (name not in ('biased', 'momentum') or len(bad) == len(keys)), \
                (case, name, bad)


@pytest.mark.parametrize('C', B.COEFF_C)
def test_backward_coefficient_bars(C):
    """k1..k3, dgamma, dbeta: count off by one and a zeroed channel group fail"""
    op = B.colred_operands(17, C, 2)
    s, _ = B.colred_ref(op['parts'], C, 2)
    k, kb = B.bwd_coeffs_ref(s[:, 0], s[:, 1], op['count'], op['gamma'], op['invstd'])
    wrong, _ = B.bwd_coeffs_ref(s[:, 0], s[:, 1], op['count'] + 1, op['gamma'], op['invstd'])
    for n in k:
        assert B.ok(k[n].float(), k[n], kb[n])
        assert not B.ok(_zero_last_group(k[n].float()), k[n], kb[n])
    assert not B.ok(wrong['k2'].float(), k['k2'], kb['k2'])
    assert not B.ok(wrong['k3'].float(), k['k3'], kb['k3'])


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('nsrc,self_,widx', B.MERGE_CASES)
@pytest.mark.parametrize('case', B.MERGE_SHAPES, ids=_ids)
def test_merge_bar(case, nsrc, self_, widx, mode):
    """the fused merge: every source skipped in turn fails"""
    mo = B.merge_operands(case, mode, nsrc)
    srcs = list(mo['src'])
    ref, mag = B.merge_ref(srcs, mo['w'], widx)
    bf16 = mode != 'f32'
    bound = B.merge_bound(ref, mag, nsrc, bf16)
    assert B.ok(_bf16(ref) if bf16 else ref.float(), ref, bound)
    for skip in range(nsrc):
        mut, _ = B.merge_ref(srcs, mo['w'], widx, skip=skip)
        assert not B.ok(_bf16(mut) if bf16 else mut.float(), ref, bound), (case, nsrc, skip)


COLRED = [(n, c) for n in B.COLRED_NPARTS for c in B.COLRED_C]


@pytest.mark.parametrize('nparts,C', COLRED)
def test_column_reduction_bar(nparts, C):
    """one part row skipped fails the f64 and the f32 output bars"""
    for nv, stride in ((2, None), (1, None)) + (((1, B.COLRED_ROWS_EXTRA[1]),) if C == 512 else ()):
        cc = B.COLRED_ROWS_EXTRA[0] if stride else C
        op = B.colred_operands(nparts, cc, nv, stride)
        ref, b = B.colred_ref(op['parts'], cc, nv)
        mut, _ = B.colred_ref(op['parts'], cc, nv, skip_last=True)
        assert B.ok(ref, ref, b) and not B.ok(mut, ref, b)
        fb = B.f32_out_bound(ref, b)
        assert B.ok(ref.float(), ref, fb) and not B.ok(mut.float(), ref, fb)
        prev = op['prev'].double()[:, None]
        fb = B.f32_out_bound(ref + prev, b, op['prev'][:, None])
        assert B.ok((ref + prev).float(), ref + prev, fb)
        assert not B.ok((mut + prev).float(), ref + prev, fb)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('C', B.MEAN_C)
@pytest.mark.parametrize('S', B.MEAN_S)
def test_channel_mean_bar(S, C, bf16):
    x = B.mean_operands(S, C, bf16)
    ref, b = B.mean_ref(x)
    mut, _ = B.mean_ref(x, drop_last=True)
    assert B.ok(ref.float(), ref, b + 2 * B.U * ref.abs())
    assert not B.ok(mut.float(), ref, b + 2 * B.U * ref.abs())
    assert not B.ok(_zero_last_group(ref.float()), ref, b + 2 * B.U * ref.abs())


@pytest.mark.parametrize('N', B.SE_N)
@pytest.mark.parametrize('C,R', B.SE_CR)
def test_se_bars(C, R, N):
    """dead ReLU rows are exactly 0 and no pre-activation is within 1e-3 of 0
    (on the f64 reference); the written-out backward equals f64 autograd; the
    ReLU gate ignored fails the dz, dw1 and dpool bars"""
    for ppi in B.SE_PARTS:
        op = B.se_operands(C, R, N, ppi)
        assert float(op['pre'].abs().min()) > 1e-3
        assert torch.equal(op['pre'] > 0, B.se_signs(N, R) > 0)
        assert bool((op['z1'] == 0).any()) and (N * R == 1 or bool((op['z1'] > 0).any()))
        for k in ('pooled', 'z1', 's'):
            assert B.ok(op[k].float(), op[k], op[k + '_b'] + B.U * op[k].abs()), (C, R, N, ppi, k)
    op = B.se_operands(C, R, N)
    ex, ag = B.se_bwd_ref(op, exact_inputs=True), B.se_bwd_autograd(op)
    for k in ('dw1', 'dw2'):
        assert float((ex[k] - ag[k]).abs().max()) <= 1e-12 * max(1.0, float(ag[k].abs().max()))
    assert float((ex['dpool'] - ag['dpool'] * op['inv_hw']).abs().max()) <= 1e-12
    ref, mut = B.se_bwd_ref(op), B.se_bwd_ref(op, gate=False)
    for k in ('dz', 'dw1', 'dw2', 'dpool'):
        assert B.ok(ref[k].float(), ref[k], ref[k + '_b'] + B.U * ref[k].abs()), (C, R, N, k)
    for k in ('dz', 'dw1', 'dpool'):
        assert not B.ok(mut[k].float(), ref[k], ref[k + '_b'] + B.U * ref[k].abs()), (C, R, N, k)


def test_tables_reach_every_arm():
    """the host queries and the documented bn_slices plan put the cases in the
    arms they are named for"""
    # rows per backward block: the library's partial-row count is the plan's
    for N, H, W, C in BN_CASES:
        M = N * H * W
        assert query('um_bn_bwd_parts', M) == B.ceil_div(M, B.bwd_rows(M)), M
    se = [(c, B.bwd_rows(c[0] * c[1] * c[2])) for c in B.SE_CASES]
    assert any(B.straddles(c[0] * c[1] * c[2], c[1] * c[2], r) for c, r in se)
    assert any(not B.straddles(c[0] * c[1] * c[2], c[1] * c[2], r) for c, r in se)
    # a block that spans three images
    assert any(r >= 2 * c[1] * c[2] for c, r in se)
    # bn_bwd_rows_max = 64 changes the plan of one case, and that case straddles
    big = [c for c in B.ROWS_MAX_CASES
           if B.bwd_rows(c[0] * c[1] * c[2]) != B.bwd_rows(c[0] * c[1] * c[2], B.ROWS_MAX_KNOB)]
    assert big
    for N, H, W, C in big:
        M = N * H * W
        with tuning(bn_bwd_rows_max=B.ROWS_MAX_KNOB):
            assert query('um_bn_bwd_parts', M) == B.ceil_div(M, B.ROWS_MAX_KNOB)
        assert query('um_bn_bwd_parts', M) == B.ceil_div(M, B.bwd_rows(M))
        assert B.straddles(M, H * W, B.ROWS_MAX_KNOB)
    # channel slices: sliced cases, unsliced ones with C >= 128, several row
    # blocks per slice; the forward's pool rows follow the same plan
    for c in B.SLICED_CASES:
        assert B.bn_slices(c[0] * c[1] * c[2], c[3])[1] > 1, c
    assert any(c[3] >= 128 and B.bn_slices(c[0] * c[1] * c[2], c[3])[1] == 1 for c in B.PLAIN_CASES)
    assert any(B.bwd_rows_c(c[0] * c[1] * c[2], c[3], True) < c[0] * c[1] * c[2]
               for c in B.SLICED_CASES)
    differs = False
    for N, H, W, C in sorted(set(B.POOL_CASES + B.SE_CASES)):
        M, HW = N * H * W, H * W
        for on in (1, 0):
            with tuning(bn_slice=on):
                parts = query('um_bn_fwd_pool_parts_c', M, HW, C)
            assert parts == M // B.fwd_rows_c(M, HW, C, bool(on)), (N, H, W, C, on)
        differs |= B.fwd_rows_c(M, HW, C, True) != B.fwd_rows_c(M, HW, C, False)
    assert differs
    assert {c[1] * c[2] for c in B.POOL_CASES} >= {35, 96, 6}
    # RowMap: a group count that divides 64, does not, and exceeds 256
    groups = {c[3] // 8 for c in B.PLAIN_CASES}
    assert any(64 % g == 0 and g < 64 for g in groups) and {3, 5, 17} <= groups
    assert any(g > 256 for g in groups)
    # column reductions: one workgroup by default up to 128K values, the ticket
    # form with at least 33 workgroups under the test's tuning, and the
    # workspace follows
    assert sum(B.colred_blocks(n, c, 2) == 1 for n, c in COLRED) >= len(COLRED) - 2
    most = 0
    for nparts, C in COLRED:
        for nv in (1, 2):
            assert query('um_colred_ws', nparts, C, nv) == B.colred_blocks(nparts, C, nv) * C * nv * 8
            with tuning(**B.COLRED_TICKET):
                ws = query('um_colred_ws', nparts, C, nv)
            blocks = B.colred_blocks(nparts, C, nv, **{k[7:]: v for k, v in B.COLRED_TICKET.items()})
            assert ws == blocks * C * nv * 8, (nparts, C, nv)
            most = max(most, blocks)
    assert most >= 33
    # channel mean: one chunk, a chunk boundary, a one-pixel tail chunk
    assert {B.ceil_div(s, B.MEAN_PIX) for s in B.MEAN_S} >= {1, 2, 3}
    # the SE pool loop: parts_per_image reaches its 8-way unrolled body for
    # every lane count (8 * 256 / min(C, 256) <= 300 only for C >= 8: L <= 32)
    assert any(p >= 8 * (256 // min(c, 256)) for p in B.SE_PARTS for c, _ in B.SE_CR)
    assert any(r % 4 for _, r in B.SE_CR) and any(r > 256 for _, r in B.SE_CR)
