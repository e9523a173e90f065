"""The BatchNorm+ELU passes (csrc/bn.hip), the column reductions
(csrc/reduce.hip) and the SE kernels (csrc/decoder.hip) against f64 references
on exact operands, entry by entry through the C ABI.  Tables, references and
per-element bars are in tests/_bn_cases.py (tests/test_bn_cases_cpu.py shows
that the bars reject a subtly wrong kernel); every comparison prints its
ratio max(|got - ref| / bound) before the test asserts it <= 1.

Arms reached here and by no other test: the SE-gradient vector of a block
that straddles two images (add_nc, one_img == false); the multi-workgroup
last-arriver finish of colred_* (ticket, reset, publish_finish); the scalar
column reduction (misaligned base, rowstride % 4 != 0, NV = 1 with
accumulate); bn_slice on and off, bn_bwd_rows_max; RowMap group counts that
do not divide 64 or exceed 256 (the g0 loop); count <= 0; accumulate and
stats_local of um_bn_bwd_coeffs; ld != C; a bf16 pre-BN y (UM_Y_ACT);
um_channel_mean, um_se_mlp_fwd, um_se_mlp_bwd."""
import ctypes

import pytest
import torch

import _bn_cases as B
from umamd._lib import UM_BF16, UM_F32, Y_ACT, UmamdError, call, ptr, query, tuning

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = 7.0   # exact in bf16; fills output guards
GUARD = 2    # sentinel rows after the last real row
NAN = float('nan')
U = B.U


def _ids(c):
    return '-'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def _types(mode):
    """-> (dtype code, activation dtype, dtype of y)"""
    if mode == 'f32':
        return UM_F32, torch.float32, torch.float32
    if mode == 'bf16':
        return UM_BF16, torch.bfloat16, torch.float32
    return UM_BF16 | Y_ACT, torch.bfloat16, torch.bfloat16


def _in(t, dt, ld=None):
    """[M][C] -> device [M][ld] of dtype dt, NaN in the columns past C"""
    M, C = t.shape
    buf = torch.full((M, ld or C), NAN, dtype=dt, device=DEV)
    buf[:, :C] = t.to(DEV).to(dt)
    return buf


def _out(M, C, dt, ld=None, fill=SENT):
    return torch.full((M + GUARD, ld or C), fill, dtype=dt, device=DEV)


def _same(t, fill):
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


def _res(buf, M, C, fill=SENT):
    """the M x C result on the CPU (f64); the guard columns and rows untouched"""
    torch.cuda.synchronize()
    assert _same(buf[:M, C:], fill), 'sentinel columns overwritten'
    assert _same(buf[M:], fill), 'sentinel rows overwritten'
    return buf[:M, :C].double().cpu()


def _vec(C, dt=torch.float32, fill=SENT):
    return torch.full((C + 8,), fill, dtype=dt, device=DEV)


def _vres(buf, C, fill=SENT):
    torch.cuda.synchronize()
    assert _same(buf[C:], fill), 'sentinel after a vector overwritten'
    return buf[:C].double().cpu()


_KEEP = []  # device inputs stay allocated until their test has finished


def _d(t, dt=torch.float32):
    _KEEP.append(t.to(dt).to(DEV).contiguous())
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_inputs():
    """a device error ends the session: nothing more is launched after it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)
    _KEEP.clear()


class Checks:
    """collects the comparisons of a test: each prints its ratio, done()
    asserts that none exceeded 1"""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def __call__(self, name, got, ref, bound):
        r = B.ratio(got, ref, bound)
        print(f'{self.tag} {name}: ratio {r:.3f}')
        if not r <= 1.0:
            self.bad.append((name, r))
        return r

    def equal(self, name, a, b):
        same = torch.equal(a, b)
        print(f'{self.tag} {name}: bit-equal {same}')
        if not same:
            self.bad.append((name, 'not bit-equal'))

    def true(self, name, cond):
        if not cond:
            print(f'{self.tag} {name}: FALSE')
            self.bad.append((name, False))

    def done(self):
        assert not self.bad, (self.tag, self.bad)


def _lds(C, ld):
    """(ldy, lda = lddy = ldda)"""
    return (C + 8, C + 16) if ld else (C, C)


def _pool_buf(op, pool):
    if not pool:
        return None, 0
    rows = query('um_bn_fwd_pool_parts_c', op['M'], op['HW'], op['C'])
    return _out(rows, op['C'], torch.float32, fill=NAN), rows


def _check_pool(ck, op, pool, rows, got_a, R):
    """the announced rows are all written and no more; per-image sums of the
    stored a within the sums bar"""
    p = _res(pool, rows, op['C'], NAN)
    ck.true('pool rows written', bool(torch.isfinite(p).all()))
    ck.true('pool rows = M / rows per block', rows == op['M'] // R)
    per = p.reshape(op['N'], rows // op['N'], op['C']).sum(1)
    ck('pool sums', per, B.image_sums(got_a, op), B.image_sum_bound(got_a, op, R))


# ------------------------------------------------------------- forward ----
FWD = ([(c, 0, 0, 0) for c in B.PLAIN_CASES] + [(c, 1, 0, 0) for c in B.LD_CASES] +
       [(c, 0, 1, 0) for c in B.POOL_CASES] + [(B.COND_CASE, 0, 0, 1)])


def _fwd_id(p):
    c, ld, pool, cond = p
    return _ids(c) + ('-ld' if ld else '') + ('-pool' if pool else '') + ('-offset64' if cond else '')


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('p', FWD, ids=_fwd_id)
def test_bn_elu_fwd(p, mode):
    """um_bn_elu_fwd with given f32 scale / shift: a within the term-based
    bar, ELU on and off, ld != C with guards, pool partial rows.  The
    offset-64 case prints its ratio against the well-conditioned bound."""
    case, ld, pool, cond = p
    op = B.bn_operands(case, mode, bool(cond))
    code, act, yt = _types(mode)
    M, C = op['M'], op['C']
    ldy, lda = _lds(C, ld)
    ck = Checks(f'fwd {_fwd_id(p)} {mode}')
    y, sc, sh = _in(op['y'], yt, ldy), _d(op['scale']), _d(op['shift'])
    for elu in (1, 0):
        a = _out(M, C, act, lda)
        pb, rows = _pool_buf(op, pool)
        call('um_bn_elu_fwd', code, M, C, ptr(y), ldy, ptr(sc), ptr(sh), ptr(a), lda, elu,
             op['HW'] if pool else 0, ptr(pb))
        got = _res(a, M, C)
        ref = B.fwd_ref(op['y'], op['scale'], op['shift'], elu)
        ck(f'a elu={elu}', got, ref, B.fwd_bound(op['y'], op['scale'], op['shift'], ref,
                                                 act == torch.bfloat16))
        if pool:
            _check_pool(ck, op, pb, rows, got, B.fwd_rows_c(M, op['HW'], C))
        if cond and act == torch.float32:
            r = B.ratio(got, ref, B.fwd_wellcond_bound(op, ref))
            print(f'CONDITIONING fwd offset-64 elu={elu}: {r:.1f} x the well-conditioned bound')
    ck.done()


def _run_fwd_slots(op, mode, ld, pool, count, elu, merge=None):
    """one launch of um_bn_elu_fwd_slots (or _merge) -> dict of CPU results"""
    code, act, yt = _types(mode)
    M, C = op['M'], op['C']
    ldy, lda = _lds(C, ld)
    yd = op['y'].double()
    stored = M if count > 0 else M + 19  # count <= 0: read after the slots, != M as after SyncBN
    slots = _d(B.make_slots(yd, yd * yd, stored), torch.float64)
    y = _in(op['y'], yt, ldy)
    g, b = _d(op['gamma']), _d(op['beta'])
    rm, rv = _vec(C), _vec(C)
    rm[:C], rv[:C] = _d(op['rm']), _d(op['rv'])
    nbt = torch.tensor([5, 77], dtype=torch.int64, device=DEV)
    outs = {k: _vec(C) for k in ('mean', 'invstd', 'scale', 'shift')}
    a = _out(M, C, act, lda)
    head = (code, M, C, ptr(y), ldy, ptr(slots), float(count), ptr(g), ptr(b), B.EPS, B.MOM,
            ptr(rm), ptr(rv), ptr(nbt), ptr(outs['mean']), ptr(outs['invstd']),
            ptr(outs['scale']), ptr(outs['shift']), ptr(a), lda, elu)
    r = dict(count=stored)
    if merge is None:
        pb, rows = _pool_buf(op, pool)
        call('um_bn_elu_fwd_slots', *head, op['HW'] if pool else 0, ptr(pb))
        r.update(pool=pb, rows=rows)
    else:
        nsrc, self_, widx, srcs, w, merged = merge
        arr = (ctypes.c_void_p * nsrc)(*[None if i == self_ else ptr(s) for i, s in enumerate(srcs)])
        wi = (ctypes.c_int * nsrc)(*widx)
        call('um_bn_elu_fwd_slots_merge', *head, nsrc, arr, wi, ptr(w), self_, ptr(merged))
    r['a'] = _res(a, M, C)
    for k, v in outs.items():
        r[k] = _vres(v, C)
    r['rm'], r['rv'] = _vres(rm, C), _vres(rv, C)
    r['nbt'] = nbt.cpu().tolist()
    return r


def _check_fwd_slots(ck, op, mode, r, elu, tag=''):
    """published coefficients and running statistics against f64 from the same
    sums, updated exactly once; a against the published scale / shift"""
    yd = op['y'].double()
    co = B.coeffs_ref(yd.sum(0), (yd * yd).sum(0), r['count'], op['gamma'], op['beta'],
                      op['rm'], op['rv'])
    cb = B.coeffs_bounds(co)
    for k in cb:
        ck(tag + k, r[k], co[k], cb[k])
    ck.true(tag + 'num_batches_tracked once', r['nbt'] == [6, 77])
    ref = B.fwd_ref(op['y'], r['scale'], r['shift'], elu)
    ck(tag + f'a elu={elu}', r['a'], ref,
       B.fwd_bound(op['y'], r['scale'], r['shift'], ref, mode != 'f32'))


FWD_SLOTS = ([(c, 0, 0) for c in B.PLAIN_CASES] + [(c, 1, 0) for c in B.LD_CASES] +
             [(c, 0, 1) for c in B.POOL_CASES])


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('p', FWD_SLOTS, ids=lambda p: _fwd_id(p + (0,)))
def test_bn_elu_fwd_slots(p, mode):
    """um_bn_elu_fwd_slots: coefficients from the f64 slots (count given and
    count = -1 read after the slots), running statistics and
    num_batches_tracked exactly once also with several channel slices and row
    blocks, bn_slice=1 and bn_slice=0 with bit-equal coefficient outputs."""
    case, ld, pool = p
    op = B.bn_operands(case, mode)
    ck = Checks(f'fwd_slots {_fwd_id(p + (0,))} {mode}')
    sliced = B.bn_slices(op['M'], op['C'])[1] > 1
    for count, elu in ((op['M'], 1), (-1, 0)):
        res = {}
        for on in (1, 0) if sliced else (1,):
            with tuning(bn_slice=on):
                r = _run_fwd_slots(op, mode, ld, pool, count, elu)
                tag = f'count={count} bn_slice={on} '
                _check_fwd_slots(ck, op, mode, r, elu, tag)
                if pool:
                    _check_pool(ck, op, r['pool'], r['rows'], r['a'],
                                B.fwd_rows_c(op['M'], op['HW'], op['C'], bool(on)))
            res[on] = r
        if sliced:
            for k in ('mean', 'invstd', 'scale', 'shift', 'rm', 'rv'):
                ck.equal(f'count={count} {k} bn_slice 1 vs 0', res[1][k], res[0][k])
    ck.done()


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('nsrc,self_,widx', B.MERGE_CASES)
@pytest.mark.parametrize('case', B.MERGE_SHAPES, ids=_ids)
def test_bn_elu_fwd_slots_merge(case, nsrc, self_, widx, mode):
    """the fused merge of the next node: a and the coefficients as in the
    unmerged entry, merged within its bar of the f64 merge of the stored
    sources (self = the a just stored)."""
    op = B.bn_operands(case, mode)
    mo = B.merge_operands(case, mode, nsrc)
    code, act, yt = _types(mode)
    M, C = op['M'], op['C']
    ck = Checks(f'merge {_ids(case)} nsrc={nsrc} self={self_} {mode}')
    srcs = [_in(mo['src'][i], act) for i in range(nsrc)]
    merged = _out(M, C, act)
    r = _run_fwd_slots(op, mode, 0, 0, M, 1, (nsrc, self_, widx, srcs, _d(mo['w']), merged))
    _check_fwd_slots(ck, op, mode, r, 1)
    plain = _run_fwd_slots(op, mode, 0, 0, M, 1)
    for k in ('a', 'mean', 'invstd', 'scale', 'shift', 'rm', 'rv'):
        ck.equal(f'{k} as the unmerged entry', r[k], plain[k])
    stored = [r['a'] if i == self_ else mo['src'][i] for i in range(nsrc)]
    ref, mag = B.merge_ref(stored, mo['w'], widx)
    ck('merged', _res(merged, M, C), ref, B.merge_bound(ref, mag, nsrc, act == torch.bfloat16))
    ck.done()


def test_bn_elu_fwd_slots_merge_refuses():
    """a null source other than self, nsrc = 1 and nsrc = 9 return an error
    on the host, before any launch: every output keeps its sentinel"""
    case, mode = B.MERGE_SHAPES[0], 'f32'
    op = B.bn_operands(case, mode)
    M, C = op['M'], op['C']
    mo = B.merge_operands(case, mode, 8)
    srcs = [_in(mo['src'][i % 8], torch.float32) for i in range(9)]
    for nsrc, null in ((1, None), (9, None), (3, 2)):
        merged = _out(M, C, torch.float32)
        use = [None if i == null else s for i, s in enumerate(srcs[:nsrc])]

        class _S:  # ptr() of a null source
            def data_ptr(self):
                return None
        use = [s if s is not None else _S() for s in use]
        with pytest.raises(UmamdError):
            _run_fwd_slots(op, mode, 0, 0, M, 1, (nsrc, 0, tuple(range(nsrc)), use, _d(mo['w']),
                                                 merged))
        torch.cuda.synchronize()
        assert bool((merged == SENT).all()), (nsrc, null)


# ------------------------------------------------------------ backward ----
# (case, ld, add_nc, bn_bwd_rows_max knob, offset 64)
BWD = ([(c, 0, 0, 0, 0) for c in B.PLAIN_CASES] + [(c, 1, 1, 0, 0) for c in B.LD_CASES] +
       [(c, 0, 1, 0, 0) for c in B.SE_CASES] + [(c, 0, 1, 1, 0) for c in B.ROWS_MAX_CASES] +
       [(B.COND_CASE, 0, 0, 0, 1)])


def _bwd_id(p):
    c, ld, add, knob, cond = p
    return (_ids(c) + ('-ld' if ld else '') + ('-add_nc' if add else '') +
            (f'-rows_max{B.ROWS_MAX_KNOB}' if knob else '') + ('-offset64' if cond else ''))


def _knob(p):
    return tuning(bn_bwd_rows_max=B.ROWS_MAX_KNOB) if p[3] else tuning()


def _bwd_inputs(op, mode, ld, add):
    code, act, yt = _types(mode)
    ldy, lda = _lds(op['C'], ld)
    return dict(code=code, act=act, ldy=ldy, lda=lda, y=_in(op['y'], yt, ldy),
                da=_in(op['da'], act, lda), add=_d(op['add']) if add else None,
                co=[_d(op[k]) for k in ('mean', 'invstd', 'scale', 'shift')])


def _bwd_head(op, d):
    return (d['code'], op['M'], op['C'], op['HW'], ptr(d['da']), d['lda'], ptr(d['y']), d['ldy'],
            *[ptr(t) for t in d['co']], ptr(d['add']))


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('p', BWD, ids=_bwd_id)
def test_bn_elu_bwd_reduce(p, mode):
    """um_bn_elu_bwd_reduce (partial rows) and um_bn_elu_bwd_reduce_slots (f64
    slots, count stored after them): sum dz and sum dz*xhat within the sums
    bar.  With add_nc the blocks straddle two images (HW = 35, one_img ==
    false), span three (HW = 6) or neither (HW = 96); bn_bwd_rows_max = 64;
    bn_slice on and off for the slots entry."""
    case, ld, add, knob, cond = p
    op = B.bn_operands(case, mode, bool(cond))
    M, C = op['M'], op['C']
    cap = B.ROWS_MAX_KNOB if knob else 1024
    ck = Checks(f'bwd_reduce {_bwd_id(p)} {mode}')
    d = _bwd_inputs(op, mode, ld, add)
    with _knob(p):
        for elu in (1, 0):
            R = B.bwd_rows(M, cap)
            ref = B.bwd_sums_ref(op, add, elu, R)
            nparts = query('um_bn_bwd_parts', M)
            ck.true('parts = ceil(M / rows)', nparts == B.ceil_div(M, R))
            parts = _out(nparts, 2 * C, torch.float32, fill=NAN)
            call('um_bn_elu_bwd_reduce', *_bwd_head(op, d), elu, ptr(parts))
            got = _res(parts, nparts, 2 * C, NAN).reshape(nparts, C, 2)
            ck.true('every partial row written', bool(torch.isfinite(got).all()))
            ck(f'sum dz elu={elu}', got[:, :, 0].sum(0), ref['s0'], ref['b0'])
            ck(f'sum dz*xhat elu={elu}', got[:, :, 1].sum(0), ref['s1'], ref['b1'])
            for on in (1, 0) if B.bn_slices(M, C)[1] > 1 else (1,):
                with tuning(bn_slice=on):
                    Rs = B.bwd_rows_c(M, C, bool(on), cap)
                    refs = B.bwd_sums_ref(op, add, elu, Rs)
                    slots = torch.zeros(B.STAT_SLOTS * C * 2 + 1 + 8, dtype=torch.float64,
                                        device=DEV)
                    slots[-8:] = SENT
                    call('um_bn_elu_bwd_reduce_slots', *_bwd_head(op, d), elu, ptr(slots))
                    torch.cuda.synchronize()
                    sl = slots.cpu()
                    ck.true('slots guard', bool((sl[-8:] == SENT).all()))
                    ck.true('count after the slots = M', float(sl[-9]) == float(M))
                    s0, s1 = B.slot_sums(sl, C)
                    ck(f'slots sum dz elu={elu} bn_slice={on}', s0, refs['s0'], refs['b0'])
                    ck(f'slots sum dz*xhat elu={elu} bn_slice={on}', s1, refs['s1'], refs['b1'])
    ck.done()


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('p', BWD, ids=_bwd_id)
def test_bn_elu_bwd_apply(p, mode):
    """um_bn_elu_bwd_apply with given f32 k1..k3 (dy within the term-based
    bar, sum dy partial rows of the stored dy) and um_bn_elu_bwd_apply_slots
    (k1..k3 from the global slots; dgamma / dbeta from the global sums x
    dbias_scale without local_slots, from the local slots with them; the
    closed-form dbias; count = -1).  The offset-64 case prints its ratio
    against the well-conditioned bound."""
    case, ld, add, knob, cond = p
    op = B.bn_operands(case, mode, bool(cond))
    M, C = op['M'], op['C']
    cap = B.ROWS_MAX_KNOB if knob else 1024
    bf16 = mode != 'f32'
    ck = Checks(f'bwd_apply {_bwd_id(p)} {mode}')
    d = _bwd_inputs(op, mode, ld, add)
    with _knob(p):
        for elu in (1, 0):
            R = B.bwd_rows(M, cap)
            ref = B.bwd_sums_ref(op, add, elu, R)
            k, _ = B.bwd_coeffs_ref(ref['s0'], ref['s1'], M, op['gamma'], op['invstd'])
            k = {n: v.float() for n, v in k.items()}
            dyr = B.dy_ref(op, ref['dz'], k['k1'], k['k2'], k['k3'])
            dyb = B.dy_bound(op, ref['dz'], ref['dzb'], k['k1'], k['k2'], k['k3'], dyr, bf16)
            nparts = query('um_bn_bwd_parts', M)
            sums = _out(nparts, C, torch.float32, fill=NAN)
            dy = _out(M, C, d['act'], d['lda'])
            kd = [_d(k[n]) for n in ('k1', 'k2', 'k3')]
            call('um_bn_elu_bwd_apply', *_bwd_head(op, d), elu, *[ptr(t) for t in kd], ptr(dy),
                 d['lda'], ptr(sums))
            got = _res(dy, M, C)
            ck(f'dy elu={elu}', got, dyr, dyb)
            sp = _res(sums, nparts, C, NAN)
            ck.true('every sum dy row written', bool(torch.isfinite(sp).all()))
            ck(f'sum dy elu={elu}', sp.sum(0), got.sum(0), B.stored_sum_bound(got, R))
            if cond and not bf16:
                r = B.ratio(got, dyr, B.dy_wellcond_bound(op, ref['dz'], k['k1'], k['k2'], k['k3']))
                print(f'CONDITIONING dy offset-64 elu={elu}: {r:.1f} x the well-conditioned bound')
            dy = _out(M, C, d['act'], d['lda'])
            call('um_bn_elu_bwd_apply', *_bwd_head(op, d), elu, *[ptr(t) for t in kd], ptr(dy),
                 d['lda'], None)
            ck.equal('dy without sum parts', _res(dy, M, C), got)
            # the slots entry: this rank holds the rows of image 0, the global
            # sums are all rows; count given, or -1 with 2 M stored (two ranks)
            local_rows = (op['img'] == 0).double()[:, None]
            for count, local in ((M, False), (-1, True)):
                n = M if count > 0 else 2 * M
                gs = B.make_slots(ref['t0'], ref['t1'], n)
                ls = B.make_slots(ref['t0'] * local_rows, ref['t1'] * local_rows, n)
                ks, kb = B.bwd_coeffs_ref(ref['s0'], ref['s1'], n, op['gamma'], op['invstd'])
                ksf = {m: v.float() for m, v in ks.items()}
                dyr2 = B.dy_ref(op, ref['dz'], ksf['k1'], ksf['k2'], ksf['k3'])
                dyb2 = B.dy_bound(op, ref['dz'], ref['dzb'], ksf['k1'], ksf['k2'], ksf['k3'],
                                  dyr2, bf16)
                res = {}
                for on in (1, 0) if B.bn_slices(M, C)[1] > 1 else (1,):
                    with tuning(bn_slice=on):
                        dy = _out(M, C, d['act'], d['lda'])
                        o = {m: _vec(C) for m in ('dgamma', 'dbeta', 'dbias')}
                        call('um_bn_elu_bwd_apply_slots', *_bwd_head(op, d), elu,
                             ptr(_d(gs, torch.float64)), float(count),
                             ptr(_d(ls, torch.float64)) if local else None, ptr(_d(op['gamma'])),
                             ptr(o['dgamma']), ptr(o['dbeta']), ptr(o['dbias']), 0.25, ptr(dy),
                             d['lda'])
                        r = {m: _vres(v, C) for m, v in o.items()}
                        r['dy'] = _res(dy, M, C)
                    tag = f'slots count={count} local={local} bn_slice={on} elu={elu} '
                    ck(tag + 'dy', r['dy'], dyr2, dyb2)
                    l0, l1 = B.slot_sums(ls, C)
                    want = (l1, l0) if local else (0.25 * ref['s1'], 0.25 * ref['s0'])
                    ck(tag + 'dgamma', r['dgamma'], want[0], 2 * U * want[0].abs())
                    ck(tag + 'dbeta', r['dbeta'], want[1], 2 * U * want[1].abs())
                    ck(tag + 'dbias (true value 0)', r['dbias'], torch.zeros(C, dtype=torch.float64),
                       0.25 * 4 * U * ks['k1'].abs() * ref['s0'].abs())
                    res[on] = r
                if len(res) == 2:
                    for m in ('dgamma', 'dbeta', 'dbias'):
                        ck.equal(tag + m + ' bn_slice 1 vs 0', res[1][m], res[0][m])
    ck.done()


# --------------------------------------------------- coefficient kernels ----
@pytest.mark.parametrize('C', B.COEFF_C)
def test_bn_coeffs(C):
    """um_bn_coeffs: null gamma / beta / running pointers, count = -1 (read
    after the sums), count = 1 (unbiased = biased, var clamps to 0)."""
    ck = Checks(f'bn_coeffs C={C}')
    op = B.colred_operands(17, C, 2)
    s, _ = B.colred_ref(op['parts'], C, 2)
    one = op['parts'][0, :C].double()
    variants = [('full', s[:, 0], s[:, 1], op['count'], op['count'], True, True),
                ('null gamma beta', s[:, 0], s[:, 1], op['count'], op['count'], False, True),
                ('null running', s[:, 0], s[:, 1], op['count'], op['count'], True, False),
                ('count=-1', s[:, 0], s[:, 1], -1.0, op['count'] + 19, True, True),
                ('count=1', one, one * one, 1.0, 1.0, True, True)]
    for name, s0, s1, count, n, affine, running in variants:
        st = _d(torch.cat([torch.stack([s0, s1], 1).reshape(-1), torch.tensor([n])]), torch.float64)
        gamma, beta = (op['gamma'], op['beta']) if affine else (None, None)
        rm, rv = _vec(C), _vec(C)
        rm[:C], rv[:C] = _d(op['rm']), _d(op['rv'])
        nbt = torch.tensor([5, 77], dtype=torch.int64, device=DEV)
        o = {k: _vec(C) for k in ('mean', 'invstd', 'scale', 'shift')}
        call('um_bn_coeffs', ptr(st), float(count), C, ptr(_d(gamma)) if affine else None,
             ptr(_d(beta)) if affine else None, B.EPS, B.MOM, ptr(rm) if running else None,
             ptr(rv) if running else None, ptr(nbt), *[ptr(o[k]) for k in o])
        co = B.coeffs_ref(s0, s1, n, gamma, beta, op['rm'] if running else None,
                          op['rv'] if running else None)
        cb = B.coeffs_bounds(co)
        got = {k: _vres(v, C) for k, v in o.items()}
        got.update(rm=_vres(rm, C), rv=_vres(rv, C))
        for k in cb:
            ck(f'{name} {k}', got[k], co[k], cb[k])
        if not running:
            ck.equal(name + ' running_mean untouched', got['rm'], op['rm'].double())
        ck.true(name + ' num_batches_tracked', nbt.cpu().tolist() == [6, 77])
    ck.done()


@pytest.mark.parametrize('C', B.COEFF_C)
def test_bn_bwd_coeffs(C):
    """um_bn_bwd_coeffs: accumulate 0 and 1, stats_local given and null, null
    gamma, count = -1, dbias_scale = 0.25."""
    ck = Checks(f'bn_bwd_coeffs C={C}')
    op = B.colred_operands(17, C, 2)
    lo = B.colred_operands(3, C, 2)
    s, _ = B.colred_ref(op['parts'], C, 2)
    sl, _ = B.colred_ref(lo['parts'], C, 2)
    for acc in (0, 1):
        for local in (False, True):
            for count, affine in ((op['count'], True), (-1.0, False)):
                n = op['count'] if count > 0 else op['count'] + 19
                st = _d(torch.cat([s.reshape(-1), torch.tensor([n])]), torch.float64)
                stl = _d(sl.reshape(-1), torch.float64)
                o = {k: _vec(C) for k in ('dgamma', 'dbeta', 'dbias', 'k1', 'k2', 'k3')}
                o['dgamma'][:C], o['dbeta'][:C] = _d(op['prev']), _d(op['rm'])
                call('um_bn_bwd_coeffs', ptr(st), float(count), C,
                     ptr(_d(op['gamma'])) if affine else None, ptr(_d(op['invstd'])),
                     ptr(stl) if local else None, ptr(o['dgamma']), ptr(o['dbeta']),
                     ptr(o['dbias']), 0.25, acc, ptr(o['k1']), ptr(o['k2']), ptr(o['k3']))
                got = {k: _vres(v, C) for k, v in o.items()}
                k, kb = B.bwd_coeffs_ref(s[:, 0], s[:, 1], n, op['gamma'] if affine else None,
                                         op['invstd'])
                tag = f'accumulate={acc} stats_local={local} count={count} '
                for m in k:
                    ck(tag + m, got[m], k[m], kb[m])
                src = sl if local else s
                for m, v, old in (('dgamma', src[:, 1], op['prev']), ('dbeta', src[:, 0], op['rm'])):
                    old = old.double() if acc else torch.zeros(C, dtype=torch.float64)
                    # one rounding of the sum, one of the addition onto the old value
                    ck(tag + m, got[m], old + v, 2 * U * ((old + v).abs() if not acc else
                                                          old.abs() + v.abs()))
                ck(tag + 'dbias (true value 0)', got['dbias'], torch.zeros(C, dtype=torch.float64),
                   0.25 * 4 * U * k['k1'].abs() * s[:, 0].abs())
    ck.done()


# ------------------------------------------------------ column reductions ----
def _colred_ws(nparts, C, nv):
    n = query('um_colred_ws', nparts, C, nv) // 8
    ws = torch.full((n + 8,), NAN, dtype=torch.float64, device=DEV)
    return ws, n


def _colred_run(entry, op, nparts, C, stride, shift, acc):
    """one launch of a column-reduction entry on fresh outputs -> dict"""
    nv = 1 if entry == 'um_reduce_rows' else 2
    flat = torch.full((nparts * stride + 4,), NAN, dtype=torch.float32, device=DEV)
    parts = flat[shift:shift + nparts * stride]  # shift = 1: the base off by one float
    parts.copy_(_d(op['parts']).reshape(-1))
    ws, n = _colred_ws(nparts, C, nv)
    g, b, ist = _d(op['gamma']), _d(op['beta']), _d(op['invstd'])
    r = {}
    if entry == 'um_bn_stats_reduce':
        out = torch.full((2 * C + 8,), SENT, dtype=torch.float64, device=DEV)
        call(entry, ptr(parts), nparts, C, ptr(out), ptr(ws))
        r['st'] = _vres(out, 2 * C).reshape(C, 2)
    elif entry == 'um_bn_stats_coeffs':
        rm, rv = _vec(C), _vec(C)
        rm[:C], rv[:C] = _d(op['rm']), _d(op['rv'])
        nbt = torch.tensor([5, 77], dtype=torch.int64, device=DEV)
        o = {k: _vec(C) for k in ('mean', 'invstd', 'scale', 'shift')}
        call(entry, ptr(parts), nparts, C, ptr(ws), op['count'], ptr(g), ptr(b), B.EPS, B.MOM,
             ptr(rm), ptr(rv), ptr(nbt), *[ptr(o[k]) for k in o])
        r = {k: _vres(v, C) for k, v in o.items()}
        r.update(rm=_vres(rm, C), rv=_vres(rv, C), nbt=nbt.cpu())
    elif entry == 'um_bn_bwd_stats_coeffs':
        o = {k: _vec(C) for k in ('dgamma', 'dbeta', 'dbias', 'k1', 'k2', 'k3')}
        call(entry, ptr(parts), nparts, C, ptr(ws), op['count'], ptr(g), ptr(ist),
             *[ptr(o[k]) for k in o])
        r = {k: _vres(v, C) for k, v in o.items()}
    else:
        out = _vec(C)
        out[:C] = _d(op['prev'])
        call(entry, ptr(parts), nparts, C, stride, ptr(out), acc, ptr(ws))
        r['out'] = _vres(out, C)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n:]).all()), 'workspace overrun'
    assert bool(torch.isnan(flat[:shift]).all()) and bool(torch.isnan(flat[shift + nparts * stride:]).all())
    return r


def _colred_check(ck, tag, entry, op, r, C, acc):
    nv = 1 if entry == 'um_reduce_rows' else 2
    s, sb = B.colred_ref(op['parts'], C, nv)
    if entry == 'um_bn_stats_reduce':
        ck(tag + 'sums', r['st'], s, sb)
    elif entry == 'um_bn_stats_coeffs':
        co = B.coeffs_ref(s[:, 0], s[:, 1], op['count'], op['gamma'], op['beta'], op['rm'], op['rv'])
        cb = B.coeffs_bounds(co)
        for k in cb:
            ck(tag + k, r[k], co[k], cb[k])
        ck.true(tag + 'num_batches_tracked once', r['nbt'].tolist() == [6, 77])
    elif entry == 'um_bn_bwd_stats_coeffs':
        k, kb = B.bwd_coeffs_ref(s[:, 0], s[:, 1], op['count'], op['gamma'], op['invstd'])
        for m in k:
            ck(tag + m, r[m], k[m], kb[m])
        ck(tag + 'dgamma', r['dgamma'], s[:, 1], 2 * U * s[:, 1].abs() + sb[:, 1])
        ck(tag + 'dbeta', r['dbeta'], s[:, 0], 2 * U * s[:, 0].abs() + sb[:, 0])
        ck(tag + 'dbias (true value 0)', r['dbias'], torch.zeros(C, dtype=torch.float64),
           4 * U * k['k1'].abs() * s[:, 0].abs())
    else:
        prev = op['prev'].double() if acc else None
        ref = s[:, 0] + (prev if acc else 0)
        ck(tag + 'out', r['out'], ref, B.f32_out_bound(ref, sb[:, 0], prev))


COLRED_ENTRIES = ['um_bn_stats_reduce', 'um_bn_stats_coeffs', 'um_bn_bwd_stats_coeffs',
                  'um_reduce_rows']
COLRED = ([(n, c, c) for n in B.COLRED_NPARTS for c in B.COLRED_C] +
          [(n,) + B.COLRED_ROWS_EXTRA for n in B.COLRED_NPARTS])


@pytest.mark.parametrize('ticket', [0, 1], ids=['one-workgroup', 'ticket'])
@pytest.mark.parametrize('nparts,C,stride', COLRED,
                         ids=lambda v: str(v))
def test_column_reductions(nparts, C, stride, ticket):
    """um_bn_stats_reduce, um_bn_stats_coeffs, um_bn_bwd_stats_coeffs and
    um_reduce_rows: the vector form, the scalar form (base pointer off by one
    float, rowstride % 4 != 0, NV = 1 with accumulate), one workgroup and the
    multi-workgroup last-arriver finish (ticket and reset of publish_finish:
    three launches back to back on fresh outputs, bit-equal and within the
    bar -- the counter reset and the fixed summation order)."""
    ck = Checks(f'colred nparts={nparts} C={C} stride={stride} ticket={ticket}')
    rows_only = stride != C
    with tuning(**(B.COLRED_TICKET if ticket else {})):
        blocks = query('um_colred_ws', nparts, C, 2) // (C * 2 * 8)
        if ticket:  # min(128, nparts, values / 64) workgroups
            ck.true('ticket form', blocks == B.colred_blocks(nparts, C, 2, 1, 64) and
                    (blocks > 1 or nparts * C * 2 <= 64 or nparts == 1))
        for entry in COLRED_ENTRIES[3:] if rows_only else COLRED_ENTRIES:
            nv = 1 if entry == 'um_reduce_rows' else 2
            op = B.colred_operands(nparts, C, nv, stride if rows_only else None)
            st = stride if rows_only else C * nv
            for shift, acc in ((0, 0), (1, 0), (0, 1)):
                if acc and nv == 2:
                    continue
                tag = f'{entry} shift={shift} accumulate={acc} '
                runs = [_colred_run(entry, op, nparts, C, st, shift, acc) for _ in range(3)]
                _colred_check(ck, tag, entry, op, runs[0], C, acc)
                for other in runs[1:]:
                    for k in runs[0]:
                        ck.equal(tag + k + ' repeat launch', other[k], runs[0][k])
    ck.done()


# -------------------------------------------------------------------- SE ----
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('C', B.MEAN_C)
@pytest.mark.parametrize('S', B.MEAN_S)
def test_channel_mean(S, C, mode):
    """um_channel_mean: one pixel, the pixel-chunk tail (2049, 4100), the
    two-rows-in-flight loop and its odd tail, ld = C and C + 8."""
    x = B.mean_operands(S, C, mode != 'f32')
    ref, bound = B.mean_ref(x)
    ck = Checks(f'channel_mean S={S} C={C} {mode}')
    dt = torch.float32 if mode == 'f32' else torch.bfloat16
    for ld in (C, C + 8):
        xb = _in(x.reshape(2 * S, C), dt, ld)
        out = torch.zeros(2 * C + 8, dtype=torch.float32, device=DEV)
        out[2 * C:] = SENT
        call('um_channel_mean', UM_F32 if mode == 'f32' else UM_BF16, 2, S, C, ptr(xb), ld, ptr(out))
        ck(f'ld={ld}', _vres(out, 2 * C).reshape(2, C), ref, bound)
    ck.done()


@pytest.mark.parametrize('N', B.SE_N)
@pytest.mark.parametrize('ppi', B.SE_PARTS)
@pytest.mark.parametrize('C,R', B.SE_CR)
def test_se_mlp_fwd(C, R, ppi, N):
    """um_se_mlp_fwd: the 8-way unrolled pool loop and its tail, R not a
    multiple of 4, R > 256, C not a multiple of 4 lanes x 4; dead ReLU rows
    are exactly 0."""
    op = B.se_operands(C, R, N, ppi)
    ck = Checks(f'se_mlp_fwd C={C} R={R} parts={ppi} N={N}')
    o = dict(pooled=_vec(N * C), z1=_vec(N * R), s=_vec(N * C))
    call('um_se_mlp_fwd', N, C, R, ptr(_d(op['parts'])), ppi, op['inv_hw'], ptr(o['pooled']),
         ptr(_d(op['w1'])), ptr(_d(op['w2'])), ptr(o['z1']), ptr(o['s']))
    for k, n in (('pooled', C), ('z1', R), ('s', C)):
        got = _vres(o[k], N * n).reshape(N, n)
        ck(k, got, op[k], op[k + '_b'])
        if k == 'z1':
            ck.true('dead rows exactly 0', bool((got[op['pre'] < 0] == 0).all()))
    ck.done()


@pytest.mark.parametrize('N', B.SE_N)
@pytest.mark.parametrize('C,R', B.SE_CR)
def test_se_mlp_bwd(C, R, N):
    """um_se_mlp_bwd against the f64 backward of sigmoid(W2 relu(W1 p)) (equal
    to f64 autograd, tests/test_bn_cases_cpu.py) on the f32 s / z1 / pooled it
    is given; some z1 are exactly 0 (the gate)."""
    op = B.se_operands(C, R, N)
    i, ref = B.se_bwd_inputs(op), B.se_bwd_ref(op)
    ck = Checks(f'se_mlp_bwd C={C} R={R} N={N}')
    o = dict(dw1=_vec(R * C), dw2=_vec(C * R), dpool=_vec(N * C), dz=_vec(N * R))
    call('um_se_mlp_bwd', N, C, R, ptr(_d(op['ds'])), ptr(_d(i['s'])), ptr(_d(i['z1'])),
         ptr(_d(i['pooled'])), ptr(_d(op['w1'])), ptr(_d(op['w2'])), ptr(o['dw1']), ptr(o['dw2']),
         ptr(o['dpool']), ptr(o['dz']), op['inv_hw'])
    for k, shape in (('dz', (N, R)), ('dw2', (C, R)), ('dw1', (R, C)), ('dpool', (N, C))):
        ck(k, _vres(o[k], shape[0] * shape[1]).reshape(shape), ref[k], ref[k + '_b'])
    ck.done()
