"""The attention core (csrc/attention.hip) against an f64 reference on exact
operands, on every dispatch path: um_attn_fwd and um_attn_bwd are called
through the C ABI (no convs in the error), the backward on the kmax / ksum /
ctx its own forward saved, as AttentionFn does.  Table, reference and
per-element bars are in tests/_attn_cases.py (tests/test_attn_cases_cpu.py
shows that the bars reject nine subtly wrong references); each case prints its
path and its worst ratio max(|got - ref| / bound) per output before it
asserts them <= 1.

Every output and workspace is a view into a larger buffer: stride-padding
columns, one row after the last pixel and 64 floats after every vector and
workspace hold a sentinel that must survive; att, the 3C columns of dqkv and
the saved state start as NaN and must end finite; the inputs' padding columns
are NaN.  Workspaces have exactly the size um_attn_ws_* report, combined as
AttentionFn combines them.  A second call must give the same bytes."""
import pytest
import torch

import _attn_cases as A
from umamd._lib import UM_BF16, UM_F32, call, ptr, query

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = 7.0   # exact in bf16
TAIL = 64    # sentinel floats after a vector / workspace
NAN = float('nan')


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    """a device error ends the session: nothing more is launched after it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


def _in(t, dt, ld):
    """[M][C] -> device [M][ld], NaN in the columns past C"""
    buf = torch.full((t.shape[0], ld), NAN, dtype=dt, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV).to(dt)
    return buf


def _rows(M, C, ld, dt):
    """[M + 1][ld]: NaN where the kernel must write, sentinel around it"""
    buf = torch.full((M + 1, ld), SENT, dtype=dt, device=DEV)
    buf[:M, :C] = NAN
    return buf


def _vec(n, fill=NAN):
    buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device=DEV)
    buf[:n] = fill
    return buf


def _rows_ok(buf, M, C):
    return bool((buf[:M, C:] == SENT).all()) and bool((buf[M:] == SENT).all())


def _run(case):
    """one forward and one backward of a case -> dict of device buffers"""
    N, S, C, heads, dtype = case[:5]
    M, d = N * S, C // heads
    ld, ldo, ldd, ldq = A.strides(case)
    dt, code = (torch.bfloat16, UM_BF16) if dtype == 'bf16' else (torch.float32, UM_F32)
    op = A.operands(case)
    o = dict(qkv=_in(op['qkv'], dt, ld), datt=_in(op['datt'], dt, ldd))
    n_ks, n_ctx = query('um_attn_ws_kstats', N, S, C), query('um_attn_ws_ctx', N, S, C, heads)
    n_tiles = query('um_attn_ws_tiles', N, S, C, heads)
    o.update(kmax=_vec(N * C), ksum=_vec(N * C), ctx=_vec(N * C * d), att=_rows(M, C, ldo, dt),
             ws_f=_vec(max(n_ks, n_ctx)), ws_b=_vec(n_tiles), dqkv=_rows(M, 3 * C, ldq, dt),
             dks=_vec(M * C), dctx=_vec(N * C * d), r=_vec(N * C))
    call('um_attn_fwd', code, N, S, C, heads, ptr(o['qkv']), ld, ptr(o['kmax']), ptr(o['ksum']),
         ptr(o['ctx']), ptr(o['ws_f']), ptr(o['att']), ldo)
    call('um_attn_bwd', code, N, S, C, heads, ptr(o['qkv']), ld, ptr(o['kmax']), ptr(o['ksum']),
         ptr(o['ctx']), ptr(o['datt']), ldd, ptr(o['dqkv']), ldq, ptr(o['dks']), ptr(o['ws_b']),
         ptr(o['dctx']), ptr(o['r']))
    torch.cuda.synchronize()
    o['sizes'] = dict(kmax=N * C, ksum=N * C, ctx=N * C * d, ws_f=max(n_ks, n_ctx),
                      ws_b=n_tiles, dks=M * C, dctx=N * C * d, r=N * C)
    return o


@pytest.mark.parametrize('case', A.CASES, ids=[A.case_id(c) for c in A.CASES])
def test_attention_core(case):
    N, S, C, heads = case[:4]
    M, p = N * S, A.case_path(case)
    ref, b = A.reference(case), A.bounds(case)
    o = _run(case)
    bad = []
    # guards: nothing written outside the announced sizes and strides
    for n, size in o['sizes'].items():
        if not bool((o[n][size:] == SENT).all()):
            bad.append(f'sentinel after {n} overwritten')
    if not _rows_ok(o['att'], M, C):
        bad.append('att guard overwritten')
    if not _rows_ok(o['dqkv'], M, 3 * C):
        bad.append('dqkv guard overwritten')
    # which path ran is observed, not assumed.  These two marks are facts of
    # today's kernels, not of the ABI: the MFMA backward ignores dctx and r,
    # the others write them; the tile workspace holds nt tiles of the path's
    # own tile size.  A kernel change that writes dctx / r on the MFMA path
    # or retiles the backward updates _attn_cases.bwd_ws_written and this
    # block with it -- the values are not at stake here.
    untouched = bool(torch.isnan(o['dctx'][:N * C * (C // heads)]).all()) and \
        bool(torch.isnan(o['r'][:N * C]).all())
    if untouched != (p == 'mfma'):
        bad.append(f'dctx / r untouched: {untouched} on path {p}')
    written = int(torch.isfinite(o['ws_b'][:o['sizes']['ws_b']]).sum())
    if written != A.bwd_ws_written(case):
        bad.append(f'tile workspace: {written} floats written, {A.bwd_ws_written(case)} expected')
    got = dict(kmax=o['kmax'][:N * C], ksum=o['ksum'][:N * C], ctx=o['ctx'][:o['sizes']['ctx']],
               att=o['att'][:M, :C], dk=o['dqkv'][:M, :C], dq=o['dqkv'][:M, C:2 * C],
               dv=o['dqkv'][:M, 2 * C:3 * C])
    if p != 'mfma':
        got.update(dctx=o['dctx'][:o['sizes']['dctx']], r=o['r'][:N * C])
    got = {n: v.double().cpu() for n, v in got.items()}
    rs = {n: A.ratio(v, ref[n], b[n]) for n, v in got.items()}  # inf: a NaN left or produced
    print(f'attn {p} {A.case_id(case)}: ' + ' '.join(f'{n} {v:.3f}' for n, v in rs.items()))
    bad += [f'{n}: ratio {v:.3f}' for n, v in rs.items() if not v <= 1.0]
    if not torch.equal(got['kmax'], ref['kmax'].reshape(-1)):
        bad.append('kmax is not the exact maximum')
    # no atomics anywhere: a second call gives the same bytes
    o2 = _run(case)
    for n in ('kmax', 'ksum', 'ctx', 'att', 'dqkv') + (('dctx', 'r') if p != 'mfma' else ()):
        if not torch.equal(o[n].view(torch.uint8), o2[n].view(torch.uint8)):
            bad.append(f'{n} differs between two calls')
    assert not bad, (p, case, bad)
