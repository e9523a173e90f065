"""The acceptance criteria of tests/test_gpu_attn.py have teeth, and its table
reaches every arm of csrc/attention.hip it names.  No GPU:
  - the table reaches the three dispatch paths with both dtypes, N = 3, every
    head width, the tile-edge pixel counts, 'wide' and 'cliff' logits at a
    ragged S, padded strides, and the arms listed in the issue (several chunks,
    tiles_per_wg = 2, more than 64 k-stat chunks, a k-stat chunk of fewer than
    4 pixels, the unrolled part-sum loop, the enlarged dynamic LDS);
  - ``path()`` agrees with the dispatch: with the path each table row was
    written for, and with the library's workspace queries (which switch on the
    same head-shape predicate);
  - the written-out f64 backward equals f64 autograd;
  - an f32 restatement of the same math (torch.exp, unchunked) passes every
    bar, and its worst ratio per output over the f32 cases is at least about
    1/8 (1/16 for dK and r): the bars leave room for another summation order
    and __expf, no more.  The ratios are printed (run with -s) and recorded
    in DESIGN.md section 5;
  - nine mutants of the reference fail the bar of the output they corrupt on
    every case where they apply.
"""
import functools

import pytest
import torch

import _attn_cases as A
from umamd._lib import query

IDS = [A.case_id(c) for c in A.CASES]
ARMS = [A.arms(c) for c in A.CASES]


def _some(**want):
    return any(all(a.get(k) == v for k, v in want.items()) for a in ARMS)


def test_table_reaches_every_arm():
    assert len(set(A.CASES)) == len(A.CASES)
    for p in ('mfma', 'small', 'generic'):
        assert _some(path=p, dtype='f32') and _some(path=p, dtype='bf16'), p
        assert _some(path=p, N=3) and _some(path=p, N=1) and _some(path=p, N=2), p
        assert _some(path=p, logits='wide', ragged=True), p
        assert _some(path=p, logits='cliff', ragged=True), p
        assert _some(path=p, odd_stride=True, off_fast_path=False), p
        assert _some(path=p, multi_chunk=True), p
        S_seen = {c[1] for c, a in zip(A.CASES, ARMS) if a['path'] == p}
        assert {1, 17, 63, 64, 65, 130} <= S_seen, (p, S_seen)
    heads_of = lambda p: {(c[2], c[3]) for c, a in zip(A.CASES, ARMS) if a['path'] == p}
    assert {(32, 2), (64, 2), (64, 1), (128, 8), (512, 8)} <= heads_of('mfma')
    assert {(32, 8), (64, 8), (64, 16), (16, 4), (8, 1)} <= heads_of('small')
    assert {(16, 8), (24, 2), (128, 16), (96, 2), (24, 3), (64, 1)} <= heads_of('generic')
    assert {a['d'] for a in ARMS if a['path'] == 'mfma'} == {16, 32, 64}
    assert {a['d'] for a in ARMS if a['path'] == 'small'} == {4, 8}
    assert _some(path='mfma', tpw2=True, N=2)
    assert _some(path='generic', ks64=True, sum_unrolled=True)
    assert _some(path='generic', short_chunk=True) and _some(path='small', short_chunk=True)
    assert _some(path='generic', big_lds=True, dtype='f32', off_fast_path=True)
    assert _some(path='generic', wide_dd=True)
    # ld = 3C + 4 takes an MFMA-shaped and a small-shaped case to the generic kernels
    off = [c for c, a in zip(A.CASES, ARMS) if a['off_fast_path']]
    assert all(A.case_path(c) == 'generic' and c[4] == 'f32' for c in off)
    assert any(A.mfma_shaped(c[2], c[3]) for c in off)
    assert any(c[2] // c[3] in (4, 8) for c in off)
    for c in A.CASES:  # the larger pixel counts keep N <= 2; operands stay small
        assert c[1] <= 130 or c[0] <= 2
        assert c[0] * c[1] * 4 * c[2] * (2 if c[4] == 'bf16' else 4) <= 12 << 20


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_path_agrees_with_dispatch(case):
    N, S, C, heads = case[:4]
    want = A.WRITTEN_FOR[case]
    assert A.case_path(case) == want
    ld, ldo, ldd, ldq = A.strides(case)
    # forward and backward take the same path for every stride set of the table
    assert A.path(C, heads, ld, ldo) == A.path(C, heads, ld, 0, ldd, ldq) == want
    # the library sizes its workspaces by the same head-shape predicate
    got = (query('um_attn_ws_kstats', N, S, C), query('um_attn_ws_ctx', N, S, C, heads),
           query('um_attn_ws_tiles', N, S, C, heads))
    assert got == A.ws_sizes(case)
    assert A.bwd_ws_written(case) <= got[2]


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_written_out_backward_is_autograd(case):
    ref, C = A.reference(case), case[2]
    ag = A.autograd_dqkv(case)
    for i, n in enumerate(('dk', 'dq', 'dv')):
        a = ag[:, i * C:(i + 1) * C]
        # two f64 evaluations: sums of S terms in different orders
        tol = max(1e-12, 16 * case[1] * 2.0 ** -52) * max(1.0, float(a.abs().max()))
        assert float((ref[n] - a).abs().max()) <= tol, n
    assert torch.equal(ref['kmax'], A.operands(case)['qkv'][:, :C].double()
                       .reshape(case[0], case[1], C).max(dim=1).values)


@functools.lru_cache(maxsize=None)
def _restatement_ratios(case):
    ref, b, got = A.reference(case), A.bounds(case), A.restatement(case)
    return {n: A.ratio(got[n], ref[n], b[n]) for n in ('kmax',) + A.OUTPUTS}


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_f32_restatement_passes(case):
    rs = _restatement_ratios(case)
    print(A.case_path(case), A.case_id(case), ' '.join(f'{n} {v:.3f}' for n, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs


def test_bars_sit_close_to_the_restatement():
    """the lower pin: over the table, the restatement's worst ratio per output
    is at least about 1/8 (f32 cases: a bf16 store alone reaches 0.99).  dK
    and r are held to 1/16: their A nests three absolute-value sums
    """
    f32 = [_restatement_ratios(c) for c in A.CASES if c[4] == 'f32']
    worst = {n: max(rs[n] for rs in f32) for n in A.OUTPUTS}
    print('restatement worst (f32 cases):', ' '.join(f'{n} {v:.3f}' for n, v in worst.items()))
    for n, v in worst.items():
        assert v >= (1 / 16 if n in ('dk', 'r') else 1 / 8), (n, v)


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_mutants_fail(case):
    op, ref, b = A.operands(case), A.reference(case), A.bounds(case)
    for m in A.MUTANTS:
        if not A.mutant_applies(m, case):
            continue
        bad = A.attn_math(case, op['qkv'], op['datt'], mut=m)
        n = A.MUTANT_SEEN_IN[m]
        got = bad[n].to(torch.bfloat16) if case[4] == 'bf16' and n in A.STORED else bad[n]
        assert A.ratio(got, ref[n], b[n]) > 1.0, (m, n)
    # one element moved by four bounds
    for n in A.OUTPUTS:
        got = ref[n].clone()
        i = got.numel() // 2
        got.view(-1)[i] += 4 * b[n].reshape(-1)[i]
        assert not A.ok(got, ref[n], b[n]), n
    nan = ref['att'].clone()
    nan.view(-1)[0] = float('nan')
    assert not A.ok(nan, ref['att'], b['att'])
    assert not A.ok(ref['kmax'] + 2.0 ** -20, ref['kmax'], b['kmax'])


def test_every_mutant_applies_somewhere_on_every_path():
    for p in ('mfma', 'small', 'generic'):
        for m in A.MUTANTS:
            assert any(A.mutant_applies(m, c) for c in A.CASES if A.case_path(c) == p), (p, m)
