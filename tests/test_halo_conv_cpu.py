"""The acceptance criteria of tests/test_gpu_halo_conv.py have teeth: for every
case of its tables, each criterion is evaluated here, without a GPU, with the
f64 reference in the kernel's place against a deliberately wrong reference --
the same convolution with tap (0, R-1) of the last real input channel zeroed
-- and must reject it (and must accept the reference itself, rounded the way
the kernel stores it).  A case whose bar a one-tap error slips under would be
mis-specified."""
import pytest
import torch

import _halo_cases as HC

FWD_CASES = sorted(set(HC.EXACT_CASES + HC.PERSIST_CASES + HC.RAGGED_CASES + HC.REFUSED_CASES +
                       HC.EPILOGUE_CASES))


def _bf16(t):
    return t.to(torch.bfloat16).double()


def _sums(y):
    return y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))


@pytest.mark.parametrize('case', FWD_CASES)
def test_forward_criteria_reject_one_tap(case):
    op = HC.fwd_operands(case)
    epis = HC.EPILOGUES if case in HC.EPILOGUE_CASES else ['bias']
    for epi in epis:
        ref, mut = HC.epilogue_ref(op['ref'], op, epi), HC.epilogue_ref(op['mut'], op, epi)
        # the right answer as the kernel stores it passes ...
        assert HC.f32_ok(ref.float(), ref), (case, epi)
        assert HC.bf16_ok(_bf16(ref), ref), (case, epi)
        # ... and is rejected against the mutant, in both output types
        assert not HC.f32_ok(ref.float(), mut), (case, epi)
        assert not HC.bf16_ok(_bf16(ref), mut), (case, epi)
    # the statistics bar alone, sum and sum of squares each on its own
    ref, mut = op['ref'], op['mut']
    s1, s2 = _sums(ref)
    assert HC.stats_ok(s1, s2, ref), case
    e1, e2 = HC.stats_err(s1, s2, mut)
    assert e1 > HC.STAT_TOL and e2 > HC.STAT_TOL, (case, e1, e2)


@pytest.mark.parametrize('case', HC.DGRAD_CASES)
def test_dgrad_criteria_reject_one_tap(case):
    op = HC.dgrad_operands(case)
    for prev in (0, op['prev'].double()):
        ref, mut = op['ref'] + prev, op['mut'] + prev
        assert HC.bf16_ok(_bf16(ref), ref), case
        assert not HC.bf16_ok(_bf16(ref), mut), case


def test_tables_are_the_smallest_shapes_of_each_arm():
    """every arm named in the tables exists in them: exact and ragged tiles in
    both directions, all three filter sizes, both pad modes, one- and
    multi-chunk inputs with a partial chunk, every column-block width"""
    cases = HC.EXACT_CASES + HC.RAGGED_CASES
    assert {c[2] for c in cases} == {3, 5, 7}
    assert {c[3] for c in cases} == {'zero', 'reflect'}
    assert any(c[0] % 32 for c in cases) and any(c[0] > 32 for c in cases)
    # one column block of 16 / 32 / 64, one of 96 and of 128, column grids
    assert {8, 32, 64, 96, 128, 160} <= {c[1] for c in HC.EXACT_CASES}
    assert any(c[4] % HC.TH for c in HC.RAGGED_CASES) and any(c[5] % HC.TW for c in HC.RAGGED_CASES)
    assert all(c[4] % HC.TH == 0 and c[5] % HC.TW == 0 for c in HC.EXACT_CASES)
    assert all(c[4] % HC.TH or c[5] % HC.TW for c in HC.RAGGED_CASES)
