"""The cases of tests/test_gpu_conv_exact.py are honest: without a device, in float64.

For every case and grid family the operands are rebuilt from their seed (the CU-sized batches at helpers.EXACT_NCU) and
1. meet the conditions under which bit equality with the float64 result IS the specification (helpers.exact_conditions): hi + lo
   carries each operand, exactly one operand has a lo term, the sum of |products| of every output stays below 2^24 quanta of
   2^-12, the reference is its own fp32 rounding.  They hold analytically: |product| <= 511 * 8 quanta, and a case has at most
   4096 products per output (asserted: K of the forward pass and the data gradient, pixels of the weight gradient):
   4096 * 4088 = 16 744 448 < 2^24 = 16 777 216;
2. give the reference exactly when restated as hi*hi + lo*hi + hi*lo (helpers.conv_bf16x3);
3. give something else under every mutant of that restatement, each a wrong hi/lo pairing or tile placement: the live cross
   product dropped, lo dropped on every 32nd channel, lo paired with the neighbouring pixel's hi on every 32nd channel and, for
   the shapes whose tiles start inside a row of a padded conv, the left padding tap reading the previous row's last pixel.
   So a kernel with such a bug cannot pass the bit equality.  (Images of a batch are independent: the mutants of the forward
   pass and the data gradient are evaluated on the first two images.)"""
import functools

import pytest
import torch

from tests import helpers

CASES = [(kind, name) for kind in sorted(helpers.EXACT_KINDS) for name in sorted(helpers.EXACT_KINDS[kind]())]


@functools.lru_cache(maxsize=None)
def _checked(kind, name, family):
    case = helpers.EXACT_KINDS[kind]()[name]
    a, b = helpers.exact_case_operands(kind, name, family)
    conditions, ref = helpers.exact_conditions(a, b, case.op, family)
    return case, a, b, conditions, ref


@pytest.mark.parametrize("family", helpers.EXACT_FAMILIES)
@pytest.mark.parametrize("kind,name", CASES)
def test_the_operands_make_bit_equality_the_specification(kind, name, family):
    case, a, b, conditions, ref = _checked(kind, name, family)
    assert case.reduction(helpers.EXACT_NCU) <= 4096
    assert conditions == dict(carried=True, one_lo=True, quanta=True, ref_is_fp32=True)
    assert float(ref.abs().max()) > 0
    if kind == "wgrad" and case.cin == 8:
        assert float(a[:, 6:].abs().max()) == 0
    if name == "bias fp32":
        dbias = b.double().sum((0, 2, 3))
        assert torch.equal(dbias.float().double(), dbias)


@pytest.mark.parametrize("family", helpers.EXACT_FAMILIES)
@pytest.mark.parametrize("kind,name", CASES)
def test_the_bit_equality_has_teeth(kind, name, family):
    case, a, b, _, ref = _checked(kind, name, family)
    if kind != "wgrad":   # two images of the batch
        a, ref = a[:2], ref[:2]
    restate = lambda mutant: helpers.conv_bf16x3(case.op, a, b, case.axes, case.pixels, mutant)
    assert torch.equal(restate(None), ref)
    mutants = ["drop_a_lo" if family == "a_lo" else "drop_b_lo", "lo32", "pair32"] + (["wrap_left"] if case.midrow else [])
    for mutant in mutants:
        changed = float((restate(mutant) != ref).double().mean())
        print("OBSERVED %s %s %s %s: %.1f %% of the outputs change" % (kind, name, family, mutant, 100 * changed))
        assert changed > 0, mutant
    # the cross product that is not live is zero: dropping it changes nothing (the family has no lo * lo product to miss)
    assert torch.equal(restate("drop_b_lo" if family == "a_lo" else "drop_a_lo"), ref)


def test_the_midrow_cases_start_tiles_inside_a_row():
    """what makes a case 'midrow': the 128-pixel tiles of the conv the kernel runs are flat runs of its output pixels, and
    some start at a column other than 0"""
    for kind, name in CASES:
        case = helpers.EXACT_KINDS[kind]()[name]
        if case.midrow:
            ho, wo = (case.H, case.W) if kind == "dgrad" else case.out_hw()
            starts = {(t * 128) % (ho * wo) % wo for t in range(case.batch(helpers.EXACT_NCU) * ho * wo // 128)}
            assert case.pad >= 1 and (ho * wo) % 128 == 0 and starts != {0}, (name, starts)
