"""conv3x3_halo_bf16x3 (csrc/conv.hip) on the 16x16x32 bf16 MFMA: fragment layout, tile placement, hi/lo pairing and the batch
invariance of its instantiations, through ops.conv2d_forward at the smallest shapes that reach each route.

1. Order-independent exactness.  Inputs on a coarse binary grid: every product and every partial sum of a convolution output is
   a multiple of 2^-12 below 2^24 * 2^-12, so fp32 accumulation is exact in ANY order and the float64 reference rounded to fp32
   is the specification, bit for bit.  One operand needs its lo term (nine significant bits), the other has none, so no
   lo * lo product is missing from hi*hi + hi*lo + lo*hi.  A wrong lane <-> k, tile <-> row or hi/lo pairing cannot pass; an
   accumulation order can not matter, so the test holds for any MFMA shape.
2. Random inputs against float64, the bound of tests/test_gpu_ops.py.
3. Image k of a batch that runs the 8 x 32-pixel tile / the 128-channel tile equals, bit for bit, the same image run alone (on
   the 64-channel tile): the instantiations add the products of an output in the same order.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import helpers
from tests.test_gpu_conv_dispatch import _profiled

pytestmark = pytest.mark.gpu


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# case -> (Cin, Cout, transposed, H, W, N(ncu)): H x W is the input map.  The first five are the halo cases of
# tests/test_gpu_conv_dispatch.py (one per instantiation without a raw input).
CASES = {
    "halo64": (32, 64, False, 4, 32, lambda ncu: 1),
    "halo128": (32, 128, False, 12, 32, lambda ncu: -(-ncu // 3)),
    "halo_tall": (32, 128, False, 8, 32, lambda ncu: ncu),
    "ct_narrow": (32, 64, True, 4, 32, lambda ncu: 1),
    "ct_wide": (32, 128, True, 16, 32, lambda ncu: -(-ncu // 4)),
    "two_slices": (64, 64, False, 8, 64, lambda ncu: 1),      # halo slot flip, ring wrap, two column tiles
    "four_slices": (128, 64, False, 4, 32, lambda ncu: 1),
    "three_columns": (32, 64, False, 12, 96, lambda ncu: 1),  # three column tiles, image borders on all four sides
}
# the batched launches whose image k is compared with the image run alone
BATCHED = ["halo128", "halo_tall", "ct_wide"]


def _conv64(x, w, transposed):
    if transposed:
        return F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1, output_padding=1)
    return F.conv2d(x.double(), w.double(), None, stride=1, padding=1)


# the grid families of tests/helpers.py under this file's names: the operands are (x, w)
_FAMILY = {"x_lo": "a_lo", "w_lo": "b_lo"}


@functools.lru_cache(maxsize=None)
def _operands(case, family):
    """(x NCHW, w, float64 reference) on the CPU.  family 'x_lo' / 'w_lo': helpers.exact_operands' 'a_lo' / 'b_lo' (x = n / 256,
    |n| <= 511, w = m / 16, |m| <= 8, and the converse); 'random': the operands of tests/test_gpu_ops.py's halo test."""
    cin, cout, transposed, H, W, n_of = CASES[case]
    N = n_of(_ncu())
    g = torch.Generator().manual_seed(sorted(CASES).index(case) * 10 + ["x_lo", "w_lo", "random"].index(family))
    wshape = (cin, cout, 3, 3) if transposed else (cout, cin, 3, 3)
    if family == "random":
        x, w = torch.randn(N, cin, H, W, generator=g), torch.randn(wshape, generator=g) * 0.05
    else:
        x, w = helpers.exact_operands(_FAMILY[family], (N, cin, H, W), wshape, g)
    return x, w, _conv64(x, w, transposed)


_RUNS = {}


def _run(case, family):
    """the kernel's output (NCHW, on the CPU) and the names of the conv kernels that ran; one launch per (case, family)"""
    if (case, family) not in _RUNS:
        from impersonator_amd import ops
        transposed = CASES[case][2]
        x, w, _ = _operands(case, family)
        xg, wg = x.permute(0, 2, 3, 1).contiguous().cuda(), w.cuda().contiguous()
        y, names = _profiled(lambda: ops.conv2d_forward(xg, wg, None, 2 if transposed else 1, 1, transposed, precision="bf16x3"))
        _RUNS[(case, family)] = (y.cpu().permute(0, 3, 1, 2), names, xg, wg)
    return _RUNS[(case, family)][:2]


_split = helpers.bf16_split_f32


@pytest.mark.parametrize("family", ["x_lo", "w_lo"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_inputs_give_the_float64_result_bit_for_bit(case, family):
    x, w, ref = _operands(case, family)
    transposed = CASES[case][2]
    # conditions on the inputs, checked in float64 on the CPU: hi + lo carries each operand exactly, one operand has no lo term
    # (no lo * lo product exists), and the sum of |products| of every output stays below 2^24 units of the products' common
    # quantum 2^-12 -- so every partial sum, in any order, is an fp32 number and the reference is its own fp32 rounding
    (xh, xl), (wh, wl) = _split(x), _split(w)
    assert torch.equal(xh + xl, x) and torch.equal(wh + wl, w)
    assert (xl if family == "w_lo" else wl).abs().max() == 0 and (wl if family == "w_lo" else xl).abs().max() > 0
    assert float(_conv64(x.abs(), w.abs(), transposed).max()) * 4096 < 2 ** 24
    assert torch.equal(ref.float().double(), ref)
    y, names = _run(case, family)
    print("OBSERVED %s %s: %s" % (case, family, names))
    assert len(names) == 1 and names[0].startswith("conv3x3_halo_bf16x3<")
    assert torch.equal(y, ref.float())


@pytest.mark.parametrize("case", sorted(CASES))
def test_random_inputs_against_float64(case):
    _, _, ref = _operands(case, "random")
    y, names = _run(case, "random")
    rel = float((y.double() - ref).abs().max()) / float(ref.abs().max())
    print("OBSERVED %s: %s rel %.3g" % (case, names, rel))
    assert len(names) == 1 and names[0].startswith("conv3x3_halo_bf16x3<")
    assert rel < helpers.BF16X3_REL


@pytest.mark.parametrize("case", BATCHED)
def test_an_image_of_a_batch_equals_the_image_run_alone(case):
    from impersonator_amd import ops
    transposed = CASES[case][2]
    y, names = _run(case, "random")
    _, _, xg, wg = _RUNS[(case, "random")]
    N = xg.shape[0]
    alone = set()
    for k in sorted({0, N // 2, N - 1}):
        yk, nk = _profiled(lambda: ops.conv2d_forward(xg[k:k + 1].contiguous(), wg, None, 2 if transposed else 1, 1, transposed,
                                                      precision="bf16x3"))
        alone.update(nk)
        assert torch.equal(yk.cpu().permute(0, 3, 1, 2)[0], y[k]), "image %d" % k
    print("OBSERVED %s: batch of %d on %s, one image on %s" % (case, N, names, sorted(alone)))
    # the comparison crossed instantiations: a Cout = 128 layer runs one image on the 64-channel tile, the batch on the 128-channel one
    assert len(alone) == 1 and alone != set(names)
