"""Order-independent exactness of the op-level convolutions and both gradients (csrc/conv.hip, csrc/train.hip): the ring kernel
conv_igemm_bf16x3, the in-kernel split conv_igemm_f32<..., X3 = true>, the data-gradient routes behind relayout modes 0, 1, 2,
every row of kWgradKernelTable with its reduce_* kernels, and the fp32 routes of the same shapes.

Operands on the coarse binary grid of tests/helpers.py (families 'a_lo' / 'b_lo': one operand n / 256, |n| <= 511, the other
m / 16, |m| <= 8).  Every product is a multiple of 2^-12 and the sum of |products| of an output stays below 2^24 of them, so
fp32 accumulation is exact in ANY order and the float64 result rounded to fp32 is the specification, bit for bit: a wrong
lane <-> k, tile <-> row or hi/lo pairing cannot pass, and the test survives a change of MFMA shape, of the K order or of the
split-K slicing.  tests/test_conv_exact_cases.py proves, without a device, that every case meets these conditions and that
the mutants of the float64 restatement (a dropped cross product, a lo dropped or mis-paired on one channel in 32, a padding tap
that misses the row wrap) do not give the reference.  The operands have at most ten and five significant bits, so fp32
products are exact too: every forward case runs a second time with precision 'fp32' and is held to the same equality.

1. Forward: the ring on every instantiation, on maps whose 128-pixel tiles start inside a row (16 x 24: tiles at row 5 column 8
   and row 10 column 16; with 3x3 / stride 2 both horizontal padding taps fall inside tiles and tiles 3 to 5 belong to image
   1), on K = 2304 (72 stages), and the in-kernel split on 100-pixel maps and the 7x7 8-channel stem.
2. Data gradient, families on (dy, w), against float64 autograd, on rectangular maps.
3. Weight gradient, families on (x, dy): every row of tests/test_gpu_wgrad_dispatch.CASES with the plan and name assertions of
   that file, a transposed layer, a batch of three, and the bias gradient.
4. Batch invariance of the ring on random operands: images 0, N/2 and N-1 of the ring128 / ring_tall batches equal, bit for
   bit, the image run alone on the 64-channel 128-row instantiation.

Kernels observed per case on a 256-CU MI355X (the OBSERVED lines of a run with -s):
  forward           bf16x3                                      fp32 (the op-level fp32 route is the general-mode kernel)
    ring64            conv_igemm_bf16x3<64,1,2,3,0,128>           conv_igemm_f32<64,1,2,false,0,true,false>
    ring128           conv_igemm_bf16x3<128,2,2,4,0,128>          conv_igemm_f32<128,2,2,false,0,true,false>
    ring_tall         conv_igemm_bf16x3<128,2,2,3,0,256>          conv_igemm_f32<128,2,2,false,0,true,false>
    ring_midrow       conv_igemm_bf16x3<64,1,2,3,0,128>           conv_igemm_f32<64,1,2,false,0,true,false>
    ring_s2_midrow    conv_igemm_bf16x3<64,1,2,3,0,128>           conv_igemm_f32<64,1,2,false,0,true,false>
    ring_long_k       conv_igemm_bf16x3<64,1,2,3,0,128>           conv_igemm_f32<64,1,2,false,0,true,false>
    gen64_x3          conv_igemm_f32<64,1,2,false,0,true,true>    conv_igemm_f32<64,1,2,false,0,true,false>
    gen128_x3         conv_igemm_f32<128,2,2,false,0,true,true>   conv_igemm_f32<128,2,2,false,0,true,false>
    gen_small_cin_x3  conv_igemm_f32<64,1,2,true,0,true,true>     conv_igemm_f32<64,1,2,true,0,true,false>
  batch invariance: ring128 (44 images) and ring_tall (256 images) on the kernels above, one image on
    conv_igemm_bf16x3<64,1,2,3,0,128>
  data gradient, bf16x3
    3x3_s1            conv3x3_halo_bf16x3<64,1,2,3,32,128,0,false>
    3x3_s1_n3         conv_igemm_bf16x3<64,1,2,3,0,128>
    1x1               conv_igemm_bf16x3<64,1,2,3,0,128>
    3x3_s2            conv3x3_halo_bf16x3<64,1,2,3,32,128,1,false>
    conv_transpose    conv_igemm_bf16x3<64,1,2,3,0,128>
  weight gradient (S slices: the reduction that follows)
    per tap fp32 <64>          wgrad_kernel<64>, S 4: reduce_slices4_kernel
    per tap fp32 <128>         wgrad_kernel<128>, S 2: reduce_slices4_kernel
    per tap bf16x3 <64>        wgrad_bf16x3_kernel<64>, S 4: reduce_slices4_kernel
    per tap one step           wgrad_bf16x3_kernel<64>, S 1
    per tap bf16x3 <128>       wgrad_bf16x3_kernel<128>, S 2: reduce_slices4_kernel
    row3 <64,64>               wgrad_row3_bf16x3_kernel<64,64,2,2,2,2>, S 32: reduce_taps_direct_kernel
    row3 <64,128>              wgrad_row3_bf16x3_kernel<64,128,2,2,2,4>, S 8: reduce_taps_direct_kernel
    row3 <128,64>              wgrad_row3_bf16x3_kernel<128,64,4,2,2,2>, S 8: reduce_taps_direct_kernel
    row3 <128,128>             wgrad_row3_bf16x3_kernel<128,128,2,2,2,4>, S 8: reduce_taps_direct_kernel
    row3 <128,128> big filter  wgrad_row3_bf16x3_kernel<128,128,2,2,2,4>, S 4: reduce_taps_kernel
    stem                       wgrad_rowk_c8_bf16x3_kernel<7>, S 4: reduce_taps_direct_kernel
    transposed                 wgrad_bf16x3_kernel<64>, S 4: reduce_slices4_kernel
    row3 <64,64> batch 3       wgrad_row3_bf16x3_kernel<64,64,2,2,2,2>, S 24: reduce_taps_direct_kernel
    bias fp32                  wgrad_kernel<64>, S 4: reduce_slices4_kernel; reduce_slices_kernel for the column sums
"""
import functools

import pytest
import torch

from tests import helpers
from tests.test_gpu_conv_dispatch import _profiled, _squash
from tests.test_gpu_wgrad_dispatch import REDUCE_NAMES, ROW_NAMES, _plan_of
from tests.test_gpu_wgrad_dispatch import _profiled as _profiled_wgrad

pytestmark = pytest.mark.gpu

FWD, DGRAD, WGRAD = helpers.exact_forward_cases(), helpers.exact_dgrad_cases(), helpers.exact_wgrad_cases()
_X3_KERNELS = ("conv3x3_halo_bf16x3<", "conv_igemm_bf16x3<")
BATCHED = ["ring128", "ring_tall"]


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _operands(kind, name, family):
    """(A, B, float64 reference) on the CPU, once per (case, family); treat as read-only"""
    case = helpers.EXACT_KINDS[kind]()[name]
    a, b = helpers.exact_case_operands(kind, name, family, _ncu())
    return a, b, case.op(a, b)


_RUNS = {}


def _forward(name, family, precision):
    """the kernel's output (NCHW, on the CPU) and the names of the conv kernels that ran; one launch per (case, family, precision)"""
    key = (name, family, precision)
    if key not in _RUNS:
        from impersonator_amd import ops
        case = FWD[name]
        x, w, _ = _operands("fwd", name, family)
        xg, wg = _nhwc(x), w.cuda().contiguous()
        y, names = _profiled(lambda: ops.conv2d_forward(xg, wg, None, case.stride, case.pad, False, precision=precision))
        _RUNS[key] = (y.cpu().permute(0, 3, 1, 2), names, xg, wg)
    return _RUNS[key][:2]


@pytest.mark.parametrize("family", helpers.EXACT_FAMILIES)
@pytest.mark.parametrize("name", sorted(FWD))
def test_forward_bf16x3_gives_the_float64_result_bit_for_bit(name, family):
    _, _, ref = _operands("fwd", name, family)
    y, names = _forward(name, family, "bf16x3")
    print("OBSERVED %s %s: %s" % (name, family, names))
    assert len(names) == 1 and names[0].startswith(FWD[name].expect + "<")
    if not name.startswith("ring"):
        assert names[0].endswith(",true>")   # X3: the split inside the register-staged kernel
    assert torch.equal(y, ref.float())


@pytest.mark.parametrize("family", helpers.EXACT_FAMILIES)
@pytest.mark.parametrize("name", sorted(FWD))
def test_forward_fp32_gives_the_float64_result_bit_for_bit(name, family):
    _, _, ref = _operands("fwd", name, family)
    y, names = _forward(name, family, "fp32")
    print("OBSERVED %s %s fp32: %s" % (name, family, names))
    assert len(names) == 1 and names[0].startswith(("conv_igemm_f32<", "conv_igemm_dma_f32<"))
    assert torch.equal(y, ref.float())


@pytest.mark.parametrize("family", helpers.EXACT_FAMILIES)
@pytest.mark.parametrize("name", sorted(DGRAD))
def test_data_gradient_gives_float64_autograd_bit_for_bit(name, family):
    from impersonator_amd import ops
    case = DGRAD[name]
    dy, w, ref = _operands("dgrad", name, family)
    x_shape = (dy.shape[0], case.H, case.W, case.cin)
    dyg, wg = _nhwc(dy), w.cuda().contiguous()
    dx, names = _profiled(lambda: ops.conv2d_backward_data(dyg, wg, x_shape, case.stride, case.pad, case.transposed,
                                                           precision="bf16x3"))
    print("OBSERVED dgrad %s %s: %s" % (name, family, names))
    assert len(names) == 1 and names[0].startswith(_X3_KERNELS) and names[0].startswith(case.expect + "<")
    assert torch.equal(dx.cpu().permute(0, 3, 1, 2), ref.float())


@pytest.mark.parametrize("family", helpers.EXACT_FAMILIES)
@pytest.mark.parametrize("name", sorted(WGRAD))
def test_weight_gradient_gives_float64_autograd_bit_for_bit(name, family):
    from impersonator_amd import ops
    case = WGRAD[name]
    x, dy, ref = _operands("wgrad", name, family)
    with_bias = name == "bias fp32"
    plan_row, S, reduce = _plan_of(case.cin, case.cout, case.k, case.stride, case.pad, x.shape[0], case.H, case.W, case.precision,
                                   case.transposed)
    xg, dyg = _nhwc(x), _nhwc(dy)
    out, names = _profiled_wgrad(lambda: ops.conv2d_backward_weight(xg, dyg, case.w_shape(), case.stride, case.pad, case.transposed,
                                                                    with_bias=with_bias, precision=case.precision))
    print("OBSERVED wgrad %s %s: plan row %d S %d reduce %d, ran %s" % (name, family, plan_row, S, reduce, names))
    assert plan_row == case.expect
    assert (S > 1) == (reduce != 0)
    assert names == [ROW_NAMES[plan_row]] + ([REDUCE_NAMES[reduce]] if S > 1 else []) + (["reduce_slices_kernel"] if with_bias else [])
    dw, dbias = out if with_bias else (out, None)
    assert torch.equal(dw.cpu(), ref.float())
    if with_bias:
        assert torch.equal(dbias.cpu(), dy.double().sum((0, 2, 3)).float())


def test_the_weight_gradient_cases_reach_every_row_and_every_reduction():
    plans = {name: _plan_of(c.cin, c.cout, c.k, c.stride, c.pad, c.batch(_ncu()), c.H, c.W, c.precision, c.transposed)
             for name, c in WGRAD.items()}
    print("OBSERVED plans at %d CUs: %r" % (_ncu(), plans))
    assert {row for row, _, _ in plans.values()} == set(range(len(ROW_NAMES)))
    assert {r for _, S, r in plans.values() if S > 1} == {1, 2, 3}


@pytest.mark.parametrize("name", BATCHED)
def test_an_image_of_a_ring_batch_equals_the_image_run_alone(name):
    """random operands: here the order of an output's products matters, and the instantiations must share it"""
    from impersonator_amd import ops
    case = FWD[name]
    _, _, ref = _operands("fwd", name, "random")
    y, names = _forward(name, "random", "bf16x3")
    _, _, xg, wg = _RUNS[(name, "random", "bf16x3")]
    rel = float((y.double() - ref).abs().max()) / float(ref.abs().max())
    assert rel < helpers.BF16X3_REL
    N = xg.shape[0]
    alone = set()
    for k in sorted({0, N // 2, N - 1}):
        yk, nk = _profiled(lambda: ops.conv2d_forward(xg[k:k + 1].contiguous(), wg, None, case.stride, case.pad, False,
                                                      precision="bf16x3"))
        alone.update(nk)
        assert torch.equal(yk.cpu().permute(0, 3, 1, 2)[0], y[k]), "image %d" % k
    print("OBSERVED %s: batch of %d on %s (rel %.3g), one image on %s" % (name, N, names, rel, sorted(alone)))
    # the comparison crossed instantiations: one image of a Cout >= 128 layer runs the 64-channel tile on 128 rows
    assert alone == {_squash("conv_igemm_bf16x3<64, 1, 2, 3, 0, 128>")} and alone != set(names)
