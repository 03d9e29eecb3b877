"""launch_wgrad (csrc/train.hip) does what its plan says: for the smallest shapes that reach every row of kWgradKernelTable and
every reduction, one lwg_conv2d_backward_weight under the torch profiler -- the wgrad* kernel that ran (demangled, template
arguments included) is the row lwg_wgrad_plan names at this device's CU count, a reduce_* kernel ran exactly when the plan splits
the pixels (S > 1) and it is the one the plan names, and dW meets the bounds of tests/test_gpu_ops.py against float64 autograd.
What the plan itself is on the training shapes is pinned without a device by tests/test_wgrad_plan.py."""
import ctypes
import functools
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_KERNEL = re.compile(r"\b((?:wgrad|reduce)\w*)(<[^<>]*>)?")
_ROW3 = "wgrad_row3_bf16x3_kernel"
ROW_NAMES = ["wgrad_kernel<64>", "wgrad_kernel<128>", "wgrad_bf16x3_kernel<64>", "wgrad_bf16x3_kernel<128>",
             _ROW3 + "<64,64,2,2,2,2>", _ROW3 + "<64,128,2,2,2,4>", _ROW3 + "<128,64,4,2,2,2>", _ROW3 + "<128,128,2,2,2,4>",
             "wgrad_rowk_c8_bf16x3_kernel<7>"]
REDUCE_NAMES = [None, "reduce_slices4_kernel", "reduce_taps_direct_kernel", "reduce_taps_kernel"]
BOUND = {"bf16x3": 3e-5, "fp32": 2e-5}   # relative to the gradient's largest entry, as tests/test_gpu_ops.py

# case -> (Cin, Cout, k, stride, pad, N, H, W, precision, table row)
CASES = {
    "row3 <64,64>": (64, 64, 3, 1, 1, 1, 32, 32, "bf16x3", 4),
    "row3 <64,128>": (128, 64, 3, 1, 1, 1, 8, 32, "bf16x3", 5),
    "row3 <128,64>": (64, 128, 3, 1, 1, 1, 8, 32, "bf16x3", 6),
    "row3 <128,128>": (128, 128, 3, 1, 1, 1, 8, 32, "bf16x3", 7),
    "row3 <128,128> big filter": (256, 256, 3, 1, 1, 1, 8, 32, "bf16x3", 7),   # more than 512 Ki weights: reduce_taps
    "stem": (8, 64, 7, 1, 3, 1, 32, 32, "bf16x3", 8),
    "per tap bf16x3 <64>": (64, 128, 3, 2, 1, 1, 32, 32, "bf16x3", 2),
    "per tap bf16x3 <128>": (128, 256, 3, 2, 1, 1, 16, 16, "bf16x3", 3),
    "per tap fp32 <64>": (64, 128, 3, 2, 1, 1, 32, 32, "fp32", 0),
    "per tap fp32 <128>": (128, 256, 3, 2, 1, 1, 16, 16, "fp32", 1),
    "per tap one step": (64, 64, 3, 1, 1, 1, 4, 4, "bf16x3", 2),               # 16 pixels: nothing to split
}


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan_of(cin, cout, k, stride, pad, N, H, W, precision, transposed=False):
    """lwg_wgrad_plan of a layer at this device's CU count -> (table row, S, reduction)"""
    from impersonator_amd import _lib, ops
    d = ops._desc((N, H, W, cin), cin, cout, k, stride, pad, transposed, precision)
    info = (ctypes.c_longlong * 10)()
    _lib.check(_lib.load().lwg_wgrad_plan(ctypes.byref(d), 0, _ncu(), info))
    return info[1], info[7], info[9]


def _plan(case):
    """lwg_wgrad_plan of a case at this device's CU count -> (table row, S, reduction)"""
    return _plan_of(*CASES[case][:9])


@functools.lru_cache(maxsize=None)
def _problem(cin, cout, k, stride, pad, N, H, W):
    """-> (x, dy as NHWC device tensors, the weight's shape, dW by float64 autograd); shared by the two precisions of a shape"""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(N, cin, H, W, generator=g)
    if cin == 8:
        x[:, 6:] = 0
    wr = (torch.randn(cout, cin, k, k, generator=g) * 0.05).double().requires_grad_(True)
    y = F.conv2d(x.double(), wr, None, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()
    return nhwc(x), nhwc(dy), tuple(wr.shape), wr.grad


def _profiled(fn):
    """fn() under the profiler -> (fn's result, the wgrad* / reduce* kernels that ran, in record order)"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    found = [_KERNEL.search(e.name) for e in prof.events() if e.device_type == DeviceType.CUDA and "lwg" in e.name]
    return out, [re.sub(r"\s+", "", m.group(0)) for m in found if m]


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_launcher_runs_what_the_plan_names(case):
    from impersonator_amd import ops
    cin, cout, k, stride, pad, N, H, W, precision, row = CASES[case]
    plan_row, S, reduce = _plan(case)
    x, dy, w_shape, ref = _problem(cin, cout, k, stride, pad, N, H, W)
    dw, names = _profiled(lambda: ops.conv2d_backward_weight(x, dy, w_shape, stride, pad, precision=precision))
    err = float((dw.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print("OBSERVED %s: plan row %d S %d reduce %d, ran %s, error %.3g" % (case, plan_row, S, reduce, names, err))
    assert plan_row == row
    assert (S > 1) == (reduce != 0)
    assert names == [ROW_NAMES[row]] + ([REDUCE_NAMES[reduce]] if S > 1 else [])
    assert err < BOUND[precision]


def test_the_cases_split_on_every_reduction_and_once_not_at_all():
    """The plan decides S from the CU count: on this device the cases must still cover each reduction behind a split, and no split."""
    plans = {case: _plan(case) for case in CASES}
    print("OBSERVED plans at %d CUs: %r" % (_ncu(), plans))
    assert {r for _, S, r in plans.values() if S > 1} == {1, 2, 3}
    assert any(S == 1 and r == 0 for _, S, r in plans.values())
    assert {row for row, _, _ in plans.values()} == set(range(9))
