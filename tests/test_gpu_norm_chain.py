"""The inference path's norm chain, link by link, against float64: conv with its statistics epilogue (lwg_norm_conv_forward),
in_finalize (lwg_norm_finalize), apply / apply8 (lwg_norm_apply) and the raw-input halo consumers -- at rectangular maps, channel
and tile counts that are no powers of two, and with the kernel instantiation pinned by the profiler's kernel name.

The expectations and their conditions are proved without a device in tests/test_norm_chain_cases.py; which 128 pixels a partial
covers is the text of include/lwg.h (helpers.stat_partition).  Every output buffer and workspace starts as NaN (the wrappers of
impersonator_amd/ops.py fill them), so an element a kernel does not write fails the comparison.

Not reachable from the dispatcher: the TC2 > 0 form of igemm_epilogue (2-D blocks on the ring kernels) is instantiated by no
kernel of the table -- the halo kernels have their own epilogue -- so the ring case with a map wider than 128 ('ring_wide_map')
checks the consecutive-run partition there instead."""
import functools
import re

import pytest
import torch

from tests import helpers
from tests.test_gpu_conv_dispatch import _name, _ncu

pytestmark = pytest.mark.gpu

STAT = sorted(helpers.NORM_STAT_CASES)


def _kernels(fn):
    """fn() under the profiler -> (result, raw names of the device kernels of this library that ran)"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "lwg" in e.name]


def _conv_names(names):
    return [n for n in (_name(r) for r in names) if n]


def _apply_names(names):
    return [m.group(0) for m in (re.search(r"\bapply8?_kernel\b", r) for r in names) if m]


def _run_conv(case, x, w, **kw):
    from impersonator_amd import ops
    return ops.norm_conv_forward(x.cuda(), w.cuda(), stride=case.stride, pad=case.pad, transposed=case.transposed,
                                 precision=case.precision, bn=kw.pop("bn", case.bn), **kw)


@functools.lru_cache(maxsize=None)
def _exact_stat(name):
    """case, operands and the float64 expectations of the exact family, once per process; read-only"""
    case = helpers.norm_case(name, _ncu())
    x, w, _, _ = helpers.onehot_stat_operands(case)
    y = helpers.onehot_conv_reference(case, x, w)
    mean, m2 = helpers.stat_expected(case, y)
    return case, x, w, y, mean, m2


def _assert_partials(partials, mean, m2):
    p = partials.cpu().double()
    assert not bool(torch.isnan(p).any()), "a partial was not written"
    assert torch.equal(p[..., 0], mean), "mean: %d of %d differ" % (int((p[..., 0] != mean).sum()), mean.numel())
    assert torch.equal(p[..., 1], m2), "M2: %d of %d differ" % (int((p[..., 1] != m2).sum()), m2.numel())


@pytest.mark.parametrize("name", STAT)
def test_exact_statistics_and_finalize_per_instantiation(name):
    from impersonator_amd import ops
    case, x, w, y_ref, mean, m2 = _exact_stat(name)
    (y, partials, variant), names = _kernels(lambda: _run_conv(case, x, w))
    print("OBSERVED %s: %s (variant %s)" % (name, _conv_names(names), ops.conv_variant_name(variant)))
    assert _conv_names(names) == [case.kernel]
    assert torch.equal(y.cpu().double(), y_ref)
    _assert_partials(partials, mean, m2)
    # finalize from the device's own partials: 1 fp32 ulp of the float64 reference on every element
    g = torch.Generator().manual_seed(21)
    gamma, beta = torch.randn(case.cout, generator=g), torch.randn(case.cout, generator=g)
    ss = ops.norm_finalize(partials, case.N, gamma.cuda(), beta.cuda(), helpers.IN_EPS).cpu()
    ulps = helpers.ulp_error(ss, helpers.finalize_reference(mean, m2, case.N, gamma, beta))
    print("MEASURED finalize %s: worst %.3f ulp" % (name, float(ulps.max())))
    assert float(ulps.max()) <= 1.0


@pytest.mark.parametrize("name", STAT)
def test_random_statistics_against_float64_of_the_device_output(name):
    case = helpers.norm_case(name, _ncu())
    g = torch.Generator().manual_seed(31 + STAT.index(name))
    x = torch.randn(case.N, case.H, case.W, case.cin, generator=g)
    w = torch.randn(case.w_shape(), generator=g) * 0.05
    y, partials, _ = _run_conv(case, x, w)
    y = y.cpu()
    assert bool(torch.isfinite(y).all())
    mean, m2 = helpers.stat_expected(case, y)
    e_mean, e_m2 = helpers.stat_errors(partials[..., 0].cpu(), partials[..., 1].cpu(), mean, m2, float(y.abs().max()))
    b_mean, b_m2 = helpers.NORM_STAT_REL["offset"]
    print("MEASURED random statistics %s: mean %.3g (bound %.3g), M2 %.3g (bound %.3g)" % (name, e_mean, b_mean, e_m2, b_m2))
    assert e_mean <= b_mean and e_m2 <= b_m2


@pytest.mark.parametrize("name", ["ring64", "halo64_8x64", "dma64"])
def test_random_statistics_at_mean_over_std_1024(name):
    """|mean| / std = 2^10 in every channel: a one-hot weight per output channel copies an input channel of 1024 + N(0, 1)."""
    case = helpers.norm_case(name, _ncu())
    g = torch.Generator().manual_seed(41)
    x = (torch.randn(case.N, case.H, case.W, case.cin, generator=g) + 1024.0) * \
        torch.pow(2.0, torch.randint(-3, 4, (case.cin,), generator=g).float())
    w = torch.zeros(case.w_shape())
    co = torch.arange(case.cout)
    w[co, co % case.cin, case.k // 2, case.k // 2] = (torch.randint(0, 2, (case.cout,), generator=g).float() * 2 - 1)
    y, partials, _ = _run_conv(case, x, w)
    y = y.cpu()
    mean, m2 = helpers.stat_expected(case, y)
    e_mean, e_m2 = helpers.stat_errors(partials[..., 0].cpu(), partials[..., 1].cpu(), mean, m2, float(y.abs().max()))
    b_mean, b_m2 = helpers.NORM_STAT_REL["ratio1024"]
    print("MEASURED ratio-1024 statistics %s: mean %.3g (bound %.3g), M2 %.3g (bound %.3g)" % (name, e_mean, b_mean, e_m2, b_m2))
    assert e_mean <= b_mean and e_m2 <= b_m2


@pytest.mark.parametrize("family", helpers.EXACT_FAMILIES)
@pytest.mark.parametrize("name", helpers.NORM_F32_CASES)
def test_exact_fp32_kernels_raw_output_bit_for_bit(name, family):
    """The non-general fp32 kernels' sums, which no other test holds to anything: operands on the coarse binary grid of
    helpers.exact_operands, float64 conv rounded to fp32 is the specification."""
    case = helpers.norm_case(name, _ncu())
    g = torch.Generator().manual_seed(51 + helpers.NORM_F32_CASES.index(name))
    a, w = helpers.exact_operands(family, (case.N, case.cin, case.H, case.W), case.w_shape(), g)
    cond, ref = helpers.exact_conditions(a, w, case.op, family)
    assert all(cond.values()), cond
    x = a.permute(0, 2, 3, 1).contiguous()
    (y, partials, _), names = _kernels(lambda: _run_conv(case, x, w))
    assert _conv_names(names) == [case.kernel]
    ref = ref.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(y.cpu().double(), ref), "%d outputs differ" % int((y.cpu().double() != ref).sum())
    assert not bool(torch.isnan(partials).any())


def test_fp32_tile_widths_give_equal_bits():
    """32-, 64- and (one round) 128-channel tiles add the products of an output in the same order"""
    case = helpers.norm_case("dma128", _ncu())
    g = torch.Generator().manual_seed(61)
    x = torch.randn(case.N, case.H, case.W, case.cin, generator=g)
    w = torch.randn(case.w_shape(), generator=g) * 0.05
    y32, p32, _ = _run_conv(case, x, w, bn=32)
    for bn in (64, 128):
        y, p, _ = _run_conv(case, x, w, bn=bn)
        assert torch.equal(y, y32) and torch.equal(p, p32), bn


# ---- finalize on synthetic partials
@pytest.mark.parametrize("C", [16, 64, 72])
@pytest.mark.parametrize("nphase", [1, 4])
@pytest.mark.parametrize("tiles", [1, 3, 17, 64])
def test_finalize_synthetic_partials_within_one_ulp(tiles, nphase, C):
    from impersonator_amd import ops
    N = 3
    mean, m2, gamma, beta = helpers.synthetic_partials(nphase, tiles, N, C)
    ref = helpers.finalize_reference(mean.double(), m2.double(), N, gamma, beta, exact=True)
    partials = torch.stack([mean, m2], dim=-1).contiguous().cuda()
    ss = ops.norm_finalize(partials, N, gamma.cuda(), beta.cuda(), helpers.IN_EPS).cpu()
    assert not bool(torch.isnan(ss).any())
    ulps = helpers.ulp_error(ss, ref)
    print("MEASURED finalize tiles %d nphase %d C %d: worst %.3f ulp" % (tiles, nphase, C, float(ulps.max())))
    assert float(ulps.max()) <= 1.0


@pytest.mark.parametrize("log2_ratio", [0, 6, 12, 14, 16])
def test_finalize_conditioning_contract(log2_ratio):
    """include/lwg.h: 2 ulp for |mean| / std <= 2^12; beyond, the measured figures are printed beside the emulation's
    (tests/test_norm_chain_cases.py: about 1.4 ulp at 2^14 and 14 at 2^16 on these partial sets), not asserted."""
    from impersonator_amd import ops
    N, C = 3, 16
    worst = worst_emu = 0.0
    for seed in range(6):
        mean, m2, gamma, beta = helpers.synthetic_partials(4, 17, N, C, ratio=2.0 ** log2_ratio, seed=seed)
        ref = helpers.finalize_reference(mean.double(), m2.double(), N, gamma, beta, exact=True)
        partials = torch.stack([mean, m2], dim=-1).contiguous().cuda()
        ss = ops.norm_finalize(partials, N, gamma.cuda(), beta.cuda(), helpers.IN_EPS).cpu()
        worst = max(worst, float(helpers.ulp_error(ss, ref).max()))
        worst_emu = max(worst_emu, float(helpers.ulp_error(helpers.finalize_emulated(mean, m2, N, gamma, beta), ref).max()))
    print("MEASURED finalize at |mean|/std = 2^%d: device %.3g ulp, emulation %.3g ulp" % (log2_ratio, worst, worst_emu))
    if log2_ratio <= 12:
        assert worst <= 2.0


# ---- apply
def _pack_split(r):
    """fp32 (..., C), C % 32 == 0 -> the split-bf16 buffer of the same shape (helpers.split_bf16_decode's inverse)"""
    hi, lo = helpers.split_bf16_encode(r)
    lead, C = r.shape[:-1], r.shape[-1]
    both = torch.stack([hi.reshape(-1, C // 32, 32), lo.reshape(-1, C // 32, 32)], dim=2)    # (P, C/32, 2, 32) bf16
    return both.reshape(-1, 2 * C).view(torch.float32).reshape(lead + (C,)).contiguous()


def _run_apply(case, o, split, lanes):
    """One call into the upper half of a NaN-filled (N,H,W,2C) buffer, the residual read from the upper half of another.
    -> (the buffer on the CPU, apply kernel names)"""
    from impersonator_amd import ops
    N, H, W, C = case.N, case.H, case.W, case.C
    nan = float("nan")
    dst = torch.full((N, H, W, 2 * C), nan, device="cuda")
    res = None
    if o["res"] is not None:
        res = torch.full((N, H, W, 2 * C), nan)
        res[..., C:] = _pack_split(o["res"]) if split else o["res"]
        res = res.cuda()
    warps = [(s.cuda(), f.cuda()) for s, f in o["warps"]]
    _, names = _kernels(lambda: ops.norm_apply(o["raw"].cuda(), o["ss"].cuda(), relu=bool(case.relu), dst=dst, dst_offset=C, res=res,
                                               res_offset=C, split=split, warps=warps, align_corners=bool(case.align), lanes=lanes))
    return dst.cpu(), _apply_names(names)


@pytest.mark.parametrize("name", sorted(helpers.APPLY_CASES))
def test_apply_against_float64(name):
    case = helpers.APPLY_CASES[name]
    o = helpers.apply_operands(case)
    C = case.C
    ref, S = helpers.apply_reference(case, with_S=True)
    exact = case.family == "exact"

    def check(got, what):
        assert not bool(torch.isnan(got).any()), what
        if exact:
            assert torch.equal(got.double(), ref), "%s: %d values differ" % (what, int((got.double() != ref).sum()))
        else:
            worst = float(((got.double() - ref).abs() / S.clamp(min=1e-30)).max())
            print("MEASURED apply %s %s: %.3g of S (bound %.3g)" % (name, what, worst, helpers.APPLY_REL))
            assert worst <= helpers.APPLY_REL

    buf, names = _run_apply(case, o, 0, 4)
    assert names == ["apply_kernel"]
    assert bool(torch.isnan(buf[..., :C]).all()), "the other half of the buffer was written"
    y32 = buf[..., C:].contiguous()
    check(y32, "fp32 lanes 4")
    assert torch.equal(_run_apply(case, o, 0, 0)[0][..., C:], y32)
    if C % 32 or (not exact and case.res == "fp32"):   # (a random fp32 residual has no split form)
        return
    want_hi, want_lo = helpers.split_bf16_encode(y32.reshape(-1, C))
    for lanes, kernel in ((4, "apply_kernel"), (8, "apply8_kernel"), (0, "apply8_kernel")):
        buf, names = _run_apply(case, o, 1, lanes)
        assert names == [kernel]
        assert bool(torch.isnan(buf[..., :C]).all()), "the other half of the buffer was written"
        hi, lo = helpers.split_bf16_decode(buf[..., C:].reshape(-1, C))
        assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo), "split, lanes %d" % lanes


# ---- raw-input consumers
@pytest.mark.parametrize("name,cin,raw_from", helpers.RAW_INPUT_CASES)
def test_raw_input_consumer_against_float64_and_against_apply_then_conv(name, cin, raw_from):
    from impersonator_amd import ops
    case = helpers.raw_input_case(name, cin, _ncu())
    x, ss, w = helpers.raw_input_operands(case, raw_from)
    ref = helpers.raw_input_reference(case, x, ss, w, raw_from)
    (y, partials, _), names = _kernels(lambda: _run_conv(case, x, w, in_scale_shift=ss.cuda(), raw_from=raw_from))
    print("OBSERVED raw %s cin %d from %d: %s" % (name, cin, raw_from, _conv_names(names)))
    assert _conv_names(names) == [case.kernel.replace("false>", "true>")]
    assert torch.equal(y.cpu().double(), ref), "%d outputs differ" % int((y.cpu().double() != ref).sum())
    # the same through apply (split) and the plain conv: bit-equal, partials included
    nr = cin - raw_from
    act = ops.norm_apply(x[..., raw_from:].contiguous().cuda(), ss.cuda(), relu=True, split=True, lanes=8).cpu()
    hi, lo = helpers.split_bf16_decode(act.reshape(-1, nr))
    x2 = x.clone()
    x2[..., raw_from:] = (hi.float() + lo.float()).view(x.shape[:3] + (nr,))
    y2, partials2, _ = _run_conv(case, x2, w)
    assert torch.equal(y2, y) and torch.equal(partials2, partials)
    assert not bool(torch.isnan(partials).any())


def test_raw_input_refusals():
    from impersonator_amd import _lib
    case = helpers.raw_input_case("halo64", 64, _ncu())
    x, ss, w = helpers.raw_input_operands(case, 32)
    with pytest.raises(_lib.LwgError) as e:
        _run_conv(case, x, w, in_scale_shift=torch.zeros(case.N, 48, 2).cuda(), raw_from=16)
    assert e.value.code == -2
    ring = helpers.raw_input_case("ring64", 64, _ncu())
    xr, ssr, wr = helpers.raw_input_operands(ring, 0)
    with pytest.raises(_lib.LwgError) as e:
        _run_conv(ring, xr, wr, in_scale_shift=ssr.cuda(), raw_from=0)
    assert e.value.code == -2


# ---- the whole chain once
@pytest.mark.parametrize("name", ["halo64_8x64", "ct_narrow"])
def test_conv_finalize_apply_against_float64_instance_norm(name):
    from impersonator_amd import ops
    case = helpers.norm_case(name, _ncu())
    g = torch.Generator().manual_seed(71)
    x = torch.randn(case.N, case.H, case.W, case.cin, generator=g)
    w = torch.randn(case.w_shape(), generator=g) * 0.05
    gamma, beta = torch.rand(case.cout, generator=g) + 0.5, torch.randn(case.cout, generator=g) * 0.3
    y, partials, _ = _run_conv(case, x, w)
    ss = ops.norm_finalize(partials, case.N, gamma.cuda(), beta.cuda(), helpers.IN_EPS)
    out = ops.norm_apply(y, ss, relu=True).cpu()
    yd = helpers.conv_reference_nhwc(case, x, w)
    flat = yd.reshape(case.N, -1, case.cout)
    norm = (flat - flat.mean(1, keepdim=True)) / torch.sqrt(flat.var(1, unbiased=False, keepdim=True) + helpers.IN_EPS)
    ref = (norm * gamma.double() + beta.double()).clamp(min=0).view(yd.shape)
    d, where = helpers.maxdiff(out, ref)
    rel = helpers.BF16X3_REL if case.precision == "bf16x3" else helpers.FP32_REL
    print("MEASURED chain %s: max diff %.3g, bound %.3g = %.3g x max |ref|" % (name, d, rel * float(ref.abs().max()), rel))
    assert d <= rel * float(ref.abs().max()), where
