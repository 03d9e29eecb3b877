"""Which kernel instantiation launch_conv_igemm (csrc/conv.hip) picks: every route of the dispatcher, pinned by the demangled
kernel name the torch profiler records (template arguments included), and for the bf16x3 kernels by the grid and the wave count
that lwg_conv_trace_launch reports.  A dispatch change that drops the tall tile or the 4-slot ring computes the same values and
would otherwise show as a speed loss at best.

Batches are sized from the device's CU count so that each "every CU still gets a workgroup" threshold is crossed by the
smallest batch that crosses it.  The generator's launch counts were recorded on a 256-CU MI355X."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_KERNEL = re.compile(r"\b((?:conv|stem)\w*)(<[^<>]*>)?")


def _name(record):
    """'void lwg::(anonymous namespace)::conv_igemm_f32<64, 1, 2, ...>(lwg::ConvArgs)' -> 'conv_igemm_f32<64,1,2,...>'"""
    m = _KERNEL.search(record)
    return re.sub(r"\s+", "", m.group(0)) if m else None


def _squash(name):
    return re.sub(r"\s+", "", name)


def _profiled(fn):
    """fn() under the profiler -> (fn's result, names of the conv* / stem* kernels that ran, in record order)"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [_name(e.name) for e in prof.events() if e.device_type == DeviceType.CUDA and "lwg" in e.name]
    return out, [n for n in names if n]


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# case -> (Cin, Cout, k, stride, pad, transposed, H, W, N(ncu), precision): H x W is the INPUT map
_HALO = "conv3x3_halo_bf16x3"
_RING = "conv_igemm_bf16x3"
_F32 = "conv_igemm_f32"
CASES = {
    "halo64": (32, 64, 3, 1, 1, False, 4, 32, lambda ncu: 1, "bf16x3"),
    "halo128": (32, 128, 3, 1, 1, False, 12, 32, lambda ncu: -(-ncu // 3), "bf16x3"),      # Hm % 8 != 0: never tall
    "halo_tall": (32, 128, 3, 1, 1, False, 8, 32, lambda ncu: ncu, "bf16x3"),
    "ct_narrow": (32, 64, 3, 2, 1, True, 4, 32, lambda ncu: 1, "bf16x3"),
    "ct_wide": (32, 128, 3, 2, 1, True, 16, 32, lambda ncu: -(-ncu // 4), "bf16x3"),
    "ring64": (32, 64, 1, 1, 0, False, 4, 32, lambda ncu: 1, "bf16x3"),
    "ring128": (32, 512, 3, 2, 1, False, 24, 64, lambda ncu: 44, "bf16x3"),               # 12 x 32 out: three tiles per image
    "ring_tall": (32, 128, 1, 1, 0, False, 8, 32, lambda ncu: ncu, "bf16x3"),
    "gen_small_cin": (8, 64, 7, 1, 3, False, 16, 16, lambda ncu: 1, "fp32"),
    "gen64": (32, 64, 3, 1, 1, False, 10, 10, lambda ncu: 1, "fp32"),                    # 100 pixels: not whole tiles
    "gen128": (32, 128, 3, 1, 1, False, 10, 10, lambda ncu: 1, "fp32"),
    "gen_small_cin_x3": (8, 64, 7, 1, 3, False, 16, 16, lambda ncu: 1, "bf16x3"),
    "gen64_x3": (32, 64, 3, 1, 1, False, 10, 10, lambda ncu: 1, "bf16x3"),
    "gen128_x3": (32, 128, 3, 1, 1, False, 10, 10, lambda ncu: 1, "bf16x3"),
}
EXPECTED = {
    "halo64": _HALO + "<64, 1, 2, 3, 32, 128, 0, false>",
    "halo128": _HALO + "<128, 2, 2, 4, 32, 128, 0, false>",
    "halo_tall": _HALO + "<128, 2, 2, 4, 32, 256, 0, false>",
    "ct_narrow": _HALO + "<64, 1, 2, 3, 32, 128, 1, false>",
    "ct_wide": _HALO + "<128, 2, 2, 4, 32, 128, 1, false>",
    "ring64": _RING + "<64, 1, 2, 3, 0, 128>",
    "ring128": _RING + "<128, 2, 2, 4, 0, 128>",
    "ring_tall": _RING + "<128, 2, 2, 3, 0, 256>",
    "gen_small_cin": _F32 + "<64, 1, 2, true, 0, true, false>",
    "gen64": _F32 + "<64, 1, 2, false, 0, true, false>",
    "gen128": _F32 + "<128, 2, 2, false, 0, true, false>",
    "gen_small_cin_x3": _F32 + "<64, 1, 2, true, 0, true, true>",
    "gen64_x3": _F32 + "<64, 1, 2, false, 0, true, true>",
    "gen128_x3": _F32 + "<128, 2, 2, false, 0, true, true>",
}
_TRACED_RING = _RING + "<128, 2, 2, 4, 512, 128>"


def _operands(case):
    cin, cout, k, stride, pad, transposed, H, W, n_of, precision = CASES[case]
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(n_of(_ncu()), H, W, cin, generator=g) * 2 - 1).cuda()
    w = (torch.randn((cin, cout, k, k) if transposed else (cout, cin, k, k), generator=g) * 0.05).cuda()
    return x, w, (None, stride, pad, transposed, precision)


def run_case(case, traced=False):
    """one conv2d_forward of `case` under the profiler -> (output, conv kernel names, traced launches as
    (gx, gy, gz, waves, stages) tuples)"""
    from impersonator_amd import _lib, ops
    lib = _lib.load()
    x, w, rest = _operands(case)
    ops.conv2d_forward(x, w, *rest)   # first launch: per-device kernel attributes
    launches = []
    buf = torch.zeros(1 << 20, dtype=torch.int64, device="cuda") if traced else None
    if traced:
        _lib.check(lib.lwg_conv_trace(_lib.ptr(buf), buf.numel() * 8))
    try:
        y, names = _profiled(lambda: ops.conv2d_forward(x, w, *rest))
        info = (ctypes.c_longlong * 10)()
        while traced and lib.lwg_conv_trace_launch(len(launches), info) == 0:
            launches.append(tuple(info)[1:6])
    finally:
        if traced:
            _lib.check(lib.lwg_conv_trace(None, 0))
    return y, names, launches


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv2d_forward_runs_the_expected_instantiation(case):
    y, names, _ = run_case(case)
    print("OBSERVED %s: %s" % (case, names))
    assert names == [_squash(EXPECTED[case])]
    assert bool(torch.isfinite(y).all())


def _mtiles(case):
    cin, cout, k, stride, pad, transposed, H, W, n_of, _ = CASES[case]
    ho, wo = (H, W) if transposed else ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
    return n_of(_ncu()) * ho * wo // 128, cout


@pytest.mark.parametrize("case,bn,rows,waves,stages", [
    ("halo64", 64, 128, 4, 9), ("halo128", 128, 128, 4, 9), ("halo_tall", 128, 256, 8, 9),
    ("ct_narrow", 64, 128, 4, -9), ("ct_wide", 128, 128, 4, -9)])
def test_traced_halo_launch_keeps_the_route_and_the_bits(case, bn, rows, waves, stages):
    """The halo kernels take a trace block themselves: with a record buffer set the same instantiation runs on the same grid
    (one launch for all four phases of a transposed conv; a negative stage count marks one) and every output bit stays."""
    ref, _, none = run_case(case)
    y, names, launches = run_case(case, traced=True)
    print("OBSERVED %s traced: %s %s" % (case, names, launches))
    mtiles, cout = _mtiles(case)
    assert none == [] and names == [_squash(EXPECTED[case])]
    assert launches == [(mtiles // (rows // 128), cout // bn, 1, waves, stages)]
    assert torch.equal(ref, y)


def test_traced_ring_launch_64_channel_tile_is_not_traced():
    ref, _, _ = run_case("ring64")
    y, names, launches = run_case("ring64", traced=True)
    assert names == [_squash(EXPECTED["ring64"])] and launches == []
    assert torch.equal(ref, y)


@pytest.mark.parametrize("case,stages", [("ring128", 9), ("ring_tall", 1)])
def test_traced_ring_launch_takes_the_traced_4_slot_kernel(case, stages):
    """With a record buffer set the 128-channel ring launches -- the 256-row tile included -- run the traced 4-slot kernel on
    128-row tiles; its grid, z included, is recorded.  The products of an output are added in the same order: same bits."""
    ref, _, _ = run_case(case)
    y, names, launches = run_case(case, traced=True)
    print("OBSERVED %s traced: %s %s" % (case, names, launches))
    mtiles, cout = _mtiles(case)
    assert names == [_squash(_TRACED_RING)]
    assert launches == [(mtiles, cout // 128, 1, 4, stages)]
    assert torch.equal(ref, y)


# ---- the A/B switches that redirect a route (read once per process: one short child each)
SWITCHED = {
    "LWG_HALO=0": ("halo64", _RING + "<64, 1, 2, 3, 0, 128>"),
    "LWG_HALO_TALL=0": ("halo_tall", _HALO + "<128, 2, 2, 4, 32, 128, 0, false>"),
    "LWG_CT_WIDE=0": ("ct_wide", _HALO + "<64, 1, 2, 3, 32, 128, 1, false>"),
    "LWG_RING=3": ("ring128", _RING + "<128, 2, 2, 3, 0, 128>"),
    "LWG_RING_TALL=0": ("ring_tall", _RING + "<128, 2, 2, 4, 0, 128>"),
}
_CHILD = ("import sys\n"
          "from tests import test_gpu_conv_dispatch as t\n"
          "print('KERNELS', '|'.join(t.run_case(sys.argv[1])[1]))\n")


@pytest.mark.parametrize("switch", sorted(SWITCHED))
def test_ab_switch_redirects_the_route(switch):
    case, expected = SWITCHED[switch]
    var, val = switch.split("=")
    assert var not in os.environ, "this suite runs with the switches at their defaults"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _CHILD, case], cwd=root, env=dict(os.environ, PYTHONPATH=root, **{var: val}),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = [l for l in p.stdout.splitlines() if l.startswith("KERNELS")][0].split(" ", 1)[1].split("|")
    print("OBSERVED %s: %s" % (switch, got))
    assert got == [_squash(expected)]


# ---- the routes only the generator reaches: exact-fp32 DMA tiles of 32 / 64 / 128 channels, the register-staged fp32 kernels,
# the raw-input halo variants.  One inference at the smallest image size lwg_generator_create takes (128: 16 x 16 trunk maps).
# (the register-staged 64-channel tile, conv_igemm_f32<64, 1, 2, false, 0, false, false>, is taken by no layer of the generator:
# its fp32 convs of 32 channels or more have at most nine taps and a zero run, and go DMA-fed on that tile)
def _generator_counts(precision, batch):
    from impersonator_amd.networks.generator import ImpersonatorGenerator
    from oracle import torch_ref
    from tests import helpers
    G = ImpersonatorGenerator(bg_dim=4, src_dim=6, tsf_dim=6, repeat_num=6, image_size=128, max_batch=batch, precision=precision)
    G.load_state_dict(torch_ref.state_dict_from_numpy(helpers.generator_state_dict(seed=0, affine="random")))
    G = G.cuda()
    g = torch.Generator().manual_seed(5)
    enc, res = G.encode_src((torch.rand(1, 6, 128, 128, generator=g) * 2 - 1).cuda())
    x = (torch.rand(batch, 6, 128, 128, generator=g) * 2 - 1).cuda()
    T = (torch.rand(batch, 128, 128, 2, generator=g) * 2.4 - 1.2).cuda()
    G.inference(enc, res, x, T)   # first pass: scratch, per-device kernel attributes
    _, names = _profiled(lambda: G.inference(enc, res, x, T))
    G.release()
    counts = {}
    for n in names:
        counts[n] = counts.get(n, 0) + 1
    return counts


def _batch(which):
    """the smallest batches that cross the generator's own thresholds (networks at image size 128, 256 tiles of 128 channels
    before the 128-channel tile is taken):
    round:  the 64 -> 128 encoder conv (64 x 64 map: 32 tiles per image) is 256 workgroups of the 128-channel tile, one per CU:
            DMA-fed in fp32;
    staged: one image more queues a second round: the register-staged fp32 kernel;
    wide:   the 256 -> 128 transposed conv (32 x 32 map: 8 tiles per image) gives every CU a 128-channel tile; the 3 x 3 convs
            of the 64 x 64 level have taken the 8 x 32-pixel tile from half that batch on"""
    ncu = _ncu()
    return {1: 1, "round": 8, "staged": max(8, ncu // 32 + 1), "wide": -(-ncu // 8)}[which]


GENERATOR_COUNTS = {
    ("fp32", 1): {
        _F32 + "<64, 1, 2, true, 0, false, false>": 1, "conv_igemm_dma_f32<32, 1, 1, 0, 3>": 18,
        "conv_igemm_dma_f32<64, 1, 2, 0, 3>": 3},
    ("fp32", "round"): {
        _F32 + "<64, 1, 2, true, 0, false, false>": 1, "conv_igemm_dma_f32<128, 2, 2, 0, 3>": 2,
        "conv_igemm_dma_f32<64, 1, 2, 0, 3>": 6, "conv_igemm_dma_f32<32, 1, 1, 0, 3>": 13},
    ("fp32", "staged"): {
        _F32 + "<64, 1, 2, true, 0, false, false>": 1, _F32 + "<128, 2, 2, false, 0, false, false>": 2,
        "conv_igemm_dma_f32<64, 1, 2, 0, 3>": 19},
    ("bf16x3", 1): {
        "stem_bf16x3_kernel": 1, _RING + "<64, 1, 2, 3, 0, 128>": 15, _RING + "<128, 2, 2, 4, 0, 128>": 1,
        _HALO + "<64, 1, 2, 3, 32, 128, 0, true>": 3, _HALO + "<64, 1, 2, 3, 32, 128, 1, true>": 2},
    ("bf16x3", "staged"): {
        "stem_bf16x3_kernel": 1, _RING + "<128, 2, 2, 4, 0, 128>": 2, _RING + "<64, 1, 2, 3, 0, 128>": 14,
        _HALO + "<64, 1, 2, 3, 32, 128, 0, true>": 2, _HALO + "<64, 1, 2, 3, 32, 128, 1, true>": 2,
        _HALO + "<128, 2, 2, 4, 32, 128, 0, true>": 1},
    ("bf16x3", "wide"): {
        "stem_bf16x3_kernel": 1, _RING + "<128, 2, 2, 3, 0, 256>": 2, _RING + "<128, 2, 2, 4, 0, 128>": 14,
        _HALO + "<128, 2, 2, 4, 32, 256, 0, true>": 2, _HALO + "<128, 2, 2, 4, 32, 128, 1, true>": 1,
        _HALO + "<64, 1, 2, 3, 32, 128, 1, true>": 1, _HALO + "<64, 1, 2, 3, 32, 128, 0, true>": 1},
}


@pytest.mark.parametrize("precision,batch", sorted(GENERATOR_COUNTS, key=str))
def test_generator_inference_launch_counts_by_instantiation(precision, batch):
    counts = _generator_counts(precision, _batch(batch))
    print("OBSERVED %s %s: %r" % (precision, batch, counts))
    assert counts == {_squash(k): v for k, v in GENERATOR_COUNTS[(precision, batch)].items()}
