"""The cases of tests/test_gpu_norm_chain.py are honest: without a device, in float64 and in emulated float32.

1. Exact statistics family (helpers.onehot_stat_operands): the raw output of every case is an integer in [-2, 2] times a
   per-channel power of two, the shifted-copy reference equals the float64 conv, and for such values the epilogues' two-level
   reduction is exact in fp32 in ANY order -- re-proved by brute force over shuffled orders on the cases' own tiles.  So a
   partial must equal the float64 statistics of its 128 pixels bit for bit, and every partition / phase / image / channel
   mutant of helpers.STAT_MUTANTS misses them.
2. Random statistics: the figures helpers.NORM_STAT_MEASURED records are measured here from the sequential fp32 restatement.
3. Finalize: the kernel's double arithmetic restated (helpers.finalize_emulated) lands within 1 fp32 ulp of the exact reference
   on exact partials; the conditioning table of include/lwg.h is re-measured against exact rationals.
4. Apply: the exact family is representable (the fp32 restatement, contracted or not, equals float64 bit for bit), every mutant
   of helpers.APPLY_MUTANTS changes a value, and the fp32 tap weights of random flows stay below helpers.APPLY_TAP_MEASURED.
5. Raw-input consumers: the conditions of the exact conv hold and normalised padding changes the result."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers

CPU_NCU = 8   # the CU-sized batches shrink with it; the statements here do not depend on the batch
STAT = sorted(helpers.NORM_STAT_CASES)


@functools.lru_cache(maxsize=None)
def _stat(name):
    case = helpers.norm_case(name, CPU_NCU)
    x, w, ci, e = helpers.onehot_stat_operands(case)
    return case, x, w, ci, e, helpers.onehot_conv_reference(case, x, w)


@pytest.mark.parametrize("name", STAT)
def test_onehot_family_is_what_the_exact_expectations_need(name):
    case, x, w, ci, e, y = _stat(name)
    assert float(x.abs().max()) == 2 and torch.equal(x, x.round())
    assert torch.equal(y, helpers.conv_reference_nhwc(case, x, w)), "shifted copy != float64 conv"
    units = y / torch.pow(2.0, e.double())
    assert torch.equal(units, units.round()) and float(units.abs().max()) == 2      # |y| <= 2 in units of 2^e
    assert int(e.min()) == -6 and int(e.max()) == 6
    assert float(y[..., 0].abs().max()) == 0                                         # the all-zero channel
    for n in range(case.N):                                                          # the constant channel (per phase)
        for ph in helpers.phase_views(case, y)[:, n, ..., 1]:
            assert float(ph.min()) == float(ph.max()) != 0
    assert case.N == 1 or not torch.equal(y[0], y[1])
    # channels differ in input channel (distribution), tap or scale: no two filters are equal, every input channel is used
    rows = (w.transpose(0, 1) if case.transposed else w).reshape(case.cout, -1)
    assert len({tuple(r.tolist()) for r in rows}) == case.cout
    assert len(set(ci.tolist())) == min(case.cin, case.cout)
    used = rows.view(case.cout, case.cin, -1).abs().sum(1).ne(0).sum(0)    # output channels per tap
    assert int((used > 0).sum()) >= (4 if case.transposed else min(case.k * case.k, 9))
    nphase, Hm, Wm = helpers.norm_grid(case)
    ph = helpers.phase_views(case, y)
    for p in range(nphase):
        assert float(ph[p].abs().max()) > 0, "phase %d carries no data" % p
    mean, m2 = helpers.stat_expected(case, y)
    assert tuple(mean.shape) == (nphase, case.N * Hm * Wm // 128, case.cout)
    # M2 <= 512 units^2 on a 2^-14 grid: below 2^24 quanta
    assert float((m2 / torch.pow(4.0, e.double())).max()) <= 512
    assert torch.equal(mean.float().double(), mean) and torch.equal(m2.float().double(), m2)


def test_two_level_reduction_is_exact_in_any_order_on_the_family():
    rng = np.random.default_rng(0)
    tiles = inexact = 0
    for name in ("halo64_8x64", "ct_narrow", "ring128", "small_cin", "dma128"):
        case, _, _, _, _, y = _stat(name)
        nphase, Hm, Wm = helpers.norm_grid(case)
        idx = helpers.stat_partition(case.partition, case.N, Hm, Wm)
        v = helpers.phase_views(case, y).reshape(nphase, -1, case.cout)[:, idx]          # (nphase, mtiles, 128, C)
        v = v.permute(0, 1, 3, 2).reshape(-1, 128)[:: max(1, v.numel() // 128 // 400)]
        ref_mean = v.mean(1)
        ref_m2 = ((v - ref_mean[:, None]) ** 2).sum(1)
        for _ in range(2):
            mean, m2 = helpers.two_level_stats_f32(v.float().numpy(), rng)
            bad = (torch.from_numpy(mean).double() != ref_mean) | (torch.from_numpy(m2).double() != ref_m2)
            tiles += len(v)
            inexact += int(bad.sum())
    # tiles of +-limit only, and tiles whose four groups have means far apart
    lim = torch.where(torch.rand(100, 128, generator=torch.Generator().manual_seed(1)) < 0.5, -2.0, 2.0).double() * 2.0 ** 6
    apart = torch.cat([torch.full((50, 32), s) for s in (2.0, -2.0, 2.0, -2.0)], dim=1).double() * 2.0 ** -6
    for v in (lim, apart):
        mean, m2 = helpers.two_level_stats_f32(v.float().numpy(), rng)
        ref_mean = v.mean(1)
        bad = (torch.from_numpy(mean).double() != ref_mean) | (torch.from_numpy(m2).double() != ((v - ref_mean[:, None]) ** 2).sum(1))
        tiles += len(v)
        inexact += int(bad.sum())
    print("two-level reduction, shuffled sequential orders: %d of %d tiles inexact" % (inexact, tiles))
    assert tiles >= 1200 and inexact == 0


def _differs(a, b):
    return not torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("name,mutant", [
    ("halo64_8x64", "other_partition"), ("ring_wide_map", "other_partition"),
    ("ct_narrow", "swap_phases"), ("ct_wide", "swap_phases"), ("ct_fused_f32", "swap_phases"),
    ("halo64_8x64", "image0_tiles"), ("ring128", "image0_tiles"), ("halo_tall", "image0_tiles"),
    ("halo64", "channel32"), ("halo128", "channel64"), ("ring64", "channel32"), ("dma128", "channel64"), ("dma32", "channel32"),
    ("halo_tall", "tall_stride")])
def test_statistics_mutants_miss_the_expectations(name, mutant):
    case, _, _, _, _, y = _stat(name)
    mean, m2 = helpers.stat_expected(case, y)
    mmean, mm2 = helpers.stat_expected(case, y, mutant)
    assert _differs(mean, mmean) and _differs(m2, mm2)


def test_partitions_coincide_only_where_the_header_says():
    assert torch.equal(helpers.stat_partition("runs", 3, 8, 32), helpers.stat_partition("blocks", 3, 8, 32))      # Wm == 32
    assert not torch.equal(helpers.stat_partition("runs", 3, 8, 64), helpers.stat_partition("blocks", 3, 8, 64))
    blocks = helpers.stat_partition("blocks", 2, 8, 64)
    assert blocks[1].tolist()[:33] == list(range(32, 64)) + [96] and int(blocks[4][0]) == 8 * 64 and int(blocks[6][0]) == 12 * 64


@pytest.mark.parametrize("family", helpers.NORM_RANDOM_FAMILIES)
def test_random_statistics_restatement_error_is_what_helpers_record(family):
    v = helpers.norm_random_tiles(family)
    ref_mean = v.double().mean(-1)
    ref_m2 = ((v.double() - ref_mean[..., None]) ** 2).sum(-1)
    mean, m2 = helpers.two_level_stats_f32(v.numpy())
    e_mean, e_m2 = helpers.stat_errors(torch.from_numpy(mean), torch.from_numpy(m2), ref_mean, ref_m2, float(v.abs().max()))
    rec_mean, rec_m2 = helpers.NORM_STAT_MEASURED[family]
    print("MEASURED random statistics %s: mean %.3g of max|y| (recorded %.3g), M2 %.3g of max M2 (recorded %.3g)"
          % (family, e_mean, rec_mean, e_m2, rec_m2))
    assert rec_mean / 2 <= e_mean <= rec_mean and rec_m2 / 2 <= e_m2 <= rec_m2      # the record is the measurement, not a cushion
    if family == "ratio1024":
        ratio = ref_mean.abs() / (ref_m2 / 128).sqrt()
        assert 1000 < float(ratio.mean()) < 1050 and 700 < float(ratio.min())   # per-tile sample ratios scatter around 2^10


# ---- finalize
@pytest.mark.parametrize("name", ["halo64_8x64", "ct_narrow", "ring128", "small_cin"])
def test_finalize_emulation_within_one_ulp_on_exact_partials(name):
    case, _, _, _, _, y = _stat(name)
    mean, m2 = helpers.stat_expected(case, y)
    g = torch.Generator().manual_seed(3)
    gamma, beta = torch.randn(case.cout, generator=g), torch.randn(case.cout, generator=g)
    ref = helpers.finalize_reference(mean, m2, case.N, gamma, beta)
    # the same from the raw output directly: biased variance over the image
    yd = y.reshape(case.N, -1, case.cout)
    inv = 1 / torch.sqrt(yd.var(1, unbiased=False) + helpers.IN_EPS)
    direct = torch.stack([gamma.double() * inv, beta.double() - yd.mean(1) * gamma.double() * inv], -1)
    assert float(((ref - direct).abs() / direct.abs().clamp(min=1e-30)).max()) < 1e-10
    ulps = helpers.ulp_error(helpers.finalize_emulated(mean.float(), m2.float(), case.N, gamma, beta), ref)
    print("finalize emulation on %s: worst %.3f ulp" % (name, float(ulps.max())))
    assert float(ulps.max()) <= 1.0


@pytest.mark.parametrize("log2_ratio,bound", [(0, 1.0), (6, 1.0), (12, 1.0), (14, None), (16, None)])
def test_finalize_conditioning_table(log2_ratio, bound):
    worst = 0.0
    for seed in range(6):
        mean, m2, gamma, beta = helpers.synthetic_partials(4, 17, 3, 16, ratio=2.0 ** log2_ratio, seed=seed)
        ref = helpers.finalize_reference(mean.double(), m2.double(), 3, gamma, beta, exact=True)
        worst = max(worst, float(helpers.ulp_error(helpers.finalize_emulated(mean, m2, 3, gamma, beta), ref)[:, 2:].max()))
    print("MEASURED finalize emulation at |mean|/std = 2^%d: worst %.3g fp32 ulp" % (log2_ratio, worst))
    if bound is not None:
        assert worst <= bound   # the contract of include/lwg.h is 2 ulp up to 2^12: the emulation keeps half of it free


def test_finalize_reference_exact_and_float64_forms_agree_when_well_conditioned():
    mean, m2, gamma, beta = helpers.synthetic_partials(1, 3, 3, 16)
    a = helpers.finalize_reference(mean.double(), m2.double(), 3, gamma, beta, exact=True)
    b = helpers.finalize_reference(mean.double(), m2.double(), 3, gamma, beta)
    assert float(((a - b).abs() / a.abs().clamp(min=1e-30)).max()) < 1e-12
    assert float(m2[..., 0].abs().max()) == 0 and float(mean[..., 1].abs().max()) == 0


# ---- apply
EXACT_APPLY = [n for n in sorted(helpers.APPLY_CASES) if n.startswith("exact")]
RANDOM_APPLY = [n for n in sorted(helpers.APPLY_CASES) if n.startswith("random")]


@pytest.mark.parametrize("name", EXACT_APPLY)
def test_exact_apply_family_is_representable(name):
    case = helpers.APPLY_CASES[name]
    o = helpers.apply_operands(case)
    ref = helpers.apply_reference(case)
    assert torch.equal(ref.float().double(), ref)
    for fma in (False, True):
        assert torch.equal(helpers.apply_f32(case, fma=fma).double(), ref), "fma=%s" % fma
    hi, lo = helpers.split_bf16_encode(ref.float())
    assert torch.equal(hi.double() + lo.double(), ref)                       # the split form carries the result
    if o["res"] is not None:
        assert float(helpers.bf16_split_f32(o["res"])[1].abs().max()) > 0    # the residual needs its lo term
    ss = o["ss"]
    assert float(ss[..., 1].min()) < 0 < float(ss[..., 1].max()) and float(ss[..., 0].min()) < 0 < float(ss[..., 0].max())
    for _, flow in o["warps"]:
        assert bool((flow == -2).all(-1).any()) and float(flow.abs().max()) > 2
        for size in (case.H, case.W):   # the unnormalise is exact in fp32 at any size
            x0, y0, w = helpers.grid_taps_f32(flow, case.H, case.W, case.align)
            t = helpers.sample_taps(flow, case.H, case.W, case.align, 1)
            assert torch.equal(torch.from_numpy(w).double(), t.w)


def _apply_mutants(case):
    o = helpers.apply_operands(case)
    m = []
    if case.relu:
        m.append("no_relu")
    if o["res"] is not None:
        m.append("res_lo_dropped")
    if "shared" in case.warps:
        m.append("shared_per_sample")
    if "per_sample" in case.warps:
        m.append("per_sample_shared")
    if case.warps:
        m += ["swap_hw", "other_align"]
    if len(case.warps) == 2:
        m.append("second_warp_ignored")
    return m


@pytest.mark.parametrize("name", EXACT_APPLY)
def test_apply_mutants_change_the_expected_values(name):
    case = helpers.APPLY_CASES[name]
    ref = helpers.apply_reference(case)
    for mutant in _apply_mutants(case):
        assert not torch.equal(helpers.apply_reference(case, mutant=mutant), ref), mutant
    # the pixel-stride mutants: the buffer a kernel leaves that took C for ld
    good = helpers.apply_layout_mutant(ref, 2 * case.C, case.C, None)
    assert _differs(good, helpers.apply_layout_mutant(ref, 2 * case.C, case.C, "ld_is_c"))
    assert bool(torch.isnan(good[..., :case.C]).all()) and torch.equal(good[..., case.C:], ref)


def test_every_apply_mutant_is_caught_by_some_case():
    seen = set()
    for name in EXACT_APPLY:
        seen.update(_apply_mutants(helpers.APPLY_CASES[name]))
    assert seen | {"ld_dst_is_c", "ld_res_is_c"} == set(helpers.APPLY_MUTANTS)


@pytest.mark.parametrize("name", RANDOM_APPLY)
def test_random_apply_restatement_and_tap_weight_allowance(name):
    case = helpers.APPLY_CASES[name]
    ref, S = helpers.apply_reference(case, with_S=True)
    worst = float(((helpers.apply_f32(case).double() - ref).abs() / S.clamp(min=1e-30)).max())
    # the share of the fp32 tap weights alone: float64 everywhere except the weights
    tap = 0.0
    o = helpers.apply_operands(case)
    for src, flow in o["warps"]:
        _, _, w32 = helpers.grid_taps_f32(flow, case.H, case.W, case.align)
        t = helpers.sample_taps(flow, case.H, case.W, case.align, src.shape[0])
        xf = src.double().reshape(-1, case.C)
        d = torch.zeros(case.N, case.H, case.W, case.C, dtype=torch.float64)
        for k in range(4):
            dw = torch.where(t.valid[..., k], torch.from_numpy(w32[..., k]).double() - t.w[..., k], torch.zeros_like(t.w[..., k]))
            d = d + dw[..., None].abs() * xf[t.tex[..., k].clamp(min=0).reshape(-1)].view(case.N, case.H, case.W, case.C).abs()
        tap = max(tap, float((d / S.clamp(min=1e-30)).max()))
    print("MEASURED random apply %s: fp32 restatement %.3g of S (bound %.3g), tap weights alone %.3g (recorded %.3g)"
          % (name, worst, helpers.APPLY_REL, tap, helpers.APPLY_TAP_MEASURED))
    assert tap <= helpers.APPLY_TAP_MEASURED
    assert worst <= 2.0 ** -19 + helpers.APPLY_TAP_MEASURED    # the restatement needs none of the 4 x margin


# ---- raw-input consumers
@pytest.mark.parametrize("name,cin,raw_from", [c for c in helpers.RAW_INPUT_CASES if c[0] in ("halo64", "ct_narrow")])
def test_raw_input_family_is_exact_and_padding_shows(name, cin, raw_from):
    case = helpers.raw_input_case(name, cin, CPU_NCU)
    x, ss, w = helpers.raw_input_operands(case, raw_from)
    act = helpers.raw_input_activation(x, ss, raw_from)
    n256 = act * 256
    assert torch.equal(n256, n256.round()) and float(act.max()) <= 511 / 256 and float(act[..., raw_from:].min()) == 0
    assert float(helpers.bf16_split_f32(act.float())[1].abs().max()) > 0       # the activation needs its lo term
    assert float(helpers.bf16_split_f32(w)[1].abs().max()) == 0                # the weights do not
    # what the kernel computes in fp32 -- fmaf or multiply then add -- is the float64 activation
    raw, s, t = x[..., raw_from:], ss[:, None, None, :, 0], ss[:, None, None, :, 1]
    assert torch.equal((raw * s + t).clamp(min=0).double(), act[..., raw_from:])
    ref = helpers.raw_input_reference(case, x, ss, w, raw_from)
    assert torch.equal(ref.float().double(), ref)
    quanta = helpers.conv_reference_nhwc(case, act.float().abs(), w.abs()) * 4096
    assert float(quanta.max()) < 2 ** 24
    assert float(ss[..., 1].max()) > 0
    assert not torch.equal(helpers.raw_input_reference(case, x, ss, w, raw_from, pad_normalised=True), ref)
