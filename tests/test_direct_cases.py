"""CPU side of tests/test_gpu_direct_kernels.py: the bounds that file holds stem_bf16x3_kernel and heads_bf16x3_kernel to are
honest.  On every input of the GPU tests, built from its seed, the float64 restatement of the split arithmetic (tests/helpers.py:
hi = bf16(v), lo = bf16(v - hi), products lo*hi + hi*lo + hi*hi) sits inside ONE THIRD of the bound, so a kernel that misses a
bound is wrong, not the bound; and a restatement with one cross product dropped, or with the padding normalised, misses it."""
import pytest
import torch

from tests import helpers

STEM_IDS = ["%dx%dx%d-cin%d" % c[:4] for c in helpers.STEM_CASES]
HEADS_IDS = ["%dx%dx%d-w%d" % c[:4] for c in helpers.HEADS_CASES]


def _max(a, b):
    return float((a - b).abs().max())


@pytest.mark.parametrize("case", helpers.STEM_CASES, ids=STEM_IDS)
def test_stem_restatement_is_inside_a_third_of_the_gpu_bounds(case):
    """Measured: restatement 3.6e-6 to 4.6e-6 of max |ref| on the output (bound 3e-5), 2.1e-7 to 2.5e-7 on the tile means, M2 1.7e-6
    to 2.2e-6 relative (its bound is ten times helpers.STEM_M2_MEASURED, which no case may exceed); a dropped cross product moves the
    output by 1.2e-3 to 1.9e-3."""
    N, H, W, cin, _ = case
    c = helpers.stem_case(N, H, W, cin)
    scale = float(c["ref"].abs().max())
    y = helpers.conv7_bf16x3(c["x"], c["w"]).permute(0, 2, 3, 1)
    err = _max(y, c["ref"]) / scale
    mean, m2 = helpers.tile_stats(y)
    mean_err = _max(mean, c["mean"]) / scale
    m2_err = _max(m2, c["m2"]) / float(c["m2"].abs().max())
    print("stem %s: restatement %.3g of max|ref| = %.3g, tile mean %.3g, M2 %.3g relative" % (case[:4], err, scale, mean_err, m2_err))
    assert err < helpers.BF16X3_REL / 3 and mean_err < helpers.BF16X3_REL / 3
    assert m2_err <= helpers.STEM_M2_MEASURED, "the M2 bound is ten times a figure measured HERE: measure again"
    assert m2_err < helpers.STEM_M2_REL / 3
    for drop in ("lo_hi", "hi_lo"):
        moved = _max(helpers.conv7_bf16x3(c["x"], c["w"], drop).permute(0, 2, 3, 1), c["ref"]) / scale
        print("    without %s: %.3g" % (drop, moved))
        assert moved > 10 * helpers.BF16X3_REL
    # the garbage channels are there and are not what the reference saw
    assert float(c["x8"][..., cin:].abs().min()) >= 500.0 and float(c["x8"][..., :cin].abs().max()) <= 1.0


@pytest.mark.parametrize("case", helpers.HEADS_CASES, ids=HEADS_IDS)
def test_heads_restatement_is_inside_a_third_of_the_gpu_bounds(case):
    """Measured: restatement 3.4e-6 to 5.8e-6 of max |pre-activation|, at most 2.3e-5 absolute on the colour (bounds 5.4e-5 to
    2.0e-4) and 6.0e-6 on the mask (bounds 2.1e-5 to 5.7e-5); a dropped cross product moves the colour by 1.6e-3 to 8.7e-3,
    normalised padding by 0.71 to 1.46."""
    N, H, W, w_rows, _ = case
    c = helpers.heads_case(N, H, W, w_rows)
    ref = c["ref"]
    tol_c, tol_m = helpers.heads_bounds(c, "bf16x3")
    out = helpers.heads_restatement(c)
    pre_max = float(ref["pre"].abs().max())
    print("heads %s: max|pre| %.3g, restatement pre %.3g relative, colour %.3g (bound %.3g), mask %.3g (bound %.3g), pred %.3g" %
          (case[:4], pre_max, _max(out["pre"], ref["pre"]) / pre_max, _max(out["color"], ref["color"]), tol_c,
           _max(out["mask"], ref["mask"]), tol_m, _max(out["pred"], ref["pred"])))
    assert _max(out["pre"], ref["pre"]) < helpers.BF16X3_REL * pre_max / 3
    assert _max(out["color"], ref["color"]) < tol_c / 3
    assert _max(out["mask"], ref["mask"]) < tol_m / 3
    assert _max(out["pred"], ref["pred"]) < tol_c / 3
    # the inputs do what they are meant to: negative scales, positive shifts, garbage in the unused weight rows
    assert float(c["ss"][..., 0].min()) < -0.5 and float(c["ss"][..., 1].max()) > 0.25
    assert w_rows == 4 or float(c["w"][4:].abs().mean()) > 1.0
    for drop in ("lo_hi", "hi_lo"):
        moved = _max(helpers.heads_restatement(c, drop)["color"], ref["color"])
        print("    without %s: colour moves by %.3g" % (drop, moved))
        assert moved > 3 * tol_c
    moved = _max(helpers.heads_restatement(c, pad_relu_shift=True)["color"], ref["color"])
    print("    padding with relu(shift): colour moves by %.3g" % moved)
    assert moved > 100 * tol_c


def test_heads_cases_cover_every_residue_of_the_ring():
    """One band of H rows takes H + 6 steps; the slot the last output row is read from is (H + 5) mod 8."""
    assert sorted({(c[1] + 5) % 8 for c in helpers.HEADS_CASES if c[2] == 27}) == list(range(8))


def test_bf16_split_carries_sixteen_bits():
    g = torch.Generator().manual_seed(5)
    v = torch.randn(4096, generator=g)
    hi, lo = helpers.bf16_split(v)
    assert float((hi + lo - v.double()).abs().max() / v.abs().max()) <= 2.0 ** -17
    assert torch.equal(hi.to(torch.bfloat16).double(), hi) and torch.equal(lo.to(torch.bfloat16).double(), lo)
