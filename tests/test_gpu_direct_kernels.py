"""stem_bf16x3_kernel (csrc/direct.hip) and heads_bf16x3_kernel (csrc/heads.hip) on their own, against float64, at the geometry the
whole-generator tests never reach: through lwg_stem_forward / lwg_heads_inference, which run the generator's launch code with two
overrides (max_workgroups, bands).  Inputs, references and bounds come from tests/helpers.py; tests/test_direct_cases.py shows on
the CPU that a float64 restatement of the split arithmetic sits inside a third of every bound used here, and that dropping one of
the three products, or normalising the padding, misses them by a wide margin."""
import functools
import itertools

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

STEM_IDS = ["%dx%dx%d-cin%d" % c[:4] for c in helpers.STEM_CASES]
HEADS_IDS = ["%dx%dx%d-w%d" % c[:4] for c in helpers.HEADS_CASES]
PRECISIONS = ("bf16x3", "fp32")


def _max(a, b):
    return float((a.double() - b.double()).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# stem
@functools.lru_cache(maxsize=None)
def _stem(N, H, W, cin, precision, max_workgroups, image=None):
    """(y, partials) on the CPU of one stem case (shared: read-only); image: run that image of the batch alone."""
    from impersonator_amd import ops
    c = helpers.stem_case(N, H, W, cin)
    x8 = c["x8"] if image is None else c["x8"][image:image + 1]
    y, partials = ops.stem_forward(x8.contiguous().cuda(), c["w"], precision, True, max_workgroups)
    return y.cpu(), partials.cpu()


@pytest.mark.parametrize("case", helpers.STEM_CASES, ids=STEM_IDS)
def test_stem_against_float64(case):
    """Raw output within 3e-5 of max |ref| (bf16x3) and 1e-5 (the fp32 kernel on the same arguments), the (mean, M2) partials of
    each 128-pixel tile against float64 statistics of the reference, the garbage in channels cin..7 ignored."""
    N, H, W, cin, grids = case
    c = helpers.stem_case(N, H, W, cin)
    scale, m2_scale = float(c["ref"].abs().max()), float(c["m2"].abs().max())
    y32, p32 = _stem(N, H, W, cin, "fp32", 0)
    err32 = _max(y32, c["ref"]) / scale
    print("stem %s fp32: %.3g of max|ref| (bound %.3g), mean %.3g, M2 %.3g relative" %
          (case[:4], err32, helpers.FP32_REL, _max(p32[..., 0], c["mean"]) / scale, _max(p32[..., 1], c["m2"]) / m2_scale))
    assert err32 <= helpers.FP32_REL
    assert _max(p32[..., 0], c["mean"]) <= helpers.FP32_REL * scale and _max(p32[..., 1], c["m2"]) <= helpers.STEM_M2_REL * m2_scale
    for grid in grids:
        y, p = _stem(N, H, W, cin, "bf16x3", grid)
        err, mean_err, m2_err = _max(y, c["ref"]) / scale, _max(p[..., 0], c["mean"]) / scale, _max(p[..., 1], c["m2"]) / m2_scale
        print("stem %s bf16x3, max_workgroups %d: %.3g of max|ref| (bound %.3g), mean %.3g, M2 %.3g relative (bound %.3g)" %
              (case[:4], grid, err, helpers.BF16X3_REL, mean_err, m2_err, helpers.STEM_M2_REL))
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(p).all()), "an output the kernel did not write"
        assert err <= helpers.BF16X3_REL
        assert not torch.equal(y, y32), "the bf16x3 route did not run"
        assert mean_err <= helpers.BF16X3_REL
        assert m2_err <= helpers.STEM_M2_REL


def test_stem_schedule_changes_no_bit():
    """One workgroup, two, or the launcher's grid: six, three or one tile per four-wave group, same bits in output and partials."""
    for N, H, W, cin, grids in ((3, 4, 256, 6, (1, 2, 0)), (1, 6, 128, 6, (1, 0)), (2, 8, 384, 6, (0, 1, 3))):
        y0, p0 = _stem(N, H, W, cin, "bf16x3", grids[0])
        for grid in grids[1:]:
            y, p = _stem(N, H, W, cin, "bf16x3", grid)
            assert torch.equal(y, y0) and torch.equal(p, p0), (N, H, W, grid)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stem_image_alone_equals_image_in_batch(precision):
    N, H, W, cin = 3, 4, 256, 6
    tiles = H * W // 128
    for grid in ((0, 1) if precision == "bf16x3" else (0,)):
        y, p = _stem(N, H, W, cin, precision, grid)
        for i in range(N):
            yi, pi = _stem(N, H, W, cin, precision, grid, i)
            assert torch.equal(yi[0], y[i]) and torch.equal(pi, p[i * tiles:(i + 1) * tiles]), (precision, grid, i)


# ---------------------------------------------------------------------------------------------------------------------
# heads
@functools.lru_cache(maxsize=None)
def _heads(N, H, W, w_rows, precision, bands=0, outputs=("color", "mask", "pred"), bg_bs=None, image=None):
    """Outputs on the CPU of one heads case (shared: read-only).  bg_bs 1: the first image's background for the whole batch;
    'repeat': the same, repeated N times; image: run that image of the batch alone (with its own background)."""
    from impersonator_amd import ops
    c = helpers.heads_case(N, H, W, w_rows)
    x, ss, bg = c["x"], c["ss"], c["bg"]
    if image is not None:
        x, ss, bg = x[image:image + 1], ss[image:image + 1], bg[image:image + 1]
    if bg_bs == 1:
        bg = bg[:1]
    elif bg_bs == "repeat":
        bg = bg[:1].repeat(x.shape[0], 1, 1, 1)
    out = ops.heads_inference(x.contiguous().cuda(), ss.contiguous().cuda(), c["w"].cuda(), precision, bg.contiguous().cuda(),
                              outputs, bands)
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("case", helpers.HEADS_CASES, ids=HEADS_IDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_heads_against_float64(precision, case):
    """Colour, mask and blend against float64 conv2d + tanh / sigmoid on relu(x * scale + shift) with zero padding after the
    normalisation; every band count of the case gives the same bits (fp32: one kernel, no bands)."""
    N, H, W, w_rows, band_list = case
    c = helpers.heads_case(N, H, W, w_rows)
    ref = c["ref"]
    tol_c, tol_m = helpers.heads_bounds(c, precision)
    first = None
    for bands in (band_list if precision == "bf16x3" else (0,)):
        out = _heads(N, H, W, w_rows, precision, bands)
        ec, em, ep = _max(out["color"], ref["color"]), _max(out["mask"], ref["mask"]), _max(out["pred"], ref["pred"])
        m, col = out["mask"].double(), out["color"].double()
        blend = _max(out["pred"], m * c["bg"].double() + (1 - m) * col)
        print("heads %s %s bands %d: colour %.3g (bound %.3g), mask %.3g (bound %.3g), pred %.3g, pred vs own blend %.3g" %
              (case[:4], precision, bands, ec, tol_c, em, tol_m, ep, blend))
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), "an output the kernel did not write"
        assert ec <= tol_c
        assert em <= tol_m
        assert ep <= tol_c
        assert blend <= 1e-6
        if first is None:
            first = out
        else:
            assert all(torch.equal(out[k], first[k]) for k in out), "bands=%d changes bits" % bands


@pytest.mark.parametrize("case", [helpers.HEADS_CASES[7], helpers.HEADS_CASES[10]], ids=[HEADS_IDS[7], HEADS_IDS[10]])
def test_heads_precisions_differ(case):
    N, H, W, w_rows, band_list = case
    a, b = _heads(N, H, W, w_rows, "bf16x3", band_list[0]), _heads(N, H, W, w_rows, "fp32")
    assert not torch.equal(a["color"], b["color"]) and not torch.equal(a["mask"], b["mask"]), "the bf16x3 route did not run"


@pytest.mark.parametrize("case", [helpers.HEADS_CASES[4], helpers.HEADS_CASES[10]], ids=[HEADS_IDS[4], HEADS_IDS[10]])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_heads_every_output_subset_and_background_broadcast(precision, case):
    """pred only, mask only, any subset: the bits of the full call.  One background for the batch (bg_bs 1) or the same one
    repeated per image (bg_bs N): the same bits."""
    N, H, W, w_rows, band_list = case
    bands = band_list[0] if precision == "bf16x3" else 0
    full = _heads(N, H, W, w_rows, precision, bands)
    names = ("color", "mask", "pred")
    for r in (1, 2):
        for subset in itertools.combinations(names, r):
            out = _heads(N, H, W, w_rows, precision, bands, subset)
            assert sorted(out) == sorted(subset)
            assert all(torch.equal(out[k], full[k]) for k in subset), subset
    one, rep = _heads(N, H, W, w_rows, precision, bands, names, 1), _heads(N, H, W, w_rows, precision, bands, names, "repeat")
    assert all(torch.equal(one[k], rep[k]) for k in names)
    assert torch.equal(one["color"], full["color"]) and torch.equal(one["pred"][0], full["pred"][0])
    assert not torch.equal(one["pred"][1], full["pred"][1])   # image 1 was blended with image 0's background


@pytest.mark.parametrize("case", [helpers.HEADS_CASES[2], helpers.HEADS_CASES[10], helpers.HEADS_CASES[11]],
                         ids=[HEADS_IDS[2], HEADS_IDS[10], HEADS_IDS[11]])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_heads_image_alone_equals_image_in_batch(precision, case):
    """Also across the banding: alone, the launcher gives an image more bands than inside the batch."""
    N, H, W, w_rows, band_list = case
    batch = _heads(N, H, W, w_rows, precision, band_list[0] if precision == "bf16x3" else 0)
    for i in range(N):
        alone = _heads(N, H, W, w_rows, precision, 0, image=i)
        assert all(torch.equal(alone[k][0], batch[k][i]) for k in batch), (precision, i)


@pytest.mark.parametrize("H,W", [(8, 27), (24, 64)])
def test_heads_forward_is_the_fp32_hook_behind_an_identity_norm(H, W):
    from impersonator_amd import ops
    g = torch.Generator().manual_seed(17)
    x = torch.rand(2, H, W, 64, generator=g).cuda()                      # post-ReLU input
    w = (torch.randn(4, 64, 7, 7, generator=g) * 0.03).cuda()
    ss = torch.tensor([1.0, 0.0]).repeat(2, 64, 1).contiguous().cuda()
    color, mask = ops.heads_forward(x, w)
    out = ops.heads_inference(x, ss, w, "fp32", None, ("color", "mask"))
    assert torch.equal(out["color"], color) and torch.equal(out["mask"], mask)
