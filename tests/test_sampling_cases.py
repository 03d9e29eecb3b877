"""The cases of tests/test_gpu_sampling_exact.py are honest: without a device, in float64.

For every case of helpers.SAMPLE_CASES the grid and the data are rebuilt from their seed and
1. meet the conditions under which bit equality with the float64 result IS the specification: the grid, the data and the float64
   reference (forward and input gradient) are their own fp32 roundings, the data are integers in [-8, 8], every weight is a
   multiple of 1/64 in [0, 1], and 8 * 64 * (longest contribution list) < 2^24 -- every partial sum of an output, in any order,
   is then an fp32 number;
2. give F.grid_sample's float64 result, forward and gradient, bit for bit when restated from helpers.sample_taps;
3. give something else under every mutant of that restatement that the case's geometry can show (helpers.sample_case_mutants), and
   the same under those it cannot -- so the table of which case catches what is itself checked.
The structural conditions the GPU cases rest on (which list lengths occur, how many texels are queued, that the -2 sentinel and the
-3 that stands in for a wild coordinate sample nothing) are asserted here from the counts, not assumed on the device.  The 'ordered'
family leaves exactness on purpose: there the order of an fp32 sum is what is tested, and this file shows that another order gives
other bits."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import helpers

CASES = sorted(helpers.SAMPLE_CASES)
EXACT = CASES   # the geometry of the 'ordered' cases is held to the same statements on integer data; their own dy is tested below
C = 4


@functools.lru_cache(maxsize=None)
def _checked(name):
    """case, the grid the reference sees (wild entries tamed), data, taps and the float64 reference; read-only"""
    case = helpers.SAMPLE_CASES[name]
    grid, wild = helpers.sample_tame(helpers.sample_grid(case))
    x, dy = helpers.sample_data(case, C)
    taps = helpers.sample_taps(grid, case.H, case.W, case.align, case.xn)
    y, dx = helpers.grid_sample_float64(x, grid, case.align, dy)
    return case, grid, wild, x, dy, taps, y, dx


def _is_fp32(t):
    return torch.equal(t.float().double(), t.double())


@pytest.mark.parametrize("name", CASES)
def test_the_grid_is_exact_in_fp32_through_the_unnormalise(name):
    case, grid, _, _, _, taps, _, _ = _checked(name)
    assert tuple(grid.shape) == (case.n, case.Ho, case.Wo, 2) and grid.dtype == torch.float32
    # sample.h::unnormalize step by step in fp32 against float64
    for axis, size in ((0, case.W), (1, case.H)):
        g32, g64 = grid[..., axis], grid[..., axis].double()
        if case.align:
            steps32 = [g32 + 1, (g32 + 1) / 2, ((g32 + 1) / 2) * float(size - 1)]
            steps64 = [g64 + 1, (g64 + 1) / 2, ((g64 + 1) / 2) * (size - 1)]
            assert size - 1 >= 1 and (size - 1) & (size - 2) == 0
        else:
            steps32 = [g32 + 1, (g32 + 1) * float(size), (g32 + 1) * float(size) - 1, ((g32 + 1) * float(size) - 1) / 2]
            steps64 = [g64 + 1, (g64 + 1) * size, (g64 + 1) * size - 1, ((g64 + 1) * size - 1) / 2]
            assert size & (size - 1) == 0
        for a, b in zip(steps32, steps64):
            assert a.dtype == torch.float32 and torch.equal(a.double(), b)
        # ... and lands on the 1/8 lattice
        assert torch.equal((steps64[-1] * 8).round(), steps64[-1] * 8)
    assert torch.equal((taps.w * 64).round(), taps.w * 64) and float(taps.w.min()) >= 0 and float(taps.w.max()) <= 1
    if case.kind != "named":   # the coordinates the case was built from come back
        ix, iy, sentinel = helpers.sample_pixel_coordinates(case)
        back = ((grid.double() + 1) / 2 * torch.tensor([case.W - 1, case.H - 1]) if case.align
                else ((grid.double() + 1) * torch.tensor([case.W, case.H]) - 1) / 2)
        assert torch.equal(back[..., 0][~sentinel], ix[~sentinel]) and torch.equal(back[..., 1][~sentinel], iy[~sentinel])
        assert not bool(taps.valid[sentinel].any())


@pytest.mark.parametrize("name", EXACT)
def test_the_operands_make_bit_equality_the_specification(name):
    case, grid, _, x, dy, taps, y, dx = _checked(name)
    for t in (x, dy):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= 8
    longest = int(taps.counts.max())
    budget = 8 * 64 * longest
    print("OBSERVED %s: longest list %d, bit budget %.3g of 2^24" % (name, longest, budget))
    assert budget < 2 ** 24
    assert _is_fp32(y) and _is_fp32(dx) and float(y.abs().max()) > 0 and float(dx.abs().max()) > 0
    # torch's own fp32 evaluation agrees with float64 on such inputs
    xr = x.clone().requires_grad_(True)
    n = grid.shape[0]
    y32 = F.grid_sample(xr.expand(n, -1, -1, -1) if case.xn == 1 and n > 1 else xr, grid, mode="bilinear", padding_mode="zeros",
                        align_corners=case.align)
    y32.backward(dy)
    assert torch.equal(y32.detach().double(), y) and torch.equal(xr.grad.double(), dx)


@pytest.mark.parametrize("name", EXACT)
def test_the_bit_equality_has_teeth(name):
    case, grid, _, x, dy, _, y, dx = _checked(name)
    shape = tuple(x.shape)
    assert torch.equal(helpers.grid_sample_restated(x, grid, case.align), y)
    assert torch.equal(helpers.grid_sample_adjoint_restated(dy, grid, shape, case.align), dx)
    applicable = helpers.sample_case_mutants(case)
    for mutant in helpers.SAMPLE_MUTANTS:
        if mutant == "first_image_only":   # a statement about the gradient of a shared source
            if case.xn > 1 or case.n == 1:
                continue
            fwd = None
        else:
            fwd = float((helpers.grid_sample_restated(x, grid, case.align, mutant) != y).double().mean())
        grad = float((helpers.grid_sample_adjoint_restated(dy, grid, shape, case.align, mutant) != dx).double().mean())
        print("OBSERVED %s %s (%s): %s of the outputs, %.1f %% of the gradient change"
              % (name, mutant, "applicable" if mutant in applicable else "hidden by this geometry",
                 "-" if fwd is None else "%.1f %%" % (100 * fwd), 100 * grad))
        if mutant in applicable:
            assert grad > 0 and (fwd is None or fwd > 0), mutant
        else:
            assert grad == 0 and not fwd, mutant


def test_every_mutant_is_caught_by_some_lattice_case_of_each_mode_and_source_kind():
    for align in (False, True):
        for xn in (1, 3):
            caught = set()
            for case in helpers.SAMPLE_CASES.values():
                if case.kind == "lattice" and case.align == align and case.xn == xn:
                    caught.update(helpers.sample_case_mutants(case))
            assert caught == set(helpers.SAMPLE_MUTANTS) - ({"first_image_only"} if xn > 1 else set()), (align, xn, caught)


@pytest.mark.parametrize("name", ["named align 0", "named align 1"])
def test_the_named_cases_hold_the_named_coordinates_and_minus_three_samples_nothing(name):
    case, grid, wild, _, _, taps, y, _ = _checked(name)
    raw = helpers.sample_grid(case)
    assert case.H != case.W
    unn = (lambda g, s: (g + 1) / 2 * (s - 1)) if case.align else (lambda g, s: ((g + 1) * s - 1) / 2)
    ix, iy = unn(raw[0].double()[..., 0], case.W).reshape(-1)[:81], unn(raw[0].double()[..., 1], case.H).reshape(-1)[:81]
    pairs = {(float(a), float(b)) for a, b in zip(ix, iy)}
    assert pairs == {(a, b) for a in helpers.named_coordinates(case.W) for b in helpers.named_coordinates(case.H)}
    # 63 wild pixels per image: 7 in x only, 7 in y only, 49 in both; every wild value in each role
    assert wild.view(case.n, -1).sum(1).tolist() == [63, 63] and not bool(wild[0].reshape(-1)[:81].any())
    tail = raw[0].reshape(-1, 2)[81:]
    is_wild = ~torch.isfinite(tail) | (tail.abs() >= 1e30)
    assert (int((is_wild[:, 0] & ~is_wild[:, 1]).sum()), int((~is_wild[:, 0] & is_wild[:, 1]).sum()), int(is_wild.all(1).sum())) == (7, 7, 49)
    for axis in (0, 1):
        seen = tail[:, axis][is_wild[:, axis]]
        assert int(torch.isnan(seen).sum()) == 8      # once alone, seven times beside each wild value of the other axis
        assert {float(v) for v in seen[~torch.isnan(seen)]} == {float(torch.tensor(v)) for v in helpers.SAMPLE_WILD[1:]}
    # the coordinate that is not wild lies inside the image: only the wild one keeps such a pixel from sampling
    probe = torch.where(is_wild, torch.zeros_like(tail), tail).view(1, 1, -1, 2)
    inside = helpers.sample_taps(probe, case.H, case.W, case.align, 1).valid.view(-1, 4)
    assert bool(inside[:14].all())
    # -3 samples nothing, in x or in y, so the tamed grid is the reference of the wild one
    assert not bool(taps.valid[wild].any())
    assert float(y.permute(0, 2, 3, 1)[wild].abs().max()) == 0
    assert bool(taps.valid[~wild].any(-1).sum() > 0)
    assert torch.equal(torch.nan_to_num(raw[1], nan=7.0), torch.nan_to_num(raw[0].flip(0, 1), nan=7.0))   # image 1: reverse order


@pytest.mark.parametrize("name", ["thresholds exact", "thresholds ordered", "thresholds ordered n3"])
def test_the_threshold_cases_put_a_list_on_every_threshold(name):
    case, grid, _, _, _, taps, _, _ = _checked(name)
    assert sum(helpers.SAMPLE_THRESHOLDS) == 13347 and len(helpers.SAMPLE_BLOCKS) == 15
    counts = taps.counts.view(case.H, case.W)
    lists = helpers.sample_threshold_lists(case, taps)
    assert [K for K, _, _ in lists] == list(helpers.SAMPLE_THRESHOLDS)
    for K, tex, pixels in lists:
        ty, tx = divmod(tex, case.W)
        assert counts[ty:ty + 2, tx:tx + 2].tolist() == [[K, K], [K, K]]        # a zero-weight valid tap counts
        assert pixels.numel() == K and bool((pixels[1:] > pixels[:-1]).all())
    assert int(counts.sum()) == 4 * 13347 and set(counts.reshape(-1).tolist()) == set(helpers.SAMPLE_THRESHOLDS) | {0}
    assert int((grid[..., 0] == -2).sum()) == case.n * case.Ho * case.Wo - 13347
    w = taps.w[taps.valid.all(-1)]
    if case.kind == "thresholds_ordered":
        assert torch.equal(w, torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).expand_as(w))
        if case.n > 1:   # a list crosses images: key order is image-major
            images = {int(p) // (case.Ho * case.Wo) for p in lists[-1][2]}
            assert images == set(range(case.n))
    else:
        assert float(w.min()) > 0


@pytest.mark.parametrize("name", ["thresholds ordered", "thresholds ordered n3"])
def test_the_ordered_family_depends_on_the_order(name):
    case, _, _, _, _, taps, _, _ = _checked(name)
    dy = helpers.sample_ordered_dy(case)
    lists = helpers.sample_threshold_lists(case, taps)
    T = case.H * case.W
    ref, rev = helpers.ordered_running_sums(dy, lists, T), helpers.ordered_running_sums(dy, lists, T, reverse=True)
    aimed = [tex for K, tex, _ in lists if K > 2]
    changed = float((ref[aimed] != rev[aimed]).double().mean())
    print("OBSERVED %s: %.1f %% of the sums of more than two terms change when the list is walked backwards" % (name, 100 * changed))
    assert changed > 0.5
    exact = helpers.grid_sample_float64(torch.zeros(1, dy.shape[1], case.H, case.W), helpers.sample_grid(case), case.align, dy)[1]
    assert not torch.equal(ref.view(case.H, case.W, -1).permute(2, 0, 1)[None].double(), exact.float().double())
    rest = torch.ones(T, dtype=torch.bool)
    rest[[tex for _, tex, _ in lists]] = False
    assert float(ref[rest].abs().max()) == 0


def test_the_crowded_case_queues_every_workgroup_twice():
    case, _, _, _, _, taps, _, _ = _checked("crowded")
    counts = taps.counts
    queued, dense, longest = int((counts > 32).sum()), int((counts > 4096).sum()), int(counts.max())
    print("OBSERVED crowded: %d of %d texels over 32 contributions, %d lists over 4096, longest %d, bit budget %.3g"
          % (queued, counts.numel(), dense, longest, 8 * 64 * longest))
    assert queued > 2048            # gs_plan_heavy_kernel runs 1024 workgroups: each takes at least two texels
    assert dense >= 1 and int(((counts > 32) & (counts <= 4096)).sum()) >= 1
    # the dense-scanned lists belong to the four taps of the aimed point, which lies inside the image
    ix, iy = helpers.SAMPLE_POINT
    point = [int(iy) * case.W + int(ix) + d for d in (0, 1, case.W, case.W + 1)]
    assert sorted(torch.nonzero(counts > 4096).reshape(-1).tolist()) == point


def test_the_flow_resize_cases_are_exact():
    T = helpers.sample_flow()
    assert tuple(T.shape) == (2, 33, 17, 2) and torch.equal((T * 64).round(), T * 64)
    assert float(T.min()) == -2 and float(T.max()) <= 1 and int((T == -2).all(-1).sum()) >= 42
    for h, w in helpers.SAMPLE_FLOW_SIZES:
        for full, out in ((32, h), (16, w)):
            scale = full / (out - 1) if out > 1 else 0.0
            assert scale == 0 or (scale * 64 == int(scale * 64) and int(scale * 64) & (int(scale * 64) - 1) == 0)
        ref = helpers.resize_flow_float64(T, h, w)
        assert tuple(ref.shape) == (2, h, w, 2) and _is_fp32(ref)
        r32 = F.interpolate(T.permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        assert torch.equal(r32.double(), ref)
        # teeth: a source read with H and W exchanged gives something else
        if (h, w) != (1, 1):
            assert not torch.equal(helpers.resize_flow_float64(T.reshape(2, 17, 33, 2), h, w), ref)
