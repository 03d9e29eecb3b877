"""Order-independent exactness of the bilinear sampling kernels: every consumer of csrc/sample.h::grid_taps with an op-level entry
-- grid_sample_nchw_kernel (warp.hip), grid_sample_nhwc_kernel and the atomic grid_sample_bwd_kernel (train.hip), the plan and the
gather of scatter.hip -- and resize_flow_kernel, against float64 torch, bit for bit.

Pixel coordinates on a 1/8-texel lattice (weights are multiples of 1/64) and integer data in [-8, 8] (tests/helpers.py): every
product is exact and every sum is exact in any order, so the float64 result rounded to fp32 is the specification for the forward
kernels, the atomic scatter and the planned gather alike.  tests/test_sampling_cases.py proves without a device that the cases meet
these conditions, that a wrong unnormalise, floor, validity rule, pitch or batch rule cannot meet the equality, and the structural
facts used below (which list lengths occur, how many texels are queued, that -2 and -3 sample nothing).

(a) lattice cases: both align modes, shared and per-image sources, sources 8x16, 16x4, 1x2 / 5x9, 17x3, 2x2, coordinates over
    [-2, W + 1] x [-2, H + 1];
(b) named coordinates: ix in {-1.5, -1, -0.5, -0.125, 0, W-1, W-0.875, W-0.5, W} against every such iy, then NaN, +-inf, +-1e30, +-3e38
    in x, in y and in both -- exact zeros forward, nothing backward (the clamps of sample.h);
(c) contribution lists of 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097 entries in one plan (per-thread sort, each
    bitonic padding size, the dense scan), on exact data and on data whose fp32 sum depends on the order: the gather must give the
    numpy float32 running sum in ascending pixel index, i.e. walk the list in key order;
(d) 2143 queued texels: every workgroup of gs_plan_heavy_kernel's 1024 takes at least two texels in turn, sorted lists and the four
    dense-scanned ones of a 6400-pixel patch aimed at one point among them;
(e) a plan built into a dirty buffer, and again into the same buffer for another grid, equals a fresh plan;
(f) resize_flow_kernel on a dyadic rectangular flow, magnifying, minifying, identity and down to 1 x 1.
No tolerance anywhere in this file."""
import functools

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

CASES = helpers.SAMPLE_CASES
LATTICE = sorted(name for name, case in CASES.items() if case.kind == "lattice")
NAMED = ["named align 0", "named align 1"]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _reference(name, C):
    """(x, dy, grid, wild pixels, float64 forward and input gradient rounded to fp32) on the CPU; read-only.  The reference sees
    the grid with its wild entries replaced by -3."""
    case = CASES[name]
    grid = helpers.sample_grid(case)
    tame, wild = helpers.sample_tame(grid)
    x, dy = helpers.sample_data(case, C)
    y, dx = helpers.grid_sample_float64(x, tame, case.align, dy)
    return x, dy, grid, wild, y.float(), dx.float()


def _grid_sample_nchw(x, grid, align):
    from impersonator_amd import _lib
    xn, c, h, w = x.shape
    n, ho, wo, _ = grid.shape
    out = torch.empty((n, c, ho, wo), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().lwg_grid_sample(_lib.ptr(x), xn, c, h, w, _lib.ptr(grid), n, ho, wo, int(align), _lib.ptr(out),
                                           _lib.stream_ptr()))
    return out


def _check_nhwc(name, C):
    """forward, atomic gradient, planned gradient with a plan of its own and with a shared one: all equal float64"""
    from impersonator_amd import ops
    case = CASES[name]
    x, dy, grid, wild, y_ref, dx_ref = _reference(name, C)
    xg, dyg, gg = _nhwc(x), _nhwc(dy), grid.cuda()
    shape = (case.xn, case.H, case.W, C)
    y = ops.grid_sample_nhwc(xg, gg, case.align)
    assert torch.equal(_nchw(y), y_ref), "forward"
    atomic = ops.grid_sample_backward(dyg, gg, shape, case.align, deterministic=False)
    assert torch.equal(_nchw(atomic), dx_ref), "atomic gradient"
    own = ops.grid_sample_backward(dyg, gg, shape, case.align)
    assert torch.equal(_nchw(own), dx_ref), "planned gradient"
    plan = ops.GridSamplePlan(gg, shape, case.align)
    for scale in (1.0, -2.0):   # one plan, two tensors
        shared = ops.grid_sample_backward(dyg * scale, gg, shape, case.align, plan=plan)
        assert torch.equal(_nchw(shared), dx_ref * scale), "shared plan, dy * %g" % scale
    return y, wild


@pytest.mark.parametrize("C", [4, 12, 64])
@pytest.mark.parametrize("name", LATTICE)
def test_lattice_nhwc_forward_and_gradients_equal_float64(name, C):
    _check_nhwc(name, C)


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("name", LATTICE)
def test_lattice_nchw_forward_equals_float64(name, C):
    x, _, grid, _, y_ref, _ = _reference(name, C)
    assert torch.equal(_grid_sample_nchw(x.cuda(), grid.cuda(), CASES[name].align).cpu(), y_ref)


@pytest.mark.parametrize("name", NAMED)
def test_named_and_wild_coordinates(name):
    y, wild = _check_nhwc(name, 4)
    assert int(wild.sum()) == 2 * 63
    y = y.cpu()
    assert bool(torch.isfinite(y).all()) and float(y[wild].abs().max()) == 0.0     # exact zeros at the wild pixels
    x, _, grid, _, y_ref, _ = _reference(name, 3)
    y3 = _grid_sample_nchw(x.cuda(), grid.cuda(), CASES[name].align).cpu()
    assert torch.equal(y3, y_ref) and float(y3.permute(0, 2, 3, 1)[wild].abs().max()) == 0.0


def test_list_lengths_on_every_threshold_exact_family():
    _check_nhwc("thresholds exact", 4)


@pytest.mark.parametrize("name", ["thresholds ordered", "thresholds ordered n3"])
def test_the_gather_walks_each_list_in_key_order(name):
    """weights 1, 0, 0, 0 and dy = normal * 2^k: the aimed texel's gradient is the fp32 running sum of its pixels' dy in ascending
    pixel index (image-major for a shared source), its three zero-weight neighbours get 0; three plans, one result"""
    from impersonator_amd import ops
    case = CASES[name]
    grid, dy = helpers.sample_grid(case), helpers.sample_ordered_dy(case)
    taps = helpers.sample_taps(grid, case.H, case.W, case.align, case.xn)
    T, C = case.H * case.W, dy.shape[1]
    ref = helpers.ordered_running_sums(dy, helpers.sample_threshold_lists(case, taps), T)
    dyg, gg, shape = _nhwc(dy), grid.cuda(), (1, case.H, case.W, C)
    runs = [ops.grid_sample_backward(dyg, gg, shape, case.align, plan=ops.GridSamplePlan(gg, shape, case.align)) for _ in range(3)]
    assert all(torch.equal(r, runs[0]) for r in runs[1:])
    got = runs[0].cpu().view(T, C)
    wrong = torch.nonzero((got != ref).any(1)).reshape(-1).tolist()
    assert not wrong, "texels %s (list lengths %s)" % (wrong, [int(taps.counts[t]) for t in wrong])


@pytest.mark.parametrize("C", [4, 12])
def test_more_queued_texels_than_workgroups(C):
    _check_nhwc("crowded", C)


def _plan_fields(buf, T, P):
    """the defined words of a plan (csrc/scatter.hip: count[T] fill[T] cursor heavy_count offset[T] heavy[HC] keys[4P] weights[4P])
    in a canonical form: where a list lives and the order of the heavy queue are left to the atomics, the lists are not"""
    w = buf.cpu()
    cap = 4 * P // 33 + 1
    count, fill, cursor, nheavy = w[:T], w[T:2 * T], int(w[2 * T]), int(w[2 * T + 1])
    offset, heavy = w[2 * T + 2:3 * T + 2].long(), w[3 * T + 2:3 * T + 2 + cap]
    keys, weights = w[3 * T + 2 + cap:3 * T + 2 + cap + 4 * P], w[3 * T + 2 + cap + 4 * P:3 * T + 2 + cap + 8 * P]
    total = int(count.sum())
    starts = torch.cumsum(count.long(), 0) - count.long()
    slot = torch.repeat_interleave(offset - starts, count.long()) + torch.arange(total)
    placed = sorted(zip(offset[count > 0].tolist(), count[count > 0].tolist()))
    assert all(a + c <= b for (a, c), (b, _) in zip(placed, placed[1:])) and (not placed or placed[-1][0] + placed[-1][1] <= cursor)
    return dict(count=count.clone(), fill=fill.clone(), cursor=cursor, heavy=sorted(heavy[:nheavy].tolist()), keys=keys[slot].clone(),
                weights=weights[slot].clone())


def test_a_plan_built_into_a_dirty_buffer_equals_a_fresh_plan():
    """lwg_grid_sample_plan on a buffer full of 0x5A bytes, then on the same buffer for another grid of the same dimensions: each
    time the counts, the cursor, the queue, every list and every weight are those of a fresh ops.GridSamplePlan, bit for bit; the
    words behind the plan are untouched; and the gradient gathered over the reused buffer is the float64 one"""
    from impersonator_amd import _lib, ops
    lib = _lib.load()
    first, second = "thresholds exact", "lattice align 0 8x16 one image 96x160"
    case = CASES[first]
    dims = (case.xn, case.H, case.W, case.n, case.Ho, case.Wo)
    assert dims == tuple(getattr(CASES[second], k) for k in ("xn", "H", "W", "n", "Ho", "Wo")) and not CASES[second].align
    T, P = case.xn * case.H * case.W, case.n * case.Ho * case.Wo
    nbytes = lib.lwg_grid_sample_plan_bytes(*dims)
    assert nbytes == 4 * (3 * T + 2 + 4 * P // 33 + 1 + 8 * P)
    guard = 64
    buf = torch.full((nbytes // 4 + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for name in (first, second):
        _, dy, grid, _, _, dx_ref = _reference(name, 4)
        gg, dyg = grid.cuda(), _nhwc(dy)
        _lib.check(lib.lwg_grid_sample_plan(_lib.ptr(gg), *dims, 0, _lib.ptr(buf), nbytes, _lib.stream_ptr()))
        fresh = ops.GridSamplePlan(gg, (case.xn, case.H, case.W, 4), False)
        assert fresh.nbytes == nbytes
        mine, theirs = _plan_fields(buf, T, P), _plan_fields(fresh.buf, T, P)
        for key in mine:
            same = torch.equal(mine[key], theirs[key]) if torch.is_tensor(mine[key]) else mine[key] == theirs[key]
            assert same, "%s: %s" % (name, key)
        taps = helpers.sample_taps(helpers.sample_tame(grid)[0], case.H, case.W, False, case.xn)
        assert torch.equal(mine["count"].long(), taps.counts) and torch.equal(mine["fill"], mine["count"])
        assert mine["cursor"] == int(taps.counts.sum()) and mine["heavy"] == torch.nonzero(taps.counts > 32).reshape(-1).tolist()
        assert bool((buf[nbytes // 4:] == 0x5A5A5A5A).all())
        dx = torch.zeros(case.xn, case.H, case.W, 4, device="cuda")
        _lib.check(lib.lwg_grid_sample_backward_planned(_lib.ptr(dyg), 4, *dims, _lib.ptr(buf), nbytes, _lib.ptr(dx), _lib.stream_ptr()))
        assert torch.equal(_nchw(dx), dx_ref), name


@pytest.mark.parametrize("h,w", helpers.SAMPLE_FLOW_SIZES)
def test_resize_flow_equals_float64_interpolate(h, w):
    from impersonator_amd import _lib
    T = helpers.sample_flow()
    bs, H, W, _ = T.shape
    Tg = T.cuda()
    out = torch.empty((bs, h, w, 2), device="cuda", dtype=torch.float32)
    _lib.check(_lib.load().lwg_resize_flow(_lib.ptr(Tg), bs, H, W, h, w, _lib.ptr(out), _lib.stream_ptr()))
    assert torch.equal(out.cpu(), helpers.resize_flow_float64(T, h, w).float())
