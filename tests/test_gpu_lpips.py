"""GPU: the LPIPS kernels (csrc/lpips.hip) against torch in fp64, op by op at the smallest shapes that exercise the tails, then
the whole model against the golden fp64 values of the live reference, the bit-for-bit properties (identity, batch position, swap,
graph replay, weight reload), and the evaluator's surface (utils/metrics.py).

Error bounds, none of them measured.
  conv: an output is an fp32 fmaf chain over K products plus the bias; against the exact value of the same fp32 operands its error
    is at most (K + 8) * 2^-24 * S, S = the same expression on absolute values (as tests/test_gpu_hmr.py).  With the prologue the
    operands are the mapped and scaled pixels, restated in numpy float32 step by step (correctly rounded, so the same bits).
  max pool: exact.
  layer distance: tests/lpips_ref.layer_distance_bound, derived there; the exact value is taken in extended precision.
  whole model: the rule of the golden tests -- relative error at most 4 x the reference's own fp32 error against fp64, worst over
    the golden's cases as recorded in the file (the factor 4 is headroom for another summation order).  Each quantity is held to
    the figure of that quantity, as features and theta are in tests/test_gpu_hmr.py: the distances to ref_fp32_rel_err (9.4e-7),
    the per-layer terms to ref_fp32_rel_err_taps (5.3e-6; a single layer's term lacks the averaging of the five-term sum, in the
    reference's arithmetic as on the device).
Every test prints the figures it compares before it asserts (run with -s); DESIGN.md section 3.10 keeps the observed ratios."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from impersonator_amd import _lib
from impersonator_amd.networks import lpips as lpips_net
from impersonator_amd.utils import metrics, synthetic
from tests import lpips_ref
from tests import metrics_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def _scaled(x, mode):
    """the prologue in numpy float32: the evaluator's pixel mode, then (x - shift) / scale, one rounding per step"""
    v = metrics_ref.map_pixels(x, mode)
    shift = np.asarray(lpips_ref.SHIFT, np.float32).reshape(1, 3, 1, 1)
    scale = np.asarray(lpips_ref.SCALE, np.float32).reshape(1, 3, 1, 1)
    return ((v - shift) / scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ conv, op level
def _conv_case(seed, N, H, W, Cin, Cout, k, stride, pad, mode=-1, relu=1, x=None):
    """Runs lwg_lpips_conv and the fp64 statement of the same thing; asserts the worst-case fp32 bound element by element.
    mode >= 0: x is (N,3,H,W) NCHW frames and the prologue applies; mode < 0: NHWC features as they are."""
    rs = np.random.RandomState(seed)
    if x is None:
        lo = 0.0 if mode == 1 else -1.0
        x = rs.uniform(lo, 1.0, (N, Cin, H, W)).astype(np.float32) if mode >= 0 else rs.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = torch.from_numpy((rs.standard_normal((Cout, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k))).astype(np.float32))
    b = torch.from_numpy(rs.normal(0, 0.2, Cout).astype(np.float32))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xa = torch.from_numpy(_scaled(x, mode) if mode >= 0 else x).double()
    want = F.conv2d(xa, w.double(), b.double(), stride=stride, padding=pad)
    if relu:
        want = F.relu(want)
    mag = F.conv2d(xa.abs(), w.double().abs(), b.double().abs(), stride=stride, padding=pad)
    bound = (k * k * Cin + 8) * U * mag + 1e-30

    lib = _lib.load()
    xd = _dev(x) if mode >= 0 else _nhwc(torch.from_numpy(x))
    wd, bd = w.permute(2, 3, 1, 0).contiguous().cuda(), b.cuda()
    y = torch.full((N, Ho, Wo, Cout), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")          # allocated right after y: an overrun of y would land here
    _lib.check(lib.lwg_lpips_conv(_lib.ptr(xd), N, H, W, Cin, _lib.ptr(wd), _lib.ptr(bd), Cout, k, stride, pad, relu, mode,
                                  _lib.ptr(y), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = y.permute(0, 3, 1, 2).double().cpu()
    assert bool(torch.isfinite(got).all()) and bool((guard == 7.0).all())
    ratio = float(((got - want).abs() / bound).max())
    print("conv k%d s%d mode %d N%d %dx%d %d->%d (M = %d, K = %d): max |err| %.3g, worst err / bound %.3g" % (
        k, stride, mode, N, H, W, Cin, Cout, N * Ho * Wo, k * k * Cin, float((got - want).abs().max()), ratio))
    assert ratio <= 1.0
    return got, want


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv11_stride4_with_the_prologue_under_two_tiles(mode):
    x = None
    if mode == 2:
        # values on the quantiser's steps, the two ends, and values outside [-1,1] that the clamp catches
        x = np.random.RandomState(20).uniform(-1, 1, (2, 3, 31, 31)).astype(np.float32)
        steps = ((np.arange(31, dtype=np.float32) * 8 / np.float32(255)) * np.float32(2)) - np.float32(1)
        x[0, 0, 0, :], x[0, 1, 1, :4], x[1, 2, 30, 27:] = steps, [-1.0, 1.0, 1.25, -1.5], [1.0, -1.0, 0.0, 1e-3]
    _conv_case(10 + mode, N=2, H=31, W=31, Cin=3, Cout=64, k=11, stride=4, pad=2, mode=mode, x=x)        # 7x7: M = 98


def test_conv11_stride4_odd_size_with_columns_no_window_reaches():
    _conv_case(14, N=1, H=35, W=47, Cin=3, Cout=64, k=11, stride=4, pad=2)                       # NHWC, Cin = 3: 8x11
    _conv_case(15, N=1, H=35, W=47, Cin=3, Cout=64, k=11, stride=4, pad=2, mode=0)               # the same geometry from frames


def test_conv11_padding_applies_after_the_scaling():
    """frames of zeros: every scaled value is (0 - shift) / scale != 0, so a padded tap that wrongly went through the scaling would
    make the border outputs equal the interior's"""
    x = np.zeros((1, 3, 31, 31), np.float32)
    got, want = _conv_case(16, N=1, H=31, W=31, Cin=3, Cout=64, k=11, stride=4, pad=2, mode=0, relu=0, x=x)
    interior, corner = want[0, :, 3, 3], want[0, :, 0, 0]
    print("constant input: interior vs corner outputs differ by up to %.3g" % float((interior - corner).abs().max()))
    assert float((interior - corner).abs().max()) > 1e-2                      # the case does tell the two apart
    assert float((got[0, :, 3, 3] - got[0, :, 2, 4]).abs().max()) < 1e-5      # and interior pixels agree among themselves


def test_conv5_every_pixel_at_a_border_three_column_tiles():
    _conv_case(17, N=2, H=7, W=7, Cin=64, Cout=192, k=5, stride=1, pad=2)                        # K = 1600


def test_conv3_long_k_under_one_tile():
    _conv_case(18, N=3, H=3, W=3, Cin=192, Cout=384, k=3, stride=1, pad=1)                       # M = 27
    _conv_case(19, N=3, H=3, W=3, Cin=384, Cout=256, k=3, stride=1, pad=1)                       # K = 3456, the longest


# ------------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize("c", [64, 192])
@pytest.mark.parametrize("h,w", [(7, 7), (8, 8), (15, 9)])
def test_maxpool_is_floor_mode(h, w, c):
    rs = np.random.RandomState(h * 100 + w + c)
    x = torch.from_numpy(-rs.uniform(0.5, 3.0, (2, c, h, w)).astype(np.float32))      # all negative: a zero tap would win
    want = F.max_pool2d(x.double(), kernel_size=3, stride=2)
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    assert tuple(want.shape[-2:]) == (ho, wo)
    y = torch.full((2, ho, wo, c), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")
    xd = _nhwc(x)
    _lib.check(_lib.load().lwg_lpips_maxpool(_lib.ptr(xd), 2, h, w, c, _lib.ptr(y), _lib.stream_ptr()))
    got = y.permute(0, 3, 1, 2).double().cpu()
    assert torch.equal(got, want) and float(got.max()) < 0 and bool((guard == 7.0).all())


# ------------------------------------------------------------------------------------------------ layer distance, op level
def _distance(f0, f1, w):
    n, P, C = f0.shape
    a, b, wd = _dev(f0), _dev(f1), _dev(w)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    guard = torch.full((512,), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().lwg_lpips_layer_distance(_lib.ptr(a), _lib.ptr(b), n, P, C, _lib.ptr(wd), _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    return out.cpu().numpy()


@pytest.mark.parametrize("P,C", [(1, 256), (9, 384), (49, 64)])
def test_layer_distance_against_the_derived_bound(P, C):
    rs = np.random.RandomState(P * 1000 + C)
    f0 = np.maximum(rs.standard_normal((3, P, C)), 0).astype(np.float32)      # independent blocks, as after a ReLU: no cancellation
    f1 = np.maximum(rs.standard_normal((3, P, C)), 0).astype(np.float32)
    w = (rs.uniform(0, 2, C) / C).astype(np.float32)
    f0[1, 0] = 0                                                               # a pixel all zero in one half ...
    f0[2, P - 1] = f1[2, P - 1] = 0                                            # ... and one all zero in both
    got = _distance(f0, f1, w)
    value, bound = lpips_ref.layer_distance_bound(f0, f1, w)
    err = np.abs(got.astype(np.longdouble) - value).astype(np.float64)
    print("layer distance P=%d C=%d: values %s, |err| %s, bound %s, worst err / bound %.3g" % (
        P, C, got, err, bound, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.isfinite(got).all() and (err <= bound).all()
    if P == 1:
        assert got[2] == 0.0                                                   # 0 / 1e-10 = 0 on both sides
        assert abs(got[1] - float((w.astype(np.float64) * (f1[1, 0].astype(np.float64) ** 2)).sum()
                                  / (np.sqrt((f1[1, 0].astype(np.float64) ** 2).sum()) + 1e-10) ** 2)) <= 1e-12
    # identical halves: exactly 0; swapped halves: the same bits
    assert np.array_equal(_distance(f0, f0.copy(), w), np.zeros(3))
    assert np.array_equal(_distance(f1, f0, w), got)


# ------------------------------------------------------------------------------------------------ whole model
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "lpips_golden.npz"))


def _state_dicts(gold, seed=None):
    alex, lin = synthetic.lpips_state_dicts(int(gold["seed"]) if seed is None else seed)
    if seed is None:
        lin = {"lin%d.model.1.weight" % j: gold["lin%d" % j].reshape(1, -1, 1, 1) for j in range(5)}   # the reference's alex.pth
    return alex, lin


@pytest.fixture(scope="module")
def model(gold):
    m = lpips_net.LPIPS(*_state_dicts(gold), max_batch=8, image_size=256)
    yield m
    m.release()


def _run(model, pred, ref, mode=0):
    taps = torch.full((pred.shape[0], 5), float("nan"), dtype=torch.float64, device="cuda")
    dist = model(pred, ref, mode=mode, taps=taps)
    return dist, taps


def test_whole_model_against_the_golden_fp64_values(model, gold):
    yard, yard_taps = float(gold["ref_fp32_rel_err"]), float(gold["ref_fp32_rel_err_taps"])
    worst_d = worst_t = 0.0
    for index, case in enumerate(lpips_ref.CASES):
        for kind in ("noise", "near"):
            pred, ref = lpips_ref.case_inputs(index, kind)
            dist, taps = _run(model, _dev(pred), _dev(ref))
            key = "%s_%s" % (case[0], kind)
            d64, t64 = gold[key + "_dist_fp64"], gold[key + "_taps_fp64"]
            ed = float((np.abs(dist.cpu().numpy() - d64) / d64).max())
            et = float((np.abs(taps.cpu().numpy() - t64) / t64).max())
            er = float((np.abs(gold[key + "_dist_fp32"] - d64) / d64).max())
            print("%-8s %-5s dist %s: device rel err %.3g (reference fp32 %.3g), taps %.3g" % (case[0], kind, dist.cpu().numpy(), ed, er, et))
            worst_d, worst_t = max(worst_d, ed), max(worst_t, et)
    print("whole model: worst device rel err dist %.3g = %.3g x ref_fp32_rel_err (%.3g); taps %.3g = %.3g x ref_fp32_rel_err_taps "
          "(%.3g)" % (worst_d, worst_d / yard, yard, worst_t, worst_t / yard_taps, yard_taps))
    assert worst_d <= 4 * yard
    assert worst_t <= 4 * yard_taps


@pytest.fixture(scope="module")
def pairs():
    """five 64x64 pairs: noise against noise, and smooth images against noisy copies"""
    rs = np.random.RandomState(77)
    a = np.concatenate([rs.uniform(-1, 1, (3, 3, 64, 64)).astype(np.float32), synthetic.smooth_image(78, (2, 3, 64, 64))])
    b = np.concatenate([rs.uniform(-1, 1, (3, 3, 64, 64)).astype(np.float32),
                        np.clip(a[3:] + 0.1 * rs.uniform(-1, 1, (2, 3, 64, 64)), -1, 1).astype(np.float32)])
    return _dev(a), _dev(b)


def test_identical_images_give_exactly_zero(model, pairs):
    a, _ = pairs
    dist, taps = _run(model, a, a)
    assert bool((dist == 0).all()) and bool((taps == 0).all())
    dist, taps = _run(model, a, a.clone())
    assert bool((dist == 0).all()) and bool((taps == 0).all())


def test_batch_position_repeat_and_swap_bit_for_bit(model, pairs):
    a, b = pairs
    five_d, five_t = _run(model, a, b)
    again_d, again_t = _run(model, a, b)
    assert torch.equal(five_d, again_d) and torch.equal(five_t, again_t)
    assert bool((five_d > 0).all()) and bool(torch.isfinite(five_t).all())
    assert torch.equal(five_d, ((((five_t[:, 0] + five_t[:, 1]) + five_t[:, 2]) + five_t[:, 3]) + five_t[:, 4]))   # taps in tap order
    for i in range(5):
        d, t = _run(model, a[i:i + 1], b[i:i + 1])
        assert torch.equal(d[0], five_d[i]) and torch.equal(t[0], five_t[i]), i
    swap_d, swap_t = _run(model, b, a)
    assert torch.equal(swap_d, five_d) and torch.equal(swap_t, five_t)


def test_the_op_level_entries_make_the_handles_bits(model, gold, pairs):
    """first layer by hand: lwg_lpips_conv on the 2n frames, lwg_lpips_layer_distance (one workgroup per frame walking the four
    chunks of the 15x15 map) == the forward's first per-layer term (one workgroup per chunk, added by the finalize kernel)"""
    a, b = pairs
    n = a.shape[0]
    alex, lin = _state_dicts(gold)
    w = _dev(alex["features.0.weight"].transpose(2, 3, 1, 0))
    bias, lin0 = _dev(alex["features.0.bias"]), _dev(lin["lin0.model.1.weight"].reshape(-1))
    x = torch.cat([a, b]).contiguous()
    y = torch.full((2 * n, 15, 15, 64), float("nan"), device="cuda")
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    lib = _lib.load()
    _lib.check(lib.lwg_lpips_conv(_lib.ptr(x), 2 * n, 64, 64, 3, _lib.ptr(w), _lib.ptr(bias), 64, 11, 4, 2, 1, 0, _lib.ptr(y), _lib.stream_ptr()))
    _lib.check(lib.lwg_lpips_layer_distance(_lib.ptr(y[:n]), _lib.ptr(y[n:]), n, 225, 64, _lib.ptr(lin0), _lib.ptr(out), _lib.stream_ptr()))
    _, taps = _run(model, a, b)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, taps[:, 0])


def test_chunked_batches_equal_the_whole(model, gold, pairs):
    a, b = pairs
    small = lpips_net.LPIPS(*_state_dicts(gold), max_batch=2, image_size=64)
    try:
        d, t = _run(small, a, b)                                               # chunks of 2, 2, 1
        want_d, want_t = _run(model, a, b)
        assert torch.equal(d, want_d) and torch.equal(t, want_t)
    finally:
        small.release()


def test_a_forward_replays_as_a_graph_on_new_inputs(model, pairs):
    a, b = pairs
    eager = [_run(model, a[s:s + 2], b[s:s + 2]) for s in (0, 2)]
    sa, sb = a[:2].clone(), b[:2].clone()
    dist = torch.zeros((2,), dtype=torch.float64, device="cuda")
    taps = torch.zeros((2, 5), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        model(sa, sb, out=dist, taps=taps)
    for s, (want_d, want_t) in zip((0, 2), eager):
        sa.copy_(a[s:s + 2])
        sb.copy_(b[s:s + 2])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dist, want_d) and torch.equal(taps, want_t), s


def test_set_weights_of_a_second_seed_and_back(model, gold, pairs):
    a, b = pairs
    before, _ = _run(model, a, b)
    handle = model._ensure_handle().value
    try:
        model.load_state_dicts(*_state_dicts(gold, seed=1))
        other, _ = _run(model, a, b)
        assert model._handle.value == handle
        rel = float(((other - before).abs() / before).min())
        print("second seed: distances change by at least %.3g relative" % rel)
        assert rel > 1e-3
    finally:
        model.load_state_dicts(*_state_dicts(gold))
    assert torch.equal(_run(model, a, b)[0], before)


def test_forward_refuses_what_the_handle_is_not_built_for(model):
    h = model._ensure_handle()
    lib = _lib.load()
    buf = torch.zeros(3 * 64 * 64, device="cuda")
    out = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    fwd = lambda n=1, hh=64, ww=64, mode=0, handle=h: lib.lwg_lpips_forward(handle, _lib.ptr(buf), _lib.ptr(buf), n, hh, ww, mode,
                                                                           _lib.ptr(out), None, _lib.stream_ptr())
    assert fwd(hh=30) == -2 and b"relu5" in lib.lwg_last_error()
    assert fwd(ww=30) == -2
    assert fwd(n=9) == -5 and b"max_pairs" in lib.lwg_last_error()
    assert fwd(hh=257) == -5 and fwd(ww=300) == -5
    assert fwd(mode=3) == -1 and fwd(mode=-1) == -1
    assert lib.lwg_lpips_weight_floats(h) == 2468544 + 1152 + 1152
    fresh = ctypes.c_void_p()
    _lib.check(lib.lwg_lpips_create(ctypes.byref(fresh), 1, 64, 64))
    try:
        assert fwd(handle=fresh) == -5 and b"weights" in lib.lwg_last_error()                      # no weights
        assert lib.lwg_lpips_set_weights(fresh, ctypes.c_void_p(buf.cpu().data_ptr()), 16) == -1
    finally:
        lib.lwg_lpips_destroy(fresh)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                            # refused before anything was launched
    with pytest.raises(_lib.LwgError) as e:
        model(torch.zeros((1, 3, 30, 40), device="cuda"), torch.zeros((1, 3, 30, 40), device="cuda"))
    assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ the evaluator's surface
def test_paired_evaluator_ragged_updates_modes_and_the_metric_class(model):
    rs = np.random.RandomState(91)
    a, b = rs.uniform(-1, 1, (9, 3, 40, 36)).astype(np.float32), rs.uniform(-1, 1, (9, 3, 40, 36)).astype(np.float32)
    da, db = _dev(a), _dev(b)
    ev = metrics.PairedEvaluator(("ssim", "psnr", "lpips"), lpips=model)
    for s, e in ((0, 4), (4, 8), (8, 9)):
        ev.update(da[s:e], db[s:e])
    out = ev.result()
    single = torch.cat([model(da[i:i + 1], db[i:i + 1]) for i in range(9)]).cpu().numpy()
    stats = torch.cat([metrics.pair_stats(da[i:i + 1], db[i:i + 1]) for i in range(9)]).cpu().numpy()
    assert out["frames"] == len(ev) == 9
    assert np.array_equal(out["per_frame"]["lpips"], single) and out["lpips"] == float(np.mean(single))
    assert np.array_equal(out["per_frame"]["ssim"], stats[:, 0]) and np.array_equal(out["per_frame"]["psnr"], metrics.psnr_from_stats(stats))
    # the table grows without losing rows
    many = metrics.PairedEvaluator(("lpips",), lpips=model)
    for _ in range(9):
        many.update(da, db)
    assert np.array_equal(many.result()["per_frame"]["lpips"], np.tile(single, 9))
    # mode 2 == quantising both images on the host and scoring in mode 0
    q = metrics.PairedEvaluator(("lpips",), lpips=model, mode=2)
    q.update(da, db)
    host = model(_dev(metrics_ref.map_pixels(a, 2)), _dev(metrics_ref.map_pixels(b, 2))).cpu().numpy()
    got = q.result()["per_frame"]["lpips"]
    print("mode 2: lpips %s; max |mode 2 - host quantised| %.3g; mode 0 differs by %.3g" % (
        got[:3], float(np.abs(got - host).max()), float(np.abs(single - host).max())))
    assert np.array_equal(got, host) and not np.array_equal(single, host)
    # the reference's class takes [0,1] images: mode 1
    ua, ub = (a + 1) / 2, (b + 1) / 2
    score = metrics.PerceptualMetric(model).calculate_score(_dev(ua), _dev(ub))
    unit = model(_dev(ua), _dev(ub), mode=1).cpu().numpy()
    mapped = model(_dev(metrics_ref.map_pixels(ua, 1)), _dev(metrics_ref.map_pixels(ub, 1))).cpu().numpy()
    assert score == float(np.mean(unit)) and np.array_equal(unit, mapped)
    assert metrics.PerceptualMetric(model).quality() == "lower"
    with pytest.raises(ValueError):
        metrics.PairedEvaluator(("lpips",))
