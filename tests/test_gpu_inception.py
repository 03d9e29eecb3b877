"""GPU: the InceptionV3 kernels (csrc/inception.hip) against torch in fp64, op by op at the smallest shapes that exercise the tails,
then the whole network against the restated fp64 module (tests/inception_ref.py), the bit-for-bit properties (batch size and
position, graph replay, weight reload), and the set evaluator's surface (utils/metrics.py: SetEvaluator, FIDMetric,
InceptionScoreMetric).

Error bounds, none of them measured.  u = 2^-24.
  conv: the accumulator A is an fp32 fmaf chain over K products; against the exact value A* of the same fp32 operands
    |A - A*| <= (K + 8) u S, S = the same expression on absolute values (the worst-case bound of tests/test_gpu_lpips.py).
    The epilogue is r = fl(fma(A, s, t)) with s = s*(1 + d1), t = t*(1 + d2) the once-rounded fp64 fold (s*, t* exact in fp64 from
    the fp32 BatchNorm parameters), |d| <= u, and one rounding d3 of the fma:
        |r - (A* s* + t*)| <= |s*| (K + 8) u S   (the accumulator)  +  u |s*| |A|   (s rounded)  +  u |t*|   (t rounded)
                              +  u |A s + t|   (the fma)            <=  u ((K + 10) |s*| S + 2 |t*|)       to first order;
    the test allows u ((K + 12) |s*| S + 3 |t*|), the two extra units absorbing every second-order term.  ReLU is 1-Lipschitz.
    With the frame prologue the operands are the mapped pixels, restated in numpy float32 step by step (the same bits).
  max pool: exact.
  avg pool: at most nine terms added in fp32 and one division: |err| <= 9 u sum|x| / 9 + u |result| <= 10 u mean9|x|, where
    mean9|x| = sum|x| / 9 over the window; a constant image gives 4/9, 6/9, 1 to one ulp (the sums 4, 6, 9 are exact).
  global pool: added and divided in fp64, rounded once: |err| <= u |exact| + P 2^-52 mean|x|.
  whole network: the project's golden rule -- the relative L2 error of a frame's features against fp64 is at most 4 x the error
    the restated fp32 torch module has against fp64 for that case (measured on the CPU, recorded in
    tests/golden/inception_synth.npz as ref_fp32_rel_err; the factor 4 is headroom for another summation order).
Every test prints the figures it compares before it asserts (run with -s); DESIGN.md section 3.10 keeps the observed ratios."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from impersonator_amd import _lib
from impersonator_amd.networks import inception as inception_net
from impersonator_amd.utils import metrics, synthetic
from tests import inception_ref
from tests import metrics_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


# ------------------------------------------------------------------------------------------------ conv, op level
def _conv_case(seed, N, H, W, Cin, Cout, k, stride=1, pad=0, mode=-1, y=None, pitch=None, off=0, x=None):
    """Runs lwg_inception_conv (BatchNorm folded, ReLU) and the fp64 statement of the same thing; asserts the bound of the module
    docstring element by element.  k, pad: an int or (h, w).  y: an NaN-prefilled (N,Ho,Wo,pitch) buffer to write channels
    off .. off + Cout - 1 of (a fresh one of pitch Cout by default).  -> (y, got, want)"""
    kh, kw = (k, k) if isinstance(k, int) else k
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    rs = np.random.RandomState(seed)
    if x is None:
        lo = 0.0 if mode == 1 else -1.0
        x = rs.uniform(lo, 1.0, (N, Cin, H, W)).astype(np.float32) if mode >= 0 else rs.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = torch.from_numpy((rs.standard_normal((Cout, Cin, kh, kw)) * np.sqrt(2.0 / (Cin * kh * kw))).astype(np.float32))
    gamma, beta = rs.uniform(0.5, 1.5, Cout).astype(np.float32), rs.normal(0, 0.1, Cout).astype(np.float32)
    mean, var = rs.normal(0, 0.2, Cout).astype(np.float32), rs.uniform(0.5, 2.0, Cout).astype(np.float32)
    scale, shift = inception_net.fold_bn(gamma, beta, mean, var)
    s64 = torch.from_numpy(gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-3))
    t64 = torch.from_numpy(beta.astype(np.float64)) - torch.from_numpy(mean.astype(np.float64)) * s64
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    xa = torch.from_numpy(metrics_ref.map_pixels(x, mode) if mode >= 0 else x).double()
    want = F.relu(F.conv2d(xa, w.double(), None, stride=stride, padding=(ph, pw)) * s64.view(1, -1, 1, 1) + t64.view(1, -1, 1, 1))
    mag = F.conv2d(xa.abs(), w.double().abs(), None, stride=stride, padding=(ph, pw))
    K = kh * kw * Cin
    bound = U * ((K + 12) * s64.abs().view(1, -1, 1, 1) * mag + 3 * t64.abs().view(1, -1, 1, 1)) + 1e-30

    lib = _lib.load()
    xd = _dev(x) if mode >= 0 else _nhwc(torch.from_numpy(x))
    wd, sd, td = w.permute(2, 3, 1, 0).contiguous().cuda(), scale.cuda(), shift.cuda()
    pitch = Cout if pitch is None else pitch
    if y is None:
        y = torch.full((N, Ho, Wo, pitch), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")          # allocated right after y: an overrun of y would land here
    _lib.check(lib.lwg_inception_conv(_lib.ptr(xd), N, H, W, Cin, _lib.ptr(wd), _lib.ptr(sd), _lib.ptr(td), Cout, kh, kw, stride, ph, pw, 1,
                                      mode, _lib.ptr(y), pitch, off, _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = y[..., off:off + Cout].permute(0, 3, 1, 2).double().cpu()
    assert tuple(got.shape) == tuple(want.shape)
    assert bool(torch.isfinite(got).all()) and bool((guard == 7.0).all())
    ratio = float(((got - want).abs() / bound).max())
    print("conv k%dx%d s%d p(%d,%d) mode %d N%d %dx%d %d->%d (M = %d, K = %d): max |err| %.3g, worst err / bound %.3g" % (
        kh, kw, stride, ph, pw, mode, N, H, W, Cin, Cout, N * Ho * Wo, K, float((got - want).abs().max()), ratio))
    assert ratio <= 1.0
    return y, got, want


def test_conv_1x7_and_7x1_cout_below_a_tile_with_an_m_tail():
    """N = 2, 5x9, 16 -> 48: the asymmetric image catches a swapped kh / kw; M = 90 leaves a tail of the second pixel tile"""
    _conv_case(1, N=2, H=5, W=9, Cin=16, Cout=48, k=(1, 7), pad=(0, 3))
    _conv_case(2, N=2, H=5, W=9, Cin=16, Cout=48, k=(7, 1), pad=(3, 0))


def test_conv_1x3_and_3x1_write_the_two_halves_of_one_buffer():
    y = torch.full((2, 3, 3, 768), float("nan"), device="cuda")
    _, first, _ = _conv_case(3, N=2, H=3, W=3, Cin=64, Cout=384, k=(1, 3), pad=(0, 1), y=y, pitch=768, off=0)
    assert bool(torch.isnan(y[..., 384:]).all())                              # the neighbouring slice is untouched
    _conv_case(4, N=2, H=3, W=3, Cin=64, Cout=384, k=(3, 1), pad=(1, 0), y=y, pitch=768, off=384)
    assert torch.equal(y[..., :384].permute(0, 3, 1, 2).double().cpu(), first)    # and the first half kept its bits
    # a slice in the middle of a wider buffer: both neighbours stay NaN
    z = torch.full((2, 3, 3, 96), float("nan"), device="cuda")
    _conv_case(5, N=2, H=3, W=3, Cin=16, Cout=48, k=(1, 3), pad=(0, 1), y=z, pitch=96, off=16)
    assert bool(torch.isnan(z[..., :16]).all()) and bool(torch.isnan(z[..., 64:]).all())


def test_conv3_stride2_rows_and_columns_no_window_reaches():
    _conv_case(6, N=1, H=8, W=10, Cin=32, Cout=64, k=3, stride=2)                 # 3x4: row 7 and column 9 are never read


def test_conv5_every_pixel_at_a_border():
    _conv_case(7, N=2, H=5, W=5, Cin=48, Cout=64, k=5, pad=2)


def test_conv1_cin_no_multiple_of_32():
    _conv_case(8, N=1, H=6, W=7, Cin=80, Cout=192, k=1)                           # K = 80: two and a half stages


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv3_stride2_from_frames(mode):
    x = None
    if mode == 2:
        # values on the quantiser's steps, the two ends, and values outside [-1,1] that the clamp catches
        x = np.random.RandomState(20).uniform(-1, 1, (2, 3, 11, 13)).astype(np.float32)
        steps = ((np.arange(13, dtype=np.float32) * 16 / np.float32(255)) * np.float32(2)) - np.float32(1)
        x[0, 0, 0, :], x[0, 1, 1, :4], x[1, 2, 10, 9:] = steps, [-1.0, 1.0, 1.25, -1.5], [1.0, -1.0, 0.0, 1e-3]
    _conv_case(10 + mode, N=2, H=11, W=13, Cin=3, Cout=32, k=3, stride=2, mode=mode, x=x)     # 5x6: M = 60, K = 27


def test_conv3_long_k():
    _conv_case(14, N=1, H=3, W=3, Cin=448, Cout=384, k=3, pad=1)                   # K = 4032, the longest of the network


def test_conv_five_channel_tiles():
    _conv_case(15, N=1, H=4, W=4, Cin=192, Cout=320, k=3, stride=1, pad=0)         # Cout = 320: five 64-wide tiles


# ------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("c,pitch,off", [(64, 64, 0), (288, 768, 480)])
@pytest.mark.parametrize("h,w", [(7, 7), (8, 8), (15, 9)])
def test_maxpool_is_floor_mode_and_writes_a_slice(h, w, c, pitch, off):
    rs = np.random.RandomState(h * 100 + w + c)
    x = torch.from_numpy(-rs.uniform(0.5, 3.0, (2, c, h, w)).astype(np.float32))      # all negative: a zero tap would win
    want = F.max_pool2d(x.double(), kernel_size=3, stride=2)
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    assert tuple(want.shape[-2:]) == (ho, wo)
    y = torch.full((2, ho, wo, pitch), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")
    xd = _nhwc(x)
    _lib.check(_lib.load().lwg_inception_maxpool(_lib.ptr(xd), 2, h, w, c, _lib.ptr(y), pitch, off, _lib.stream_ptr()))
    got = y[..., off:off + c].permute(0, 3, 1, 2).double().cpu()
    assert torch.equal(got, want) and float(got.max()) < 0 and bool((guard == 7.0).all())
    assert bool(torch.isnan(y[..., :off]).all()) and bool(torch.isnan(y[..., off + c:]).all())


def _avgpool(x):
    n, c, h, w = x.shape
    y = torch.full((n, h, w, c), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")
    xd = _nhwc(x)
    _lib.check(_lib.load().lwg_inception_avgpool(_lib.ptr(xd), n, h, w, c, _lib.ptr(y), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    return y.permute(0, 3, 1, 2).cpu()


def test_avgpool_divides_by_nine_everywhere():
    got = _avgpool(torch.ones((1, 8, 4, 5))).double()
    want = torch.full((4, 5), 1.0, dtype=torch.float64)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 6.0 / 9.0
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = 4.0 / 9.0
    err = float((got - want).abs().max())
    print("avg pool of ones: corners %.9g, edges %.9g, inside %.9g; max |err| %.3g (one ulp of 4/9 = %.3g)" % (
        float(got[0, 0, 0, 0]), float(got[0, 0, 0, 1]), float(got[0, 0, 1, 1]), err, 2.0 ** -25))
    assert bool((got[0, :, 1:-1, 1:-1] == 1.0).all())
    assert bool(((got - want).abs() <= want * 2.0 ** -23).all())                  # one ulp: ulp(x) <= 2^-23 x


@pytest.mark.parametrize("h,w,c", [(1, 1, 4), (3, 2, 192), (6, 7, 288)])
def test_avgpool_against_fp64(h, w, c):
    rs = np.random.RandomState(h * 10 + w)
    x = torch.from_numpy(rs.standard_normal((2, c, h, w)).astype(np.float32))
    got = _avgpool(x).double()
    want = F.avg_pool2d(x.double(), 3, 1, 1)                                    # count_include_pad=True
    bound = 10 * U * F.avg_pool2d(x.double().abs(), 3, 1, 1) + 1e-30
    ratio = float(((got - want).abs() / bound).max())
    print("avg pool %dx%dx%d: max |err| %.3g, worst err / bound %.3g" % (h, w, c, float((got - want).abs().max()), ratio))
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0


@pytest.mark.parametrize("P,C", [(1, 2048), (2, 2048), (64, 320)])
def test_global_pool_against_fp64(P, C):
    rs = np.random.RandomState(P + C)
    x = np.maximum(rs.standard_normal((3, P, C)), 0).astype(np.float32) * 3
    xd = _dev(x)
    y = torch.full((3, C), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")
    _lib.check(_lib.load().lwg_inception_global_pool(_lib.ptr(xd), 3, P, C, _lib.ptr(y), _lib.stream_ptr()))
    got = y.double().cpu().numpy()
    want = x.astype(np.float64).mean(axis=1)
    bound = U * np.abs(want) + P * 2.0 ** -52 * np.abs(x.astype(np.float64)).mean(axis=1) + 1e-300
    ratio = float((np.abs(got - want) / bound).max())
    print("global pool P=%d C=%d: max |err| %.3g, worst err / bound %.3g" % (P, C, float(np.abs(got - want).max()), ratio))
    assert np.isfinite(got).all() and ratio <= 1.0 and bool((guard == 7.0).all())


# ------------------------------------------------------------------------------------------------ whole network
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "inception_synth.npz"))


@pytest.fixture(scope="module")
def weights(gold):
    return synthetic.inception_state_dict(int(gold["seed"]))


@pytest.fixture(scope="module")
def model(weights):
    m = inception_net.InceptionV3(weights, max_batch=8, image_size=112)
    yield m
    m.release()


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.linalg.norm(a.reshape(len(a), -1) - b.reshape(len(b), -1), axis=1) / np.linalg.norm(b.reshape(len(b), -1), axis=1)).max())


def _first_bad_stage(model, weights, frames, resize, yard):
    """walks tap_stage over the 18 stages against the restated modules on the CPU: the name of the first stage whose relative L2
    error exceeds 4 x max(the fp32 module's error at that stage, the case's yardstick)"""
    x = torch.from_numpy(frames)
    s64, s32 = [], []
    with torch.no_grad():
        inception_ref.build(weights, torch.float64)(inception_ref.preprocess(x.double(), resize), stages=s64)
        inception_ref.build(weights, torch.float32)(inception_ref.preprocess(x, resize), stages=s32)
    hw = (resize, resize) if resize else frames.shape[-2:]
    for stage, (hs, ws, cs) in enumerate(inception_net.stage_shapes(*hw)):
        tap = torch.full((len(frames), hs, ws, cs), float("nan"), device="cuda")
        model(_dev(frames), mode=1, resize=resize, tap=(stage, tap))
        got = tap.permute(0, 3, 1, 2).double().cpu().numpy()
        e_dev, e_ref = _rel_l2(got, s64[stage].numpy()), _rel_l2(s32[stage].numpy(), s64[stage].numpy())
        print("  stage %2d %-14s %s: device rel L2 %.3g, restated fp32 %.3g" % (stage, inception_ref.STAGES[stage], (hs, ws, cs), e_dev, e_ref))
        if not e_dev <= 4 * max(e_ref, yard):
            return "%d (%s)" % (stage, inception_ref.STAGES[stage])
    return "none: the stages hold, the global pool does not"


@pytest.mark.parametrize("index", [0, 1])
def test_whole_network_against_fp64(model, weights, gold, index):
    """case 0: three 107x91 frames as they are -- 53x45 -> 51x43 -> 25x21 -> 23x19 -> 11x9 -> 5x4 -> 2x1, the final pool averages
    two pixels -- against the fp64 module live; case 1: one 64x48 frame resized to 299x299, against the golden fp64 features"""
    name, n, h, w, resize = inception_ref.CASES[index]
    assert str(gold["case_names"][index]) == name and gold["case_shapes"][index].tolist() == [n, h, w, resize]
    frames = inception_ref.case_frames(index)
    yard = float(gold["ref_fp32_rel_err"][index])
    if index == 0:
        with torch.no_grad():
            want = inception_ref.build(weights, torch.float64)(inception_ref.preprocess(torch.from_numpy(frames).double(), resize)).numpy()
        assert _rel_l2(want, gold[name + "_features_fp64"]) <= 1e-12             # the live module is the golden's
    else:
        want = gold[name + "_features_fp64"]
    got = model(_dev(frames), mode=1, resize=resize).cpu().numpy()
    err = _rel_l2(got, want)
    print("%s: device rel L2 %.3g = %.3g x ref_fp32_rel_err (%.3g); features mean %.3g, max |err| %.3g" % (
        name, err, err / yard, yard, float(np.abs(want).mean()), float(np.abs(got - want).max())))
    assert got.shape == (n, 2048) and np.isfinite(got).all()
    if not err <= 4 * yard:
        pytest.fail("%s: rel L2 %.3g above 4 x %.3g; first stage out of bound: %s" % (name, err, yard, _first_bad_stage(model, weights, frames, resize, yard)))


def test_a_tap_is_the_stage_of_the_restated_module(model, weights):
    """the tap mechanism itself, on the smallest input: Mixed_6a (a block with a max-pool branch) and the pre-pool map"""
    frames = ((synthetic.smooth_image(31, (2, 3, 75, 80)) + 1) / 2).astype(np.float32)
    stages = []
    with torch.no_grad():
        want = inception_ref.build(weights, torch.float64)(inception_ref.preprocess(torch.from_numpy(frames).double(), 0), stages=stages)
    shapes = inception_net.stage_shapes(75, 80)
    feats = None
    for stage in (3, 10, 17):
        hs, ws, cs = shapes[stage]
        assert tuple(stages[stage].shape) == (2, cs, hs, ws)
        tap = torch.full((2, hs, ws, cs), float("nan"), device="cuda")
        feats = model(_dev(frames), mode=1, resize=0, tap=(stage, tap))
        err = _rel_l2(tap.permute(0, 3, 1, 2).cpu().numpy(), stages[stage].numpy())
        print("tap %d (%s) %s: rel L2 against fp64 %.3g" % (stage, inception_ref.STAGES[stage], (hs, ws, cs), err))
        assert bool(torch.isfinite(tap).all()) and err <= 1e-5
    assert _rel_l2(feats.cpu().numpy(), want.numpy()) <= 1e-5
    assert torch.equal(feats, model(_dev(frames), mode=1, resize=0))              # a tap changes nothing


# ------------------------------------------------------------------------------------------------ bit-for-bit properties
@pytest.fixture(scope="module")
def eight():
    """eight 88x80 frames in [-1,1]: noise and smooth images"""
    rs = np.random.RandomState(77)
    return _dev(np.concatenate([rs.uniform(-1, 1, (4, 3, 88, 80)).astype(np.float32), synthetic.smooth_image(78, (4, 3, 88, 80))]))


def test_batch_size_and_position_bit_for_bit(model, eight):
    whole = model(eight, resize=0)
    assert bool(torch.isfinite(whole).all()) and torch.equal(whole, model(eight, resize=0))
    assert float((whole[0] - whole[1]).abs().max()) > 1e-3                        # the frames do differ
    for i in (0, 3, 7):
        assert torch.equal(model(eight[i:i + 1], resize=0)[0], whole[i]), i       # batch 1
    for s in (0, 2, 5):
        assert torch.equal(model(eight[s:s + 3], resize=0), whole[s:s + 3]), s    # batch 3, three positions
    moved = model(torch.cat([eight[5:], eight[:5]]).contiguous(), resize=0)
    assert torch.equal(moved, torch.cat([whole[5:], whole[:5]]))
    # the resized path, and a batch above max_batch (chunks of 8, 8, 1)
    resized = model(eight)
    assert torch.equal(model(eight[6:7])[0], resized[6]) and not torch.equal(resized, whole)
    many = model(torch.cat([eight, eight, eight[2:3]]).contiguous(), resize=0)
    assert torch.equal(many, torch.cat([whole, whole, whole[2:3]]))


def test_a_forward_replays_as_a_graph_on_new_inputs(model, eight):
    eager = [model(eight[s:s + 2]) for s in (0, 4)]
    static = eight[:2].clone()
    out = torch.zeros((2, 2048), device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        model(static, out=out)
    for s, want in zip((0, 4), eager):
        static.copy_(eight[s:s + 2])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), s


def test_set_weights_of_a_second_seed_and_back(model, weights, eight):
    before = model(eight[:2], resize=0)
    handle = model._ensure_handle().value
    try:
        model.load_state_dicts(synthetic.inception_state_dict(1))
        other = model(eight[:2], resize=0)
        assert model._handle.value == handle
        rel = _rel_l2(other.cpu().numpy(), before.cpu().numpy())
        print("second seed: features change by %.3g relative L2" % rel)
        assert rel > 1e-2
    finally:
        model.load_state_dicts(weights)
    assert torch.equal(model(eight[:2], resize=0), before)


def test_forward_refuses_what_the_handle_is_not_built_for(model):
    h = model._ensure_handle()
    lib = _lib.load()
    buf = torch.zeros(3 * 112 * 112, device="cuda")
    out = torch.full((9 * 2048,), 7.0, device="cuda")
    fwd = lambda n=1, hh=96, ww=96, mode=0, oh=0, ow=0, stage=-1, tap=None: lib.lwg_inception_forward(
        h, _lib.ptr(buf), n, hh, ww, mode, oh, ow, _lib.ptr(out), stage, _lib.ptr(tap), _lib.stream_ptr())
    assert fwd(hh=74) == -2 and b"Mixed_7c" in lib.lwg_last_error()
    assert fwd(ww=74) == -2 and fwd(hh=20, ww=20, oh=299, ow=299) == 0            # resized, a small frame is fine
    assert fwd(n=9) == -5 and b"max_images" in lib.lwg_last_error()
    assert fwd(hh=113) == -5 and fwd(ww=300) == -5
    assert fwd(mode=3) == -1 and fwd(mode=-1) == -1
    assert fwd(oh=299) == -1 and fwd(oh=224, ow=224) == -1
    assert fwd(stage=18) == -1 and fwd(stage=-2) == -1 and fwd(stage=4) == -1     # a stage without tap_out
    with pytest.raises(_lib.LwgError) as e:
        model(torch.zeros((1, 3, 60, 80), device="cuda"), resize=0)
    assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ the evaluator's surface
# One 2048 x 2048 sqrtm takes about 4 s on the host (the cost of the reference's own method), so the three routes to the same FID
# -- SetEvaluator.result(), the host functions on the same features, the reference-shaped metric classes -- are one sqrtm each:
# the evaluator's in the fixture, the other two in a test each.  The host side is fp64 and deterministic: they agree to 1e-12.
@pytest.fixture(scope="module")
def scored(model):
    """40 synthetic [0,1] frames and 40 references through SetEvaluator(mode=1) in updates of 8, under torch's synchronisation
    guard: a .cpu(), .item() or synchronize() inside update would raise"""
    rs = np.random.RandomState(91)
    preds = np.clip(synthetic.smooth_image(92, (40, 3, 40, 36)) + 0.2 * rs.uniform(-1, 1, (40, 3, 40, 36)), -1, 1)
    refs = np.clip(synthetic.smooth_image(93, (40, 3, 40, 36)) + 0.1 * rs.uniform(-1, 1, (40, 3, 40, 36)), -1, 1)
    dp, dr = _dev(((preds + 1) / 2).astype(np.float32)), _dev(((refs + 1) / 2).astype(np.float32))
    model(dp[:1], mode=1)                             # the handle exists and the weights are up before the guard is set
    ev = metrics.SetEvaluator(model, mode=1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(0, 40, 8):
            ev.update(dp[s:s + 8], dr[s:s + 8])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return dp, dr, ev, ev.result()


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(b), 1e-300)


def test_set_evaluator_against_the_host_functions(model, scored):
    dp, dr, ev, out = scored
    fp, fr = model(dp, mode=1).cpu().numpy().astype(np.float64), model(dr, mode=1).cpu().numpy().astype(np.float64)
    got_p, got_r = ev.features()
    assert np.array_equal(got_p, fp) and np.array_equal(got_r, fr) and out["frames"] == len(ev) == 40
    fid = metrics.fid_from_features(fp, fr)
    is_mean, is_std = metrics.inception_score(fp, 32)
    print("SetEvaluator: fid %.12g (host functions %.12g), is %.12g +- %.12g (host %.12g +- %.12g), is_ref %.12g" % (
        out["fid"], fid, out["is"], out["is_std"], is_mean, is_std, out["is_ref"]))
    assert sorted(out) == ["fid", "frames", "is", "is_ref", "is_std"]
    assert np.isfinite([out["fid"], out["is"], out["is_std"], out["is_ref"]]).all() and out["fid"] > 0 and out["is"] >= 1 and out["is_std"] > 0
    assert _close(out["fid"], fid) and _close(out["is"], is_mean) and _close(out["is_std"], is_std)
    assert _close(out["is_ref"], metrics.inception_score(fr, 32)[0])
    # preds alone: no fid; the table grows without losing rows
    alone = metrics.SetEvaluator(model, mode=1)
    for _ in range(3):
        alone.update(dp)
    res = alone.result()
    assert sorted(res) == ["frames", "is", "is_std"] and res["frames"] == 120
    assert np.array_equal(alone.features()[0], np.tile(fp, (3, 1))) and alone.features()[1] is None
    # mode 1 is 2*x - 1 in front of the network
    mapped = model(_dev(metrics_ref.map_pixels(dp[:2].cpu().numpy(), 1)), mode=0)
    assert torch.equal(mapped, model(dp[:2], mode=1))


def test_set_evaluator_against_the_metric_classes(model, scored):
    dp, dr, ev, out = scored
    score = metrics.FIDMetric(model).calculate_score(dp, dr)
    m, s = metrics.InceptionScoreMetric(model).calculate_score(dp)
    print("FIDMetric %.12g (SetEvaluator %.12g), InceptionScoreMetric %.12g +- %.12g (SetEvaluator %.12g +- %.12g)" % (
        score, out["fid"], m, s, out["is"], out["is_std"]))
    assert _close(score, out["fid"]) and _close(m, out["is"]) and _close(s, out["is_std"])
    assert _close(metrics.InceptionScoreMetric(model).calculate_score(list(dr))[0], out["is_ref"])     # a list of frames, as the reference takes
