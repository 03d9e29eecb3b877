"""GPU: the HMR regressor's kernels (csrc/hmr.hip) against torch in fp64, op by op at the smallest shapes that exercise the
tails, then whole models against the golden fp64 values, batch invariance bit for bit, weight reloads, the profiler / HIP-graph
check, and the Imitator end to end from images only.

Error bounds.  A convolution output is an fp32 fmaf chain over K products plus a handful of roundings in the prologue and
epilogue; against the exact value its error is at most (K + 8) * 2^-24 * S, S = the same expression evaluated on absolute
values (the standard worst-case bound of a length-K recursive sum; nothing here is measured).  Whole models are held to the
rule of the golden file: at most 4 x the error the reference's OWN fp32 forward has against fp64 (headroom for another
summation order plus the one extra rounding of the folded BatchNorm).
Every test prints the figures it compares before it asserts (run with -s); DESIGN.md section 3.8 keeps the observed ratios."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from impersonator_amd import _lib, demo
from impersonator_amd.networks import batch_smpl
from impersonator_amd.networks import hmr as hmr_net
from impersonator_amd.utils import synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def _conv_case(seed, N, H, W, Cin, Cout, k, stride, pad, pre=False, bias=False, post=False, res_stride=0, res_hw=None):
    """Runs lwg_hmr_conv and the fp64 statement of the same thing; asserts the worst-case fp32 bound element by element."""
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    x = t(rs.standard_normal((N, Cin, H, W)))
    w = t(rs.standard_normal((Cout, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k)))
    ps, pb = (t(rs.uniform(0.5, 1.5, Cin)), t(rs.normal(0, 0.3, Cin))) if pre else (None, None)
    b = t(rs.normal(0, 0.2, Cout)) if bias else None
    qs, qb = (t(rs.uniform(0.5, 1.5, Cout)), t(rs.normal(0, 0.3, Cout))) if post else (None, None)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = None
    if res_stride:
        rh, rw = res_hw if res_hw else (Ho, Wo)
        res = t(rs.standard_normal((N, Cout, rh, rw)))
    # fp64 statement (on the fp32 operands) and the magnitude S of the bound
    xa = x.double()
    if pre:
        xa = F.relu(xa * ps.double().view(1, -1, 1, 1) + pb.double().view(1, -1, 1, 1))
    want = F.conv2d(xa, w.double(), None if b is None else b.double(), stride=stride, padding=pad)
    mag = F.conv2d(xa.abs(), w.double().abs(), None if b is None else b.double().abs(), stride=stride, padding=pad)
    if post:
        want = F.relu(want * qs.double().view(1, -1, 1, 1) + qb.double().view(1, -1, 1, 1))
        mag = mag * qs.double().abs().view(1, -1, 1, 1) + qb.double().abs().view(1, -1, 1, 1)
    if res is not None:
        sl = res.double()[:, :, ::res_stride, ::res_stride][:, :, :Ho, :Wo]
        want = want + sl
        mag = mag + sl.abs()
    bound = (k * k * Cin + 8) * U * mag + 1e-30

    lib = _lib.load()
    dev = lambda v: None if v is None else v.cuda().contiguous()
    xd, wd = _nhwc(x), w.permute(2, 3, 1, 0).contiguous().cuda()
    psd, pbd, bd, qsd, qbd = dev(ps), dev(pb), dev(b), dev(qs), dev(qb)
    resd = None if res is None else _nhwc(res)
    y = torch.full((N, Ho, Wo, Cout), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")          # allocated right after y: an overrun of y would land here
    _lib.check(lib.lwg_hmr_conv(_lib.ptr(xd), N, H, W, Cin, _lib.ptr(wd), Cout, k, stride, pad, _lib.ptr(psd), _lib.ptr(pbd),
                                _lib.ptr(bd), _lib.ptr(qsd), _lib.ptr(qbd), _lib.ptr(resd), max(res_stride, 1),
                                res.shape[2] if res is not None else 1, res.shape[3] if res is not None else 1, _lib.ptr(y),
                                _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = y.permute(0, 3, 1, 2).double().cpu()
    assert bool(torch.isfinite(got).all()) and bool((guard == 7.0).all())
    ratio = float(((got - want).abs() / bound).max())
    print("conv k%d s%d N%d %dx%d %d->%d: max |err| %.3g, worst err / bound %.3g" % (
        k, stride, N, H, W, Cin, Cout, float((got - want).abs().max()), ratio))
    assert ratio <= 1.0


def test_conv1x1_prologue_bias_residual_under_one_tile():
    _conv_case(1, N=3, H=7, W=7, Cin=64, Cout=256, k=1, stride=1, pad=0, pre=True, bias=True, res_stride=1)   # M = 147


def test_conv1x1_long_k_ragged_m():
    _conv_case(2, N=1, H=14, W=14, Cin=1024, Cout=256, k=1, stride=1, pad=0, pre=True, bias=True, res_stride=1)   # M = 196


def test_conv1x1_residual_from_a_stride_two_slice():
    _conv_case(3, N=2, H=7, W=7, Cin=128, Cout=256, k=1, stride=1, pad=0, pre=True, bias=True, res_stride=2, res_hw=(14, 14))


def test_conv3x3_stride1_every_pixel_at_a_border():
    _conv_case(4, N=2, H=7, W=7, Cin=64, Cout=64, k=3, stride=1, pad=1, post=True)


def test_conv3x3_stride2():
    _conv_case(5, N=1, H=14, W=14, Cin=128, Cout=128, k=3, stride=2, pad=1, post=True)


def test_stem_7x7_stride2_with_bias():
    _conv_case(6, N=2, H=32, W=32, Cin=3, Cout=64, k=7, stride=2, pad=3, bias=True)


def test_maxpool_overhang_is_ignored_not_zero():
    rs = np.random.RandomState(7)
    x = torch.from_numpy(-rs.uniform(0.5, 3.0, (2, 64, 16, 16)).astype(np.float32))      # all negative: a zero tap would win
    want = F.max_pool2d(x.double(), kernel_size=3, stride=2, ceil_mode=True)
    assert want.shape[-1] == 8
    y = torch.full((2, 8, 8, 64), float("nan"), device="cuda")
    xd = _nhwc(x)
    _lib.check(_lib.load().lwg_hmr_maxpool(_lib.ptr(xd), 2, 16, 16, 64, _lib.ptr(y), _lib.stream_ptr()))
    got = y.permute(0, 3, 1, 2).double().cpu()
    assert torch.equal(got, want) and float(got.max()) < 0


def test_pool_features_against_fp64():
    rs = np.random.RandomState(8)
    x = torch.from_numpy(rs.standard_normal((3, 2048, 7, 7)).astype(np.float32) * 3)
    s = torch.from_numpy(rs.uniform(0.5, 1.5, 2048).astype(np.float32))
    b = torch.from_numpy(rs.normal(0, 0.3, 2048).astype(np.float32))
    act = F.relu(x.double() * s.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1))
    want = act.mean(dim=(2, 3))
    out = torch.full((3, 2048), float("nan"), device="cuda")
    xd, sd, bd = _nhwc(x).reshape(3, 49, 2048), s.cuda(), b.cuda()
    _lib.check(_lib.load().lwg_hmr_pool_features(_lib.ptr(xd), 3, 49, 2048, _lib.ptr(sd), _lib.ptr(bd), _lib.ptr(out),
                                                 _lib.stream_ptr()))
    # 49 additions of non-negative terms + the affine + the division: (49 + 4) * 2^-24 relative to the mean itself
    err = (out.double().cpu() - want).abs()
    bound = (49 + 4) * U * (x.double().abs() * s.double().view(1, -1, 1, 1) + b.double().abs().view(1, -1, 1, 1)).mean(dim=(2, 3))
    print("pool_features: worst err / bound %.3g" % float((err / bound).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("n", [3, 9])
def test_regress_against_fp64(n):
    """ThetaRegressor on device rows (9: more than the eight rows one launch carries).  The yardstick is the regressor's own
    fp32 evaluation by torch on the CPU: the device may be at most 4 x as far from fp64 as that is."""
    torch.manual_seed(0)
    reg = hmr_net.ThetaRegressor(2048 + 85, 85, 3).eval()
    sd = {k[len("regressor."):]: torch.from_numpy(np.asarray(v)) for k, v in synthetic.hmr_state_dict(2, (1, 1, 1, 1)).items()
          if k.startswith("regressor.")}
    reg.load_state_dict(sd)
    feat = torch.from_numpy(np.abs(np.random.RandomState(9).standard_normal((n, 2048))).astype(np.float32))
    with torch.no_grad():
        t32 = reg(feat)
        t64 = reg.double()(feat.double())
    reg.float()
    fc = reg.fc_blocks
    w = [t.detach().float().cuda().contiguous() for t in (reg.mean_theta, fc.fc1.weight, fc.fc1.bias, fc.fc2.weight, fc.fc2.bias,
                                                          fc.fc3.weight, fc.fc3.bias)]
    lib = _lib.load()
    nbytes = lib.lwg_hmr_regress_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((n, 85), float("nan"), device="cuda")
    fd = feat.cuda()
    _lib.check(lib.lwg_hmr_regress(_lib.ptr(fd), n, *[_lib.ptr(t) for t in w], _lib.ptr(out), _lib.ptr(ws), nbytes,
                                   _lib.stream_ptr()))
    e_dev = float((out.double().cpu() - t64).abs().max())
    e_ref = float((t32.double() - t64).abs().max())
    print("regress n=%d: device %.3g, torch fp32 %.3g, ratio %.3g" % (n, e_dev, e_ref, e_dev / e_ref))
    assert e_dev <= 4 * e_ref


# ------------------------------------------------------------------------------------------------ whole models
def _module(seed, num_blocks, max_batch=8):
    m = hmr_net.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0), num_blocks=num_blocks, max_batch=max_batch).eval()
    _load_seed(m, seed)
    return m


def _load_seed(m, seed):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.hmr_state_dict(seed, m.resnet.num_blocks).items()}
    for k, v in m.smpl.state_dict().items():
        sd["smpl." + k] = v.cpu()
    m.load_state_dict(sd)


def _errors(theta, feat, theta64, feat64):
    theta, feat = np.asarray(theta, np.float64), np.asarray(feat, np.float64)
    return float(np.abs(theta - theta64).max()), float(np.linalg.norm(feat - feat64) / np.linalg.norm(feat64))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "hmr_golden.npz"))


@pytest.fixture(scope="module")
def full_model(gold):
    return _module(int(gold["seed"]), (3, 4, 6, 3))


@pytest.fixture(scope="module")
def small_model():
    """[3,2,2,2]: every block kind -- shortcut conv, identity at stride 1, identity at stride 2."""
    return _module(1, (3, 2, 2, 2))


@pytest.fixture(scope="module")
def small_reference(small_model):
    """Nine images and the reduced net's tensor-op forward on the CPU in fp32 and fp64 (computed once, shared)."""
    x = torch.from_numpy(synthetic.smooth_image(21, (9, 3, 224, 224)))
    with torch.no_grad():
        t32, f32 = small_model.forward_ops(x[:3], return_features=True)
        small_model.resnet.double(), small_model.regressor.double()
        t64, f64 = small_model.forward_ops(x[:3].double(), return_features=True)
        small_model.resnet.float(), small_model.regressor.float()
    return x, t32.numpy(), f32.numpy(), t64.numpy(), f64.numpy()


def test_full_model_against_the_golden_fp64_values(full_model, gold):
    x = torch.from_numpy(synthetic.smooth_image(int(gold["input_seed"]), (2, 3, 224, 224))).cuda()
    full_model.cuda()
    theta, feat = full_model(x, return_features=True)
    theta, feat = theta.cpu().numpy(), feat.cpu().numpy()
    et_dev, ef_dev = _errors(theta, feat, gold["theta_fp64"], gold["features_fp64"])
    et_ref, ef_ref = _errors(gold["theta_fp32"], gold["features_fp32"], gold["theta_fp64"], gold["features_fp64"])
    d32 = float(np.abs(theta - gold["theta_fp32"]).max())
    print("full model: features rel L2 device %.3g / reference fp32 %.3g = %.3g; theta max abs device %.3g / reference fp32 %.3g "
          "= %.3g; |theta_device - theta_reference_fp32| %.3g = %.3g x e_theta(reference fp32)"
          % (ef_dev, ef_ref, ef_dev / ef_ref, et_dev, et_ref, et_dev / et_ref, d32, d32 / et_ref))
    assert np.isfinite(theta).all() and np.isfinite(feat).all()
    assert ef_dev <= 4 * ef_ref
    assert et_dev <= 4 * et_ref
    assert d32 <= 5 * et_ref


def test_reduced_net_against_fp64_at_batch_three(small_model, small_reference):
    x, t32, f32, t64, f64 = small_reference
    small_model.cuda()
    theta, feat = small_model(x[:3].cuda(), return_features=True)
    et_dev, ef_dev = _errors(theta.cpu().numpy(), feat.cpu().numpy(), t64, f64)
    et_ref, ef_ref = _errors(t32, f32, t64, f64)
    print("reduced net: features rel L2 device %.3g / torch fp32 %.3g = %.3g; theta max abs device %.3g / torch fp32 %.3g = %.3g"
          % (ef_dev, ef_ref, ef_dev / ef_ref, et_dev, et_ref, et_dev / et_ref))
    assert ef_dev <= 4 * ef_ref and et_dev <= 4 * et_ref


def test_batch_invariance_bit_for_bit(full_model):
    x = torch.from_numpy(synthetic.smooth_image(33, (9, 3, 224, 224))).cuda()
    full_model.cuda()
    alone_t, alone_f = full_model(x[0:1], return_features=True)
    three_t, three_f = full_model(x[0:3], return_features=True)
    eight = torch.cat([x[1:6], x[0:1], x[6:8]])                       # the image as row 5 of a batch of 8
    eight_t, eight_f = full_model(eight, return_features=True)
    assert torch.equal(alone_t[0], three_t[0]) and torch.equal(alone_f[0], three_f[0])
    assert torch.equal(alone_t[0], eight_t[5]) and torch.equal(alone_f[0], eight_f[5])
    # n = 9 through a handle sized for 4 (chunks of 4, 4, 1) == the same rows
    chunked = hmr_net.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0), max_batch=4).eval()
    chunked.load_state_dict({k: v.cpu() for k, v in full_model.state_dict().items()})
    chunked.cuda()
    nine_t, nine_f = chunked(x, return_features=True)
    assert torch.equal(nine_t[0], alone_t[0]) and torch.equal(nine_t[:3], three_t) and torch.equal(nine_f[:3], three_f)
    assert torch.equal(nine_t[8], full_model(x[8:9])[0])
    chunked.release()


def test_load_state_dict_of_a_second_seed_without_recreating_the_module(small_model, small_reference):
    x = small_reference[0]
    small_model.cuda()
    handle = small_model._ensure_handle().value
    before = small_model(x[:1].cuda()).cpu()
    _load_seed(small_model, 2)
    try:
        after_t, after_f = small_model(x[:1].cuda(), return_features=True)
        assert small_model._handle.value == handle
        with torch.no_grad():
            cpu = small_model.cpu()
            t32, f32 = cpu.forward_ops(x[:1], return_features=True)
            cpu.resnet.double(), cpu.regressor.double()
            t64, f64 = cpu.forward_ops(x[:1].double(), return_features=True)
            cpu.resnet.float(), cpu.regressor.float()
        et_dev, ef_dev = _errors(after_t.cpu().numpy(), after_f.cpu().numpy(), t64.numpy(), f64.numpy())
        et_ref, ef_ref = _errors(t32.numpy(), f32.numpy(), t64.numpy(), f64.numpy())
        print("second seed: features ratio %.3g, theta ratio %.3g" % (ef_dev / ef_ref, et_dev / et_ref))
        assert ef_dev <= 4 * ef_ref and et_dev <= 4 * et_ref
        assert float((after_t.cpu() - before).abs().max()) > 1e-3
    finally:
        _load_seed(small_model, 1)
        small_model.cuda()
    assert torch.equal(small_model(x[:1].cuda()).cpu(), before)


def test_forward_refuses_what_the_handle_is_not_built_for(small_model):
    small_model.cuda()
    h = small_model._ensure_handle()
    lib = _lib.load()
    buf = torch.zeros(16, device="cuda")
    assert lib.lwg_hmr_forward(h, _lib.ptr(buf), 9, 224, 224, _lib.ptr(buf), None, _lib.stream_ptr()) == -5
    assert b"max_batch" in lib.lwg_last_error()
    assert lib.lwg_hmr_forward(h, _lib.ptr(buf), 1, 256, 256, _lib.ptr(buf), None, _lib.stream_ptr()) == -2
    assert lib.lwg_hmr_weight_floats(h) == hmr_net.pack_weights(small_model.resnet, small_model.regressor).numel()
    fresh = ctypes.c_void_p()
    _lib.check(lib.lwg_hmr_create(ctypes.byref(fresh), 1, None))
    try:
        assert lib.lwg_hmr_forward(fresh, _lib.ptr(buf), 1, 224, 224, _lib.ptr(buf), None, _lib.stream_ptr()) == -5   # no weights
        assert lib.lwg_hmr_set_weights(fresh, ctypes.c_void_p(buf.cpu().data_ptr()), 16) == -1
    finally:
        lib.lwg_hmr_destroy(fresh)


def test_forward_launches_no_framework_kernel_and_replays_as_a_graph(full_model):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    x = torch.from_numpy(synthetic.smooth_image(41, (2, 3, 224, 224))).cuda()
    full_model.cuda()
    eager = full_model(x).clone()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        again = full_model(x)
        torch.cuda.synchronize()
    assert torch.equal(again, eager)
    records = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    foreign = sorted({k for k in records if "lwg" not in k})
    print("hmr forward: %d device records, others: %s" % (len(records), foreign))
    assert len(records) >= 53 + 2 + 1 + 10 and not foreign, foreign
    graph = torch.cuda.CUDAGraph()
    static = x.clone()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out = full_model(static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def _same(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a.float()), torch.nan_to_num(b.float()))


def test_imitator_from_images_only(small_model, tmp_path):
    """personalize / inference without SMPL vectors == the same calls with the vectors the regressor gives for those images.
    (On the code before the regressor both raised NotImplementedError.)  At image_size 128: the smallest the generator's handle takes
    ((image_size / 8)^2 must be a multiple of 128 pixels; 64 is refused by lwg_generator_create)."""
    from PIL import Image
    imitator, _, src_img, bg_img = demo.build_synthetic_imitator(batch_size=2, seed=0, image_size=128)
    small_model.cuda()
    imitator.hmr = small_model
    imitator.personalize(src_img, bg_img=bg_img)
    got = imitator.src_info
    img224 = torch.from_numpy(imitator._hmr_image(src_img)).cuda()[None]
    src_smpl = small_model(img224)[0]
    assert src_smpl.shape == (85,) and torch.equal(src_smpl, imitator._extract_smpls(src_img))
    imitator.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
    want = imitator.src_info
    for k in ("theta", "cam", "pose", "shape", "verts", "j2d", "j3d", "fim", "wim", "cond", "f2verts", "bg", "img", "p2verts_c"):
        assert _same(got[k], want[k]), k
    for a, b in zip(got["feats"], want["feats"]):
        for fa, fb in zip(a, b):
            assert _same(fa, fb)
    paths = []
    for i in range(3):
        arr = ((synthetic.smooth_image(50 + i, (1, 3, 96, 80))[0].transpose(1, 2, 0) + 1) * 127.5).astype(np.uint8)
        paths.append(str(tmp_path / ("frame_%d.png" % i)))
        Image.fromarray(arr).save(paths[-1])
    outs = imitator.inference(paths, verbose=False)
    smpls = [imitator._extract_smpls(p) for p in paths]
    outs2 = imitator.inference(paths, tgt_smpls=smpls, verbose=False)
    assert len(outs) == 3 and outs[0].shape == (128, 128, 3)
    for a, b in zip(outs, outs2):
        assert np.array_equal(a, b, equal_nan=True)
    assert not torch.equal(smpls[0], smpls[1])
    # transfer_params from a path alone (imitator.py:270-283)
    t_inputs = imitator.transfer_params(paths[1], cam_strategy="copy")
    t_inputs2 = imitator.transfer_params(paths[1], tgt_smpl=smpls[1], cam_strategy="copy")
    assert _same(t_inputs, t_inputs2)
