"""CPU: the host side of LPIPS -- tests/lpips_ref.py against the live reference and against the golden file, the weight blob's
layout, the missing-key errors, and every refusal of the lwg_lpips_* entry points that comes before the first HIP call."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from impersonator_amd import _lib
from impersonator_amd.networks import lpips as lpips_net
from impersonator_amd.utils import metrics, synthetic
from tests import lpips_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lpips_golden.npz")
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _golden_lin(gold):
    return {"lin%d.model.1.weight" % j: gold["lin%d" % j].reshape(1, -1, 1, 1) for j in range(5)}


def _maker():
    spec = importlib.util.spec_from_file_location("make_lpips_golden", os.path.join(ROOT, "tests", "golden", "make_lpips_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_equals_the_live_reference_in_fp64(gold):
    maker = _maker()
    if not maker.reference_available():
        pytest.skip("the reference tree is not present")
    alex, _ = synthetic.lpips_state_dicts(3)                      # not the golden's seed
    lin = maker.reference_lin_state_dict()
    for j in range(5):
        assert np.array_equal(lin["lin%d.model.1.weight" % j].numpy().reshape(-1), gold["lin%d" % j])
    net = maker.reference_model(alex, lin)
    worst = 0.0
    for index, kind in ((0, "noise"), (1, "near"), (2, "near")):
        pred, ref = lpips_ref.case_inputs(index, kind)
        d_ref, t_ref = maker.reference_forward(net, pred, ref, torch.float64)
        d, t = lpips_ref.lpips(pred, ref, alex, lin)
        worst = max(worst, float((np.abs(d - d_ref) / d_ref).max()), float((np.abs(t - t_ref) / t_ref).max()))
    print("lpips_ref vs the live reference, fp64: worst relative difference %.3g" % worst)
    assert worst <= 1e-12


def test_restatement_reproduces_the_golden_values(gold):
    alex, _ = synthetic.lpips_state_dicts(int(gold["seed"]))
    lin = _golden_lin(gold)
    assert [str(s) for s in gold["case_names"]] == [c[0] for c in lpips_ref.CASES]
    assert gold["case_shapes"].tolist() == [list(c[1:]) for c in lpips_ref.CASES]
    assert sum(gold["lin%d" % j].size for j in range(5)) == 1152 and all((gold["lin%d" % j] >= 0).all() for j in range(5))
    worst = 0.0
    for index, case in enumerate(lpips_ref.CASES[:3]):            # 256x256 is scored on the device (tests/test_gpu_lpips.py)
        for kind in ("noise", "near"):
            pred, ref = lpips_ref.case_inputs(index, kind)
            d, t = lpips_ref.lpips(pred, ref, alex, lin)
            key = "%s_%s" % (case[0], kind)
            worst = max(worst, float((np.abs(d - gold[key + "_dist_fp64"]) / gold[key + "_dist_fp64"]).max()),
                        float((np.abs(t - gold[key + "_taps_fp64"]) / gold[key + "_taps_fp64"]).max()))
    print("lpips_ref vs the golden fp64 values: worst relative difference %.3g; the reference's fp32 error %.3g (taps %.3g)"
          % (worst, float(gold["ref_fp32_rel_err"]), float(gold["ref_fp32_rel_err_taps"])))
    assert worst <= 1e-12
    assert 1e-9 < float(gold["ref_fp32_rel_err"]) < 1e-5


def test_pack_weights_layout():
    alex, lin = synthetic.lpips_state_dicts(5)
    blob = lpips_net.pack_weights(alex, lin).numpy()
    assert blob.dtype == np.float32 and blob.size == 2468544 + 1152 + 1152                 # conv weights, biases, lin
    off = 0
    for i, cout, cin, k in lpips_net.CONVS:
        w = alex["features.%d.weight" % i]
        assert w.shape == (cout, cin, k, k)
        block = blob[off:off + w.size].reshape(k, k, cin, cout)               # [kh][kw][ci][co]
        assert np.array_equal(block, w.transpose(2, 3, 1, 0))
        assert block[k - 1, 1, cin - 1, 2] == w[2, cin - 1, k - 1, 1]
        off += w.size
        assert np.array_equal(blob[off:off + cout], alex["features.%d.bias" % i])
        off += cout
    for j, c in enumerate(lpips_net.CHANNELS):
        v = lin["lin%d.model.1.weight" % j]
        assert v.shape == (1, c, 1, 1) and (v >= 0).all()
        assert np.array_equal(blob[off:off + c], v.reshape(-1))
        off += c
    assert off == blob.size
    # tensors, extra keys and DataParallel-free torchvision names are all accepted
    alex_t = {k: torch.from_numpy(v) for k, v in alex.items()}
    alex_t["classifier.1.weight"] = torch.zeros(4, 4)
    assert torch.equal(lpips_net.pack_weights(alex_t, lin), torch.from_numpy(blob))


def test_a_missing_key_is_named():
    alex, lin = synthetic.lpips_state_dicts(5)
    for drop in ("features.6.bias", "features.0.weight"):
        with pytest.raises(KeyError, match=drop.replace(".", r"\.")):
            lpips_net.pack_weights({k: v for k, v in alex.items() if k != drop}, lin)
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        lpips_net.LPIPS(alex, {k: v for k, v in lin.items() if k != "lin3.model.1.weight"})
    bad = dict(lin)
    bad["lin0.model.1.weight"] = np.zeros((1, 32, 1, 1), np.float32)
    with pytest.raises(ValueError):
        lpips_net.pack_weights(alex, bad)


def test_lpips_needs_a_model_and_cuda_tensors():
    with pytest.raises(ValueError):
        metrics.PairedEvaluator(("lpips",))
    with pytest.raises(ValueError):
        metrics.PairedEvaluator(("ssim", "lpips"), lpips=None)
    with pytest.raises(ValueError):
        metrics.PerceptualMetric(None)
    assert metrics.PairedEvaluator.__init__.__defaults__[0] == ("ssim", "psnr", "sspe")      # the default set is unchanged
    m = lpips_net.LPIPS(*synthetic.lpips_state_dicts(5))
    assert metrics.PerceptualMetric(m).quality() == "lower"
    assert metrics.PairedEvaluator(("ssim", "lpips"), lpips=m).metrics == ("ssim", "lpips")  # constructing launches nothing
    x = torch.zeros((1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="contiguous float32 CUDA"):
        m(x, x)                                                                              # no CPU fallback


def test_refusals_before_any_hip_call():
    lib = _lib.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    h = ctypes.c_void_p()
    # create / handle entries
    assert lib.lwg_lpips_create(None, 1, 64, 64) == INVALID and b"NULL" in lib.lwg_last_error()
    for pairs, mh, mw in ((0, 64, 64), (-1, 64, 64), (1, 30, 64), (1, 64, 30), (1, 0, 0)):
        assert lib.lwg_lpips_create(ctypes.byref(h), pairs, mh, mw) == INVALID and h.value is None, (pairs, mh, mw)
    assert lib.lwg_lpips_weight_floats(None) == 0
    assert lib.lwg_lpips_set_weights(None, p, 16) == INVALID
    assert lib.lwg_lpips_forward(None, p, p, 1, 64, 64, 0, p, None, None) == INVALID and b"NULL" in lib.lwg_last_error()
    lib.lwg_lpips_destroy(None)
    # conv (x, N, H, W, Cin, w, bias, Cout, k, stride, pad, relu, input_mode, y, stream)
    conv = lambda x=p, n=2, hh=7, ww=7, cin=64, w=p, b=p, cout=192, k=5, s=1, pad=2, relu=1, mode=-1, y=p: lib.lwg_lpips_conv(
        x, n, hh, ww, cin, w, b, cout, k, s, pad, relu, mode, y, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        assert conv(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(n=0), dict(hh=0), dict(ww=-1), dict(cin=0), dict(cout=0), dict(relu=2), dict(mode=3), dict(mode=0),   # mode 0: Cin 64
               dict(w=odd), dict(x=odd), dict(x=ctypes.c_void_p(4098), cin=3, mode=1, k=11, s=4, pad=2, hh=31, ww=31, cout=64)):
        assert conv(**kw) == INVALID, kw
    for k, s, pad in ((7, 2, 3), (1, 1, 0), (3, 2, 1), (11, 4, 0), (5, 1, 1), (3, 1, 0), (11, 1, 2)):
        assert conv(k=k, s=s, pad=pad) == UNSUPPORTED and b"(11,4,2)" in lib.lwg_last_error(), (k, s, pad)
    assert conv(cout=96) == UNSUPPORTED and b"multiple of 64" in lib.lwg_last_error()
    assert conv(cin=3, mode=0, k=11, s=4, pad=2, hh=6, ww=31, cout=64) == INVALID and b"empty" in lib.lwg_last_error()
    # maxpool (x, N, H, W, C, y, stream)
    pool = lambda x=p, n=2, hh=7, ww=7, c=64, y=p: lib.lwg_lpips_maxpool(x, n, hh, ww, c, y, None)
    for kw in (dict(x=None), dict(y=None)):
        assert pool(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(n=0), dict(hh=2), dict(ww=2), dict(c=0), dict(x=odd), dict(y=odd)):
        assert pool(**kw) == INVALID, kw
    assert pool(c=66) == UNSUPPORTED
    # layer_distance (f0, f1, n, P, C, w, out, stream)
    dist = lambda f0=p, f1=p, n=3, P=9, C=384, w=p, out=p: lib.lwg_lpips_layer_distance(f0, f1, n, P, C, w, out, None)
    for kw in (dict(f0=None), dict(f1=None), dict(w=None), dict(out=None)):
        assert dist(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(n=0), dict(P=0), dict(C=0), dict(f0=odd), dict(f1=odd), dict(w=odd), dict(out=odd)):
        assert dist(**kw) == INVALID, kw
    assert dist(C=62) == UNSUPPORTED
