"""GPU: the paired-evaluation kernels (csrc/eval.hip) and their Python surface (utils/metrics.py) against the numpy fp64
statement in tests/metrics_ref.py, at the smallest shapes that can still go wrong: one window, one window row / column, ragged
16x16 tiles in both directions, and 256x256 once.

Bounds.  |mssim - ref| <= 1e-10: two fp64 formulations of the same moments differ by <= 3e-14 (tests/test_metrics_host.py
prints it), float32 moments by ~1e-6 on the near-flat pair, so the bound separates the two with margin on both sides.  mse is a
sum of exact fp64 squares in another order: 1e-12 relative.  ref_min / ref_max are float32 values: exact.  resize: 1e-6 against
torch's CPU F.interpolate (a handful of float32 roundings).  SSPE: the rule of tests/test_gpu_hmr.py -- the device may be at
most 4 x as far from the fp64 route as torch's own float32 route is.
Every test prints the figures it compares before it asserts (run with -s)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from impersonator_amd import _lib
from impersonator_amd.networks import batch_smpl
from impersonator_amd.networks import hmr as hmr_net
from impersonator_amd.utils import metrics, synthetic
from tests import metrics_ref as ref

pytestmark = pytest.mark.gpu

SSIM_TOL, MSE_RTOL = 1e-10, 1e-12


def _noise(seed, shape, lo=-1.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(pred, gt, mode=0, what=""):
    """device pair_stats == the restatement, within the module's bounds; returns the device rows"""
    got = metrics.pair_stats(_dev(pred), _dev(gt), mode=mode).cpu().numpy()
    want = ref.pair_stats(pred, gt, mode)
    assert got.shape == want.shape == (len(pred), 4) and got.dtype == np.float64
    d_ssim = float(np.abs(got[:, 0] - want[:, 0]).max())
    d_mse = float((np.abs(got[:, 1] - want[:, 1]) / np.maximum(want[:, 1], 1e-300)).max())
    print("%s %s mode %d: mssim %s, |d mssim| %.3g, mse rel %.3g, ref range [%g, %g]"
          % (what, tuple(pred.shape), mode, np.array2string(got[:, 0], precision=12), d_ssim, d_mse, got[:, 2].min(), got[:, 3].max()))
    assert d_ssim <= SSIM_TOL
    assert d_mse <= MSE_RTOL
    assert np.array_equal(got[:, 2:], want[:, 2:])
    return got


# ------------------------------------------------------------------------------------------------ pair_stats
@pytest.mark.parametrize("h,w", [(7, 7), (8, 9), (7, 40), (40, 7), (37, 45)])
def test_pair_stats_noise_at_the_small_shapes(h, w):
    _check(_noise(h * 100 + w, (2, 3, h, w)), _noise(h * 100 + w + 1, (2, 3, h, w)), what="noise")
    close = _noise(h + w, (1, 3, h, w))
    _check(np.clip(close + 0.05 * _noise(h + w + 1, close.shape), -1, 1).astype(np.float32), close, what="noisy copy")


def test_pair_stats_smooth_images_ragged_tiles():
    a = synthetic.smooth_image(31, (2, 3, 37, 45))
    b = np.clip(a + 0.02 * synthetic.smooth_image(32, (2, 3, 37, 45)), -1, 1).astype(np.float32)
    _check(a, b, what="smooth")


def test_pair_stats_near_flat_bright_pair_needs_fp64_moments():
    a, b = ref.near_flat_pair(37, 45)
    got = _check(a, b, what="near-flat")
    f32 = ref.ssim(a[0], b[0], channel=ref.ssim_channel_float32)
    print("near-flat: float32 moments would give %.12g, off by %.3g" % (f32, abs(f32 - got[0, 0])))
    assert abs(f32 - got[0, 0]) > 100 * SSIM_TOL          # the case does separate the two arithmetics


def test_pair_stats_256_once():
    a = np.concatenate([synthetic.smooth_image(41, (1, 3, 256, 256)), _noise(42, (1, 3, 256, 256)), ref.near_flat_pair(256, 256)[0]])
    b = np.concatenate([np.clip(a[:1] + 1e-3 * _noise(43, (1, 3, 256, 256)), -1, 1).astype(np.float32), _noise(44, (1, 3, 256, 256)),
                        ref.near_flat_pair(256, 256)[1]])
    _check(a, b, what="256x256 smooth / noise / near-flat")


@pytest.mark.parametrize("corner", ["first", "last"])
def test_every_pixel_belongs_to_exactly_one_tile(corner):
    """a difference confined to one corner pixel of one channel: mse = d^2 / (3HW), and SSIM falls below 1 only through the one
    window that holds the pixel"""
    h, w = 37, 45
    gt = synthetic.smooth_image(51, (1, 3, h, w))
    pred = gt.copy()
    y, x = (0, 0) if corner == "first" else (h - 1, w - 1)
    pred[0, 1, y, x] += np.float32(0.25)
    d = float(pred[0, 1, y, x]) - float(gt[0, 1, y, x])
    got = _check(pred, gt, what="corner " + corner)
    want_mse = d * d / (3 * h * w)
    ys, xs = (slice(0, 7), slice(0, 7)) if corner == "first" else (slice(h - 7, h), slice(w - 7, w))
    s_one = ref.ssim_channel(pred[0, 1, ys, xs], gt[0, 1, ys, xs])          # the single window over that pixel
    want_ssim = 1.0 - (1.0 - s_one) / (3 * (h - 6) * (w - 6))
    print("corner %s: mse %.17g (want %.17g), mssim %.17g (want %.17g)" % (corner, got[0, 1], want_mse, got[0, 0], want_ssim))
    assert abs(got[0, 1] - want_mse) <= MSE_RTOL * want_mse
    assert got[0, 0] < 1.0 and abs(got[0, 0] - want_ssim) <= SSIM_TOL


# ------------------------------------------------------------------------------------------------ modes and PSNR
def test_mode_1_maps_unit_images_like_the_references_preprocess():
    a, b = _noise(61, (2, 3, 37, 45), 0, 1), _noise(62, (2, 3, 37, 45), 0, 1)
    got = _check(a, b, mode=1, what="unit")
    assert got[:, 2].min() >= -1 and got[:, 3].max() <= 1 and got[:, 2].min() < 0


def test_mode_2_quantises_through_eight_bits_steps_and_ends_included():
    a, b = _noise(63, (2, 3, 37, 45)), _noise(64, (2, 3, 37, 45))
    # frame 1: values sitting exactly on the quantiser's steps (what the loader hands back for every byte), and +-1
    k = np.arange(37 * 45, dtype=np.float32) % 256
    grid = ((k / np.float32(255)) * np.float32(2)) - np.float32(1)
    a[1, :] = grid.reshape(37, 45)
    b[1, :] = grid[::-1].reshape(37, 45)
    a[1, 0, 0, :4] = [-1.0, 1.0, 1.0, -1.0]
    b[1, 0, 0, :4] = [1.0, -1.0, 1.0, -1.0]
    got = _check(a, b, mode=2, what="quantize")
    assert got[1, 2] == -1.0 and got[1, 3] == 1.0
    same = metrics.pair_stats(_dev(a), _dev(ref.map_pixels(a, 2)), mode=2).cpu().numpy()     # the mapped image re-quantised
    want = ref.pair_stats(a, ref.map_pixels(a, 2), 2)
    assert np.abs(same[:, 0] - want[:, 0]).max() <= SSIM_TOL and np.allclose(same[:, 1], want[:, 1], rtol=MSE_RTOL, atol=0)


def test_psnr_data_range_inf_and_the_out_of_range_reference():
    pos = _noise(71, (1, 3, 16, 16), 0, 1)
    neg = _noise(72, (1, 3, 16, 16), -1, 1)
    pred_pos = np.clip(pos + 0.01 * _noise(73, pos.shape), -1, 1).astype(np.float32)
    pred_neg = np.clip(neg + 0.01 * _noise(74, neg.shape), -1, 1).astype(np.float32)
    stats = metrics.pair_stats(_dev(np.concatenate([pred_pos, pred_neg, neg])), _dev(np.concatenate([pos, neg, neg]))).cpu().numpy()
    got = metrics.psnr_from_stats(stats)
    want = [ref.psnr(pred_pos[0], pos[0]), ref.psnr(pred_neg[0], neg[0])]
    print("psnr: device", got, "reference", want)
    assert stats[0, 2] >= 0 and stats[1, 2] < 0
    assert abs(got[0] - want[0]) <= 1e-9 and abs(got[1] - want[1]) <= 1e-9
    assert abs(got[0] - 10 * np.log10(1 / stats[0, 1])) <= 1e-12 and abs(got[1] - 10 * np.log10(4 / stats[1, 1])) <= 1e-12
    assert got[2] == float("inf") and stats[2, 0] == 1.0 and stats[2, 1] == 0.0
    # the reference's classes take [0,1] images
    u_pred, u_gt = _dev((pred_neg + 1) / 2), _dev((neg + 1) / 2)
    m = ref.map_pixels
    assert abs(metrics.SSIMMetric().calculate_score(u_pred, u_gt) - ref.ssim(m((pred_neg[0] + 1) / 2, 1), m((neg[0] + 1) / 2, 1))) <= SSIM_TOL
    assert abs(metrics.PSNRMetric().calculate_score(u_pred, u_gt) - ref.psnr(m((pred_neg[0] + 1) / 2, 1), m((neg[0] + 1) / 2, 1))) <= 1e-9
    assert metrics.SSIMMetric().quality() == "higher" and metrics.PSNRMetric().quality() == "higher"
    bad = neg.copy()
    bad[0, 2, 5, 5] = 1.5
    ev = metrics.PairedEvaluator(("psnr",))
    ev.update(_dev(pred_neg), _dev(bad))              # launching is fine ...
    with pytest.raises(ValueError):
        ev.result()                                   # ... reading the numbers raises, as scikit-image does


# ------------------------------------------------------------------------------------------------ invariance
def test_batch_invariance_and_repeatability_bit_for_bit():
    a = np.concatenate([_noise(81, (3, 3, 37, 45)), synthetic.smooth_image(82, (2, 3, 37, 45))])
    b = np.concatenate([_noise(83, (3, 3, 37, 45)), synthetic.smooth_image(84, (2, 3, 37, 45))])
    da, db = _dev(a), _dev(b)
    five = metrics.pair_stats(da, db)
    again = metrics.pair_stats(da, db)
    assert torch.equal(five, again)
    for i in range(5):
        alone = metrics.pair_stats(da[i:i + 1].contiguous(), db[i:i + 1].contiguous())
        assert torch.equal(alone[0], five[i]), i


def test_paired_evaluator_ragged_updates_equal_single_calls():
    a, b = _dev(_noise(91, (9, 3, 24, 24))), _dev(_noise(92, (9, 3, 24, 24)))
    ev = metrics.PairedEvaluator(("ssim", "psnr"))
    for s, e in ((0, 4), (4, 8), (8, 9)):
        ev.update(a[s:e], b[s:e])
    out = ev.result()
    single = torch.cat([metrics.pair_stats(a[i:i + 1], b[i:i + 1]) for i in range(9)]).cpu().numpy()
    assert out["frames"] == len(ev) == 9
    assert np.array_equal(out["per_frame"]["ssim"], single[:, 0])
    assert np.array_equal(out["per_frame"]["psnr"], metrics.psnr_from_stats(single))
    assert out["ssim"] == float(np.mean(single[:, 0])) and out["psnr"] == float(np.mean(metrics.psnr_from_stats(single)))
    # the table grows without losing rows
    many = metrics.PairedEvaluator(("ssim",))
    for _ in range(9):
        many.update(a, b)
    assert np.array_equal(many.result()["per_frame"]["ssim"], np.tile(single[:, 0], 9))
    with pytest.raises(ValueError):
        metrics.PairedEvaluator(("ssim", "sspe"))
    with pytest.raises(ValueError):
        metrics.PairedEvaluator(("lpips",))


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("src,dst", [((256, 256), (224, 224)), ((7, 9), (4, 5)), ((3, 3), (8, 8)), ((6, 6), (6, 6))])
def test_resize_bilinear_is_f_interpolate(src, dst):
    x = _noise(101, (2, 3) + src)
    got = metrics.resize_bilinear(_dev(x), dst).cpu().numpy()
    want = ref.resize_bilinear_ref(x, dst)
    err = float(np.abs(got - want).max())
    print("resize %s -> %s: max |device - F.interpolate| %.3g, device vs the restated arithmetic %.3g"
          % (src, dst, err, float(np.abs(got - ref.resize_bilinear_restated(x, dst)).max())))
    assert got.shape == want.shape and err <= 1e-6
    if src == dst:
        assert np.array_equal(got, x)


# ------------------------------------------------------------------------------------------------ SSPE
def test_sspe_terms_against_fp64():
    a, b = np.random.RandomState(111).standard_normal((5, 85)).astype(np.float32), \
        np.random.RandomState(112).standard_normal((5, 85)).astype(np.float32)
    got = metrics.sspe_terms(_dev(a), _dev(b)).cpu().numpy()
    want = ref.sspe_terms(a, b)
    rel = float((np.abs(got - want) / want).max())
    print("sspe_terms: worst relative error %.3g" % rel)
    assert got.shape == (5, 3) and rel <= 1e-12
    assert got[0, 2] > got[0, 0] > 0          # the "pose" term holds the scale term's value again


def _reduced_regressor():
    m = hmr_net.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0), num_blocks=(3, 2, 2, 2), max_batch=8).eval()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.hmr_state_dict(1, m.resnet.num_blocks).items()}
    for k, v in m.smpl.state_dict().items():
        sd["smpl." + k] = v.cpu()
    m.load_state_dict(sd)
    return m


def test_scale_shape_pose_error_against_the_fp64_route():
    """three 256x256 pairs in [0,1]: 2x-1, F.interpolate to 224, the reduced regressor's tensor-op forward, the three sums.
    Oracle: that route on the CPU with the regressor in fp64; yardstick: the same route in torch CPU float32."""
    model = _reduced_regressor()
    pred = (synthetic.smooth_image(121, (3, 3, 256, 256)) + 1) / 2
    gt = (synthetic.smooth_image(122, (3, 3, 256, 256)) + 1) / 2
    prep = lambda x: F.interpolate(torch.from_numpy(x) * 2 - 1, (224, 224), mode="bilinear", align_corners=False)
    with torch.no_grad():
        p32, g32 = model.forward_ops(prep(pred)).numpy(), model.forward_ops(prep(gt)).numpy()
        model.resnet.double(), model.regressor.double()
        p64, g64 = model.forward_ops(prep(pred).double()).numpy(), model.forward_ops(prep(gt).double()).numpy()
        model.resnet.float(), model.regressor.float()
    want_terms, want = ref.sspe_terms(p64, g64), ref.sspe(p64, g64)
    cpu_terms, cpu = ref.sspe_terms(p32, g32), ref.sspe(p32, g32)

    model.cuda()
    metric = metrics.ScaleShapePoseError(model)
    dp, dg = _dev(pred), _dev(gt)
    got_terms = metric.terms(dp, dg).cpu().numpy()
    got = metric.calculate_score(dp, dg)
    e_dev, e_ref = float(np.abs(got_terms - want_terms).max()), float(np.abs(cpu_terms - want_terms).max())
    s_dev, s_ref = abs(got - want), abs(cpu - want)
    print("sspe %.9g (fp64 route %.9g): per-frame terms, device error %.3g, torch fp32 %.3g, ratio %.3g; score, device error %.3g, "
          "torch fp32 %.3g" % (got, want, e_dev, e_ref, e_dev / e_ref, s_dev, s_ref))
    assert metric.quality() == "lower" and want > 1e-3
    assert e_dev <= 4 * e_ref
    # the evaluator's rows are the metric's rows (frames in [-1,1]: mode 0 hands them to the regressor as they are)
    ev = metrics.PairedEvaluator(("sspe",), hmr=model)
    dp2, dg2 = _dev(pred * 2 - 1), _dev(gt * 2 - 1)
    ev.update(dp2[:2], dg2[:2])
    ev.update(dp2[2:], dg2[2:])
    out = ev.result()
    direct = metrics.ScaleShapePoseError(model, unit=False).terms(dp2, dg2).cpu().numpy()
    assert np.array_equal(out["per_frame"]["sspe"], direct.sum(1)) and out["frames"] == 3
    model.release()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    small = torch.zeros((1, 3, 6, 9), device="cuda")
    with pytest.raises(_lib.LwgError) as e:
        metrics.pair_stats(small, small)
    assert e.value.code == -2 and "LWG_ERR_UNSUPPORTED" in str(e.value)
    ok = torch.zeros((1, 3, 8, 8), device="cuda")
    with pytest.raises(RuntimeError, match="contiguous float32 CUDA"):
        metrics.pair_stats(ok.cpu(), ok.cpu())
    wide = torch.zeros((1, 3, 8, 16), device="cuda")
    with pytest.raises(RuntimeError, match="contiguous float32 CUDA"):
        metrics.pair_stats(wide[..., ::2], ok)
    with pytest.raises(RuntimeError, match="contiguous float32 CUDA"):
        metrics.resize_bilinear(ok.double(), (4, 4))
    with pytest.raises(RuntimeError, match="contiguous float32 CUDA"):
        metrics.sspe_terms(torch.zeros((2, 85)), torch.zeros((2, 85)))
    with pytest.raises(ValueError):
        metrics.pair_stats(ok, ok, mode=3)
    lib = _lib.load()
    need = lib.lwg_eval_workspace_bytes(1, 8, 8)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    stats = torch.full((1, 4), 7.0, dtype=torch.float64, device="cuda")
    rc = lib.lwg_eval_pair_stats(_lib.ptr(ok), _lib.ptr(ok), 1, 8, 8, 0, _lib.ptr(stats), _lib.ptr(ws), ctypes.c_size_t(need - 1),
                                 _lib.stream_ptr())
    assert rc == -3 and b"workspace" in lib.lwg_last_error()
    torch.cuda.synchronize()
    assert bool((stats == 7.0).all())                  # refused before anything was launched
