"""CPU: the host side of FID and Inception Score -- pack_weights' refusals and its BatchNorm fold, the metric functions of
utils/metrics.py against the reference's own outputs (tests/golden/fid_reference.npz: fid_score_func, calculate_frechet_distance
and is_score_func of thirdparty/his_evaluators/.../metrics/metrics.py run on small feature sets), the restatement in
tests/inception_ref.py against the same file, and every refusal of the lwg_inception_* entry points that comes before the first
HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from impersonator_amd import _lib
from impersonator_amd.networks import inception as inception_net
from impersonator_amd.utils import metrics, synthetic
from tests import inception_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def sd():
    return synthetic.inception_state_dict(3)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "fid_reference.npz"))


# ------------------------------------------------------------------------------------------------ weights
def test_the_table_is_the_network_of_the_restated_module(sd):
    own = inception_ref.InceptionFeatures().state_dict()
    assert len(inception_net.CONVS) == 94
    assert sorted(own) == sorted(sd)                                            # the seeded weights carry exactly its keys
    for name, cin, cout, k, _, _ in inception_net.CONVS:
        assert tuple(own[name + ".conv.weight"].shape) == (cout, cin, k[0], k[1]), name
    assert [n for n, *_ in inception_net.CONVS] == [k[:-len(".conv.weight")] for k in own if k.endswith(".conv.weight")]   # definition order
    assert inception_net.STAGES == inception_ref.STAGES
    assert _lib.load().lwg_inception_weight_floats() == sum(c[1] * c[2] * c[3][0] * c[3][1] + 2 * c[2] for c in inception_net.CONVS)


def test_pack_weights_layout_and_ignored_keys(sd):
    blob = inception_net.pack_weights(sd)
    assert blob.dtype == torch.float32 and blob.numel() == _lib.load().lwg_inception_weight_floats()
    off = 0
    for name, cin, cout, (kh, kw), _, _ in inception_net.CONVS[:12] + inception_net.CONVS[-3:]:
        if name == inception_net.CONVS[-3][0]:
            off = blob.numel() - sum(c[1] * c[2] * c[3][0] * c[3][1] + 2 * c[2] for c in inception_net.CONVS[-3:])
        w = sd[name + ".conv.weight"]
        block = blob[off:off + w.size].numpy().reshape(kh, kw, cin, cout)         # [kh][kw][ci][co]
        assert np.array_equal(block, w.transpose(2, 3, 1, 0)), name
        assert block[kh - 1, 0, cin - 1, 2] == w[2, cin - 1, kh - 1, 0]
        off += w.size + 2 * cout
    extra = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    extra["fc.weight"], extra["AuxLogits.conv0.conv.weight"] = torch.zeros(1000, 2048), torch.zeros(128, 768, 1, 1)
    assert torch.equal(inception_net.pack_weights(extra), blob)


def test_pack_weights_refuses_by_name(sd):
    for drop in ("Mixed_6c.branch7x7dbl_3.conv.weight", "Conv2d_1a_3x3.bn.running_var", "Mixed_7c.branch_pool.bn.bias"):
        with pytest.raises(KeyError, match=drop.replace(".", r"\.")):
            inception_net.pack_weights({k: v for k, v in sd.items() if k != drop})
    bad = dict(sd)
    bad["Mixed_6b.branch7x7_2.conv.weight"] = np.zeros((128, 128, 7, 1), np.float32)      # (7,1) where (1,7) belongs
    with pytest.raises(ValueError, match=r"Mixed_6b\.branch7x7_2\.conv\.weight"):
        inception_net.pack_weights(bad)
    bad = dict(sd)
    bad["Mixed_5b.branch5x5_1.bn.weight"] = np.zeros((64,), np.float32)                   # 48 channels
    with pytest.raises(ValueError, match=r"Mixed_5b\.branch5x5_1\.bn\.weight"):
        inception_net.pack_weights(bad)
    bad = dict(sd)
    bad["Conv2d_3b_1x1.bn.running_mean"] = np.zeros((80,), np.int64)
    with pytest.raises(TypeError, match=r"Conv2d_3b_1x1\.bn\.running_mean"):
        inception_net.pack_weights(bad)
    with pytest.raises(KeyError):
        inception_net.InceptionV3({})


def test_the_fold_is_batchnorm_eval_in_fp64():
    rs = np.random.RandomState(4)
    c = 80
    bn = torch.nn.BatchNorm2d(c, eps=1e-3).double().eval()
    params = {"weight": rs.uniform(0.5, 1.5, c), "bias": rs.normal(0, 0.1, c), "running_mean": rs.normal(0, 0.2, c),
              "running_var": rs.uniform(0.5, 2.0, c)}
    params = {k: v.astype(np.float32) for k, v in params.items()}
    bn.load_state_dict({**{k: torch.from_numpy(v).double() for k, v in params.items()}, "num_batches_tracked": torch.tensor(0)})
    x = torch.from_numpy(rs.standard_normal((2, c, 3, 5)))
    with torch.no_grad():
        want = bn(x)
    scale, shift = inception_net.fold_bn(params["weight"], params["bias"], params["running_mean"], params["running_var"])
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    # the fp64 fold itself, before its one rounding, is BatchNorm to fp64 rounding
    s64 = params["weight"].astype(np.float64) / np.sqrt(params["running_var"].astype(np.float64) + 1e-3)
    t64 = params["bias"].astype(np.float64) - params["running_mean"].astype(np.float64) * s64
    got = x * torch.from_numpy(s64).view(1, c, 1, 1) + torch.from_numpy(t64).view(1, c, 1, 1)
    err = float((got - want).abs().max())
    print("fp64 fold vs BatchNorm2d.eval(): max |difference| %.3g" % err)
    assert err <= 1e-14
    assert np.array_equal(scale.numpy(), s64.astype(np.float32)) and np.array_equal(shift.numpy(), t64.astype(np.float32))
    assert float(np.abs(s64 - 1).min()) > 1e-4                                    # not an identity BatchNorm


def test_seeded_weights_have_a_non_trivial_batchnorm(sd):
    for name in ("Conv2d_1a_3x3", "Mixed_7c.branch_pool"):
        for key, trivial in (("weight", 1.0), ("bias", 0.0), ("running_mean", 0.0), ("running_var", 1.0)):
            assert float(np.abs(sd["%s.bn.%s" % (name, key)] - trivial).mean()) > 0.05
    again = synthetic.inception_state_dict(3)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    assert not np.array_equal(sd["Conv2d_1a_3x3.conv.weight"], synthetic.inception_state_dict(4)["Conv2d_1a_3x3.conv.weight"])


# ------------------------------------------------------------------------------------------------ the metric functions
def _rel(a, b):
    return abs(a - b) / abs(b)


def test_fid_against_the_reference_well_conditioned(ref):
    assert str(ref["source"]) == "reference"
    a, b = ref["well_a"], ref["well_b"]
    for fn in (metrics.fid_from_features, inception_ref.fid):
        got = fn(a, b)
        print("%s d=64 N=256: %.15g, the reference's fid_score_func %.15g, rel %.3g" % (fn.__module__, got, float(ref["well_fid"]),
                                                                                         _rel(got, float(ref["well_fid"]))))
        assert _rel(got, float(ref["well_fid"])) <= 1e-9
    for fn in (metrics.frechet_distance, inception_ref.frechet_distance):
        got = fn(ref["well_mu1"], ref["well_s1"], ref["well_mu2"], ref["well_s2"])
        assert _rel(got, float(ref["well_frechet"])) <= 1e-9


def test_fid_against_the_reference_rank_deficient(ref):
    """16 samples in 64 dimensions: both covariances have rank 15, their product is singular and scipy's sqrtm returns a complex
    matrix (the path with the imaginary-part check).  The square root of a singular matrix is itself only good to about
    sqrt(eps) = 1.5e-8 relative -- its error is not a rounding error of these functions -- so two runs that differ in anything
    (a thread count, a LAPACK build) may differ by that much: the bound here is 1e-6, not 1e-9."""
    from scipy import linalg
    root, _ = linalg.sqrtm(ref["rank_s1"].dot(ref["rank_s2"]), disp=False)
    assert np.iscomplexobj(root) and np.linalg.matrix_rank(ref["rank_s1"]) == 15
    for fn in (metrics.fid_from_features, inception_ref.fid):
        got = fn(ref["rank_a"], ref["rank_b"])
        print("%s d=64 N=16: %.15g, the reference's fid_score_func %.15g, rel %.3g" % (fn.__module__, got, float(ref["rank_fid"]),
                                                                                        _rel(got, float(ref["rank_fid"]))))
        assert _rel(got, float(ref["rank_fid"])) <= 1e-6
    got = metrics.frechet_distance(ref["rank_mu1"], ref["rank_s1"], ref["rank_mu2"], ref["rank_s2"])
    assert _rel(got, float(ref["rank_frechet"])) <= 1e-6


def test_inception_score_against_the_reference_with_a_short_last_batch(ref):
    f = ref["is_features"]
    assert f.shape[0] == 70 and len(ref["is_batch_scores"]) == 3                  # 32 + 32 + 6
    for fn in (metrics.inception_score, inception_ref.inception_score):
        mean, std = fn(f, 32)
        print("%s: IS %.15g +- %.15g, the reference's %.15g +- %.15g" % (fn.__module__, mean, std, float(ref["is_mean"]), float(ref["is_std"])))
        assert _rel(mean, float(ref["is_mean"])) <= 1e-9 and _rel(std, float(ref["is_std"])) <= 1e-9
    one, zero = metrics.inception_score(f[:6], 32)
    assert one > 1.0 and zero == 0.0                                              # a single batch: std 0
    assert _rel(metrics.inception_score(f[64:], 32)[0], float(ref["is_batch_scores"][2])) <= 1e-9
    # a softmax over the features, not over logits of a classifier: shifting every feature of a row changes nothing
    assert _rel(metrics.inception_score(f.astype(np.float64) + 5.0, 32)[0], mean) <= 1e-9


def test_a_set_against_itself_and_empty_sets(ref):
    a = ref["well_a"]
    trace = float(np.trace(np.cov(a, rowvar=False)))
    same = metrics.fid_from_features(a, a.copy())
    print("FID of a set against itself: %.3g (trace %.3g)" % (same, trace))
    assert abs(same) <= 1e-6 * trace
    r = ref["rank_a"]
    assert abs(metrics.fid_from_features(r, r)) <= 1e-6 * float(np.trace(np.cov(r, rowvar=False)))
    empty = np.zeros((0, 64))
    assert metrics.fid_from_features(empty, a) == 0 and metrics.fid_from_features(a, empty) == 0 and metrics.fid_from_features([], []) == 0
    assert metrics.inception_score(empty) == (0.0, 0.0)
    with pytest.raises(ValueError):
        metrics.frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    with pytest.raises(ValueError, match="Imaginary"):
        metrics.frechet_distance(np.zeros(2), np.diag([-1.0, 1.0]), np.zeros(2), np.eye(2))   # sqrtm has i on its diagonal


# ------------------------------------------------------------------------------------------------ the surface, without a device
def test_metric_classes_need_a_model_and_cuda_tensors(sd):
    for cls in (metrics.FIDMetric, metrics.InceptionScoreMetric, metrics.SetEvaluator):
        with pytest.raises(ValueError):
            cls(None)
    net = inception_net.InceptionV3(sd)                                            # constructing launches nothing
    assert metrics.FIDMetric(net).quality() == "lower" and metrics.InceptionScoreMetric(net).quality() == "higher"
    ev = metrics.SetEvaluator(net, mode=2)
    assert len(ev) == 0 and ev.result() == {"frames": 0}
    with pytest.raises(ValueError):
        metrics.SetEvaluator(net, mode=3)
    with pytest.raises(RuntimeError, match="contiguous float32 CUDA"):
        net(torch.zeros((1, 3, 96, 96)))                                           # no CPU fallback
    assert metrics.PairedEvaluator.METRICS == ("ssim", "psnr", "sspe", "lpips")     # the paired evaluator is as it was
    assert [s[:2] for s in inception_net.stage_shapes(299, 299)][::3] == [(149, 149), (73, 73), (35, 35), (35, 35), (17, 17), (8, 8)]
    assert inception_net.stage_shapes(107, 91)[-1] == (2, 1, 2048) and inception_net.stage_shapes(75, 75)[-1] == (1, 1, 2048)


def test_refusals_before_any_hip_call():
    lib = _lib.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    h = ctypes.c_void_p()
    assert lib.lwg_inception_create(None, 1, 64, 64) == INVALID and b"NULL" in lib.lwg_last_error()
    for images, mh, mw in ((0, 64, 64), (-1, 64, 64), (1, 0, 64), (1, 64, 9000)):
        assert lib.lwg_inception_create(ctypes.byref(h), images, mh, mw) == INVALID and h.value is None, (images, mh, mw)
    assert lib.lwg_inception_set_weights(None, p, 16) == INVALID
    assert lib.lwg_inception_forward(None, p, 1, 96, 96, 0, 0, 0, p, -1, None, None) == INVALID and b"NULL" in lib.lwg_last_error()
    lib.lwg_inception_destroy(None)
    # conv (x, N, H, W, Cin, w, scale, shift, Cout, kh, kw, stride, ph, pw, relu, input_mode, y, y_pitch, y_offset, stream)
    conv = lambda x=p, n=2, hh=5, ww=9, cin=16, w=p, sc=p, sh=p, cout=48, kh=1, kw=7, s=1, ph=0, pw=3, relu=1, mode=-1, y=p, pitch=48, off=0: \
        lib.lwg_inception_conv(x, n, hh, ww, cin, w, sc, sh, cout, kh, kw, s, ph, pw, relu, mode, y, pitch, off, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        assert conv(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(n=0), dict(hh=0), dict(ww=-1), dict(cin=0), dict(cout=0), dict(relu=2), dict(mode=3), dict(mode=0), dict(kh=0), dict(kw=12),
               dict(s=0), dict(s=5), dict(ph=1), dict(pw=7), dict(pw=-1), dict(pitch=40), dict(off=4), dict(off=-4), dict(w=odd), dict(x=odd),
               dict(sc=ctypes.c_void_p(4098)), dict(kh=7, ph=3, hh=5, kw=7, pw=0, ww=5)):
        assert conv(**kw) == INVALID, kw
    assert b"empty" in lib.lwg_last_error()
    assert conv(cin=18) == UNSUPPORTED and conv(cout=46, pitch=46) == UNSUPPORTED
    # pools
    mp = lambda x=p, n=2, hh=7, ww=7, c=64, y=p, pitch=64, off=0: lib.lwg_inception_maxpool(x, n, hh, ww, c, y, pitch, off, None)
    for kw in (dict(x=None), dict(y=None), dict(n=0), dict(hh=2), dict(ww=2), dict(c=0), dict(x=odd), dict(y=odd), dict(pitch=32), dict(off=4)):
        assert mp(**kw) == INVALID, kw
    assert mp(c=66, pitch=66) == UNSUPPORTED and mp(pitch=130, off=2) == UNSUPPORTED
    ap = lambda x=p, n=2, hh=7, ww=7, c=64, y=p: lib.lwg_inception_avgpool(x, n, hh, ww, c, y, None)
    for kw in (dict(x=None), dict(y=None), dict(n=0), dict(hh=0), dict(c=0), dict(x=odd), dict(y=odd)):
        assert ap(**kw) == INVALID, kw
    assert ap(c=66) == UNSUPPORTED
    gp = lambda x=p, n=2, P=4, c=64, y=p: lib.lwg_inception_global_pool(x, n, P, c, y, None)
    for kw in (dict(x=None), dict(y=None), dict(n=0), dict(P=0), dict(c=0), dict(x=ctypes.c_void_p(4098))):
        assert gp(**kw) == INVALID, kw
