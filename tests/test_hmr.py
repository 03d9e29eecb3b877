"""CPU checks of the HMR regressor (impersonator_amd/networks/hmr.py, csrc/hmr.hip): the module surface and the tensor-op
forward against the LIVE reference (networks/hmr.py; skipped where the reference tree is absent), the golden file, the fp64
BatchNorm fold, the light class, and the argument validation of every lwg_hmr_* entry point without a device."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from impersonator_amd import _lib
from impersonator_amd.networks import batch_smpl
from impersonator_amd.networks import hmr as hmr_net
from impersonator_amd.utils import synthetic
from oracle import reference_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hmr_golden.npz")
needs_reference = pytest.mark.skipif(not reference_loader.available(), reason="/root/reference not present")


def _maker():
    spec = importlib.util.spec_from_file_location("make_hmr_golden", os.path.join(ROOT, "tests", "golden", "make_hmr_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def full():
    m = hmr_net.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0)).eval()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.hmr_state_dict(0).items()}
    for k, v in m.smpl.state_dict().items():
        sd["smpl." + k] = v
    m.load_state_dict(sd)
    return m


@needs_reference
def test_state_dict_keys_and_shapes_equal_the_reference(full):
    """`resnet.*` and `regressor.*` against the reference's own modules, key by key in order; `smpl.*` (the reference builds it
    from a pickle this tree does not hold) against the six buffers networks/batch_smpl.py:251-283 registers."""
    maker = _maker()
    ref, _ = maker.reference_module(0)
    theirs = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    mine = [(k, tuple(v.shape)) for k, v in full.state_dict().items()]
    assert [e for e in mine if not e[0].startswith("smpl.")] == theirs
    assert [k for k, _ in mine if k.startswith("smpl.")] == ["smpl." + k for k in (
        "v_template", "shapedirs", "J_regressor", "posedirs", "weights", "joint_regressor")]
    # the reference's attribute order: resnet, smpl, regressor (hmr.py:264-273)
    heads = [k.split(".")[0] for k, _ in mine]
    assert heads.index("smpl") > heads.index("resnet") and heads.index("regressor") > heads.index("smpl")
    for k in ("resnet.conv1.weight", "resnet.layer1.0.bn1.running_mean", "resnet.layer1.0.shortcut.0.bias",
              "resnet.post_bn.running_var", "regressor.mean_theta", "regressor.fc_blocks.fc1.weight"):
        assert k in dict(mine), k
    # the seeded fill covers exactly the regressor's entries
    assert [(k, tuple(np.shape(v))) for k, v in synthetic.hmr_state_dict(3).items()] == theirs


@needs_reference
def test_forward_ops_is_bit_identical_to_the_reference_forward(full):
    maker = _maker()
    ref, ref_hmr = maker.reference_module(0)
    x = maker.golden_input()
    with torch.no_grad():
        want = ref_hmr.HumanModelRecovery.forward(ref, x)
        want_feat = ref.resnet(x)
        got, got_feat = full(x, return_features=True)
    assert got.shape == (2, 85) and torch.equal(got, want) and torch.equal(got_feat, want_feat)


@needs_reference
def test_golden_file_equals_the_live_reference():
    data = _maker().compute()
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(data)
    for k, v in data.items():
        assert np.array_equal(gold[k], v), k


def test_golden_file_is_data_of_the_expected_shapes():
    gold = np.load(GOLDEN)
    assert gold["theta_fp32"].shape == (2, 85) and gold["theta_fp64"].dtype == np.float64
    assert gold["features_fp32"].shape == (2, 2048) and gold["features_fp64"].dtype == np.float64
    assert np.all(np.isfinite(gold["stage_absmax"])) and np.all(gold["stage_absmax"] > 0)


def test_forward_ops_reproduces_the_golden_thetas(full):
    """Without the reference tree: the tensor-op forward against the recorded reference output (same ops, same order)."""
    gold = np.load(GOLDEN)
    x = torch.from_numpy(synthetic.smooth_image(int(gold["input_seed"]), (2, 3, 224, 224)))
    with torch.no_grad():
        got, feat = full(x, return_features=True)
    e_ref = np.abs(gold["theta_fp32"] - gold["theta_fp64"]).max()
    assert np.abs(got.numpy() - gold["theta_fp64"]).max() <= 4 * e_ref
    f64 = gold["features_fp64"]
    assert np.linalg.norm(feat.numpy() - f64) / np.linalg.norm(f64) <= 4 * np.linalg.norm(gold["features_fp32"] - f64) / np.linalg.norm(f64)


def test_batchnorm_fold_equals_eval_batchnorm_in_fp64():
    rs = np.random.RandomState(7)
    bn = nn.BatchNorm2d(96).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, 96)))
        bn.bias.copy_(torch.from_numpy(rs.normal(0, 0.1, 96)))
        bn.running_mean.copy_(torch.from_numpy(rs.normal(0, 0.2, 96)))
        bn.running_var.copy_(torch.from_numpy(rs.uniform(0.5, 2.0, 96)))
    scale, shift = hmr_net.fold_batchnorm(bn)
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    x = torch.from_numpy(rs.normal(0, 2.0, (2, 96, 5, 5)))
    with torch.no_grad():
        want = bn.double()(x)
    got = x * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    # one fp32 rounding of scale (relative 2^-24, times |x|) and one of shift
    bound = 2.0 ** -24 * (x.abs() * scale.double().abs().view(1, -1, 1, 1) + shift.double().abs().view(1, -1, 1, 1)) + 1e-15
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())
    # and the exact statement: the fp32 pair is the rounding of the fp64 fold
    g, b, m, v = (t.double() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    s64 = g / torch.sqrt(v + 1e-5)
    assert torch.equal(scale, s64.float()) and torch.equal(shift, (b - m * s64).float())


def test_pack_weights_matches_the_library_plan():
    """The blob's length is what the C plan computes for the same block counts (checked on the host, no device needed)."""
    nb = (3, 2, 2, 2)
    m = hmr_net.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0), num_blocks=nb)
    blob = hmr_net.pack_weights(m.resnet, m.regressor)
    n_params = sum(int(np.prod(v.shape)) for k, v in m.state_dict().items()
                   if not k.startswith("smpl.") and not k.endswith("num_batches_tracked"))
    n_bn = sum(mod.num_features for mod in m.resnet.modules() if isinstance(mod, nn.BatchNorm2d))
    assert blob.numel() == n_params - 2 * n_bn and blob.dtype == torch.float32    # four BatchNorm vectors fold into two


def test_the_light_class_still_raises_and_the_full_class_validates(full):
    light = batch_smpl.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0))
    assert not hasattr(light, "resnet") and sum(p.numel() for p in light.parameters()) == 0
    with pytest.raises(NotImplementedError):
        light(torch.zeros(1, 3, 224, 224))
    assert isinstance(full, batch_smpl.HumanModelRecovery)
    with pytest.raises(ValueError):
        full(torch.zeros(1, 3, 256, 256))
    with pytest.raises(TypeError):
        full(torch.zeros(1, 3, 224, 224, dtype=torch.float64))
    full.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            full(torch.zeros(1, 3, 224, 224))
    finally:
        full.eval()
    from impersonator_amd.networks.networks import NetworksFactory
    assert type(NetworksFactory.get_by_name("hmr", smpl_params=batch_smpl.synthetic_smpl_params(0), num_blocks=(1, 1, 1, 1))) \
        is hmr_net.HumanModelRecovery


def test_imitator_without_a_regressor_keeps_raising():
    """The three entry points of Imitator with the light class: the wiring decides before anything touches the device."""
    from impersonator_amd.models.imitator import Imitator
    stub = Imitator.__new__(Imitator)
    stub.hmr = batch_smpl.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0))
    with pytest.raises(NotImplementedError):
        stub.transfer_params("frame.jpg")
    with pytest.raises(NotImplementedError):
        stub.inference(["frame.jpg"])
    with pytest.raises(NotImplementedError):
        stub._extract_smpls("frame.jpg")
    img = stub._hmr_image((np.random.RandomState(0).rand(40, 30, 3) * 255).astype(np.uint8))
    assert img.shape == (3, 224, 224) and img.dtype == np.float32 and -1.0 <= img.min() and img.max() <= 1.0


def test_argument_validation_without_a_device():
    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    p = ctypes.c_void_p(4096)
    h = ctypes.c_void_p()
    nb = (ctypes.c_int * 4)(3, 4, 6, 3)
    assert lib.lwg_hmr_create(None, 8, nb) == INVALID and b"NULL" in lib.lwg_last_error()
    assert lib.lwg_hmr_create(ctypes.byref(h), 0, nb) == INVALID and h.value is None
    assert lib.lwg_hmr_create(ctypes.byref(h), 8, (ctypes.c_int * 4)(3, 0, 6, 3)) == INVALID and h.value is None
    lib.lwg_hmr_destroy(None)
    assert lib.lwg_hmr_weight_floats(None) == 0
    assert lib.lwg_hmr_set_weights(None, p, 16) == INVALID
    assert lib.lwg_hmr_forward(None, p, 1, 224, 224, p, None, None) == INVALID and b"NULL" in lib.lwg_last_error()

    def conv(x=p, w=p, y=p, N=1, H=7, W=7, Cin=64, Cout=64, k=1, s=1, pad=0, pre=(None, None), post=(None, None), res=None, rs=1,
             rh=7, rw=7):
        return lib.lwg_hmr_conv(x, N, H, W, Cin, w, Cout, k, s, pad, pre[0], pre[1], None, post[0], post[1], res, rs, rh, rw, y, None)

    assert conv(x=None) == INVALID and conv(w=None) == INVALID and conv(y=None) == INVALID
    assert conv(N=0) == INVALID and conv(H=0) == INVALID and conv(Cin=0) == INVALID
    assert conv(pre=(p, None)) == INVALID and conv(post=(None, p)) == INVALID
    assert conv(x=ctypes.c_void_p(4100)) == INVALID
    assert conv(k=5, pad=2) == UNSUPPORTED and conv(k=3, s=2, pad=0) == UNSUPPORTED and conv(k=1, s=2) == UNSUPPORTED
    assert conv(Cout=96) == UNSUPPORTED and b"Cout" in lib.lwg_last_error()
    assert conv(res=p, rs=2, rh=7, rw=7) == INVALID          # a stride-2 read of a 7 x 7 tensor does not cover 7 x 7 outputs
    assert conv(res=p, rs=0) == INVALID
    assert lib.lwg_hmr_maxpool(None, 1, 16, 16, 64, p, None) == INVALID
    assert lib.lwg_hmr_maxpool(p, 1, 2, 16, 64, p, None) == INVALID
    assert lib.lwg_hmr_maxpool(p, 1, 16, 16, 6, p, None) == UNSUPPORTED
    assert lib.lwg_hmr_pool_features(p, 1, 49, 2048, None, p, p, None) == INVALID
    assert lib.lwg_hmr_pool_features(p, 0, 49, 2048, p, p, p, None) == INVALID
    ws = lib.lwg_hmr_regress_workspace_bytes
    assert ws(3) == 3 * 2 * 1024 * 4 and ws(0) == 0
    reg = lambda feat, n, out, w, nbytes, fc3=p: lib.lwg_hmr_regress(feat, n, p, p, p, p, p, fc3, p, out, w, nbytes, None)
    assert reg(None, 3, p, p, ws(3)) == INVALID and reg(p, 3, None, p, ws(3)) == INVALID and reg(p, 3, p, p, ws(3), fc3=None) == INVALID
    assert reg(p, 0, p, p, ws(3)) == INVALID and reg(p, 3, p, None, 0) == INVALID
    assert reg(p, 3, p, p, ws(3) - 1) == WORKSPACE
