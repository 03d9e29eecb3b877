#!/usr/bin/env python
"""Writes tests/golden/lpips_golden.npz from the LIVE reference (thirdparty/his_evaluators/.../metrics/lpips):

    python tests/golden/make_lpips_golden.py

The reference's own `networks_basic.PNetLin('alex', version='0.1')` on the CPU in eval mode, its `lin` layers loaded from the
reference's weights/v0.1/alex.pth and its AlexNet from `synthetic.lpips_state_dicts(seed)` (the trained torchvision AlexNet is a
download; `torchvision.models.alexnet` is stubbed with a stand-in module of the standard architecture, `skimage` with an empty
module -- neither is installed, and the forward touches neither).  Run in fp32 (the reference's arithmetic) and in fp64 (the
yardstick both that and the device kernels are measured against) over the cases of tests/lpips_ref.py.

Data only: the five `lin` vectors (1152 floats), the case list by seed and shape, distances and per-layer terms in both precisions,
and the worst relative error of the reference's fp32 results against fp64 over the cases: `ref_fp32_rel_err` for the distances,
`ref_fp32_rel_err_taps` for the per-layer terms.  Images and AlexNet weights are regenerated from their seeds.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from impersonator_amd.utils import synthetic  # noqa: E402
from oracle import reference_loader  # noqa: E402
from tests import lpips_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lpips_golden.npz")
LPIPS_DIR = os.path.join(reference_loader.REFERENCE_ROOT, "thirdparty", "his_evaluators", "his_evaluators", "metrics", "lpips")


class _AlexNetFeatures(nn.Module):
    """stand-in for torchvision.models.alexnet: `.features` with the standard layers at the standard indices"""

    def __init__(self, pretrained=False):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))


def reference_available():
    return os.path.isdir(LPIPS_DIR)


def reference_networks_basic():
    """the reference's lpips/models/networks_basic.py, imported under a private package name WITHOUT running lpips/__init__.py
    (which pulls in the training harness and its dependencies).  The stubs stand in sys.modules only while it is imported."""
    if "_ref_lpips.models.networks_basic" in sys.modules:
        return sys.modules["_ref_lpips.models.networks_basic"]
    stubs = {"torchvision": {}, "torchvision.models": {"alexnet": _AlexNetFeatures}, "skimage": {}, "skimage.measure": {"compare_ssim": None}}
    saved = {name: sys.modules.get(name) for name in stubs}
    try:
        for name, attrs in stubs.items():
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
        sys.modules["torchvision"].models = sys.modules["torchvision.models"]
        sys.modules["skimage"].measure = sys.modules["skimage.measure"]
        for name, sub in (("_ref_lpips", ""), ("_ref_lpips.models", "models")):
            pkg = types.ModuleType(name)
            pkg.__path__ = [os.path.join(LPIPS_DIR, sub)]
            sys.modules[name] = pkg
        return importlib.import_module("_ref_lpips.models.networks_basic")
    finally:
        for name, old in saved.items():
            if old is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = old


def reference_lin_state_dict():
    sd = torch.load(os.path.join(LPIPS_DIR, "weights", "v0.1", "alex.pth"), map_location="cpu")
    return {k: v.detach().float() for k, v in sd.items()}


def reference_model(alex, lin):
    """PNetLin('alex') in eval mode with `alex` (torchvision keys) in its backbone and `lin` in its linear layers; every key matched"""
    nb = reference_networks_basic()
    net = nb.PNetLin(pnet_type="alex", pnet_rand=True, pnet_tune=False, use_dropout=True, use_gpu=False, spatial=False, version="0.1")
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in lin.items()}, strict=True)
    backbone = net.net[0]
    sd = {}
    for key in backbone.state_dict():                      # slice<j>.<i>.weight / .bias  <-  features.<i>.weight / .bias
        sd[key] = torch.as_tensor(np.asarray(alex["features." + key.split(".", 1)[1]]))
    assert len(sd) == 10, sorted(sd)
    backbone.load_state_dict(sd, strict=True)
    backbone.eval()
    return net.eval()


@torch.no_grad()
def reference_forward(net, pred, ref, dtype):
    """-> (dist (n,), taps (n,5)) by the reference's forward in `dtype`; the per-layer terms by its own modules, layer by layer"""
    net = net.to(dtype)
    net.net[0].to(dtype)
    p, r = torch.as_tensor(pred).to(dtype), torch.as_tensor(ref).to(dtype)
    dist = net.forward(p, r).reshape(-1)
    sc = lambda x: (x - net.shift.expand_as(x)) / net.scale.expand_as(x)
    o0, o1 = net.net[0].forward(sc(p)), net.net[0].forward(sc(r))
    nb = sys.modules["_ref_lpips.models.networks_basic"]
    taps = []
    for k in range(5):
        diff = (nb.util.normalize_tensor(o0[k]) - nb.util.normalize_tensor(o1[k])) ** 2
        taps.append(torch.mean(torch.mean(net.lins[k].model(diff), dim=3), dim=2).reshape(-1))
    return dist.double().numpy(), torch.stack(taps, dim=1).double().numpy()


def compute():
    alex, _ = synthetic.lpips_state_dicts(lpips_ref.GOLDEN_SEED)
    lin = reference_lin_state_dict()
    assert sorted(lin) == ["lin%d.model.1.weight" % j for j in range(5)], sorted(lin)
    net = reference_model(alex, lin)
    out = dict(seed=np.int64(lpips_ref.GOLDEN_SEED), case_names=np.array([c[0] for c in lpips_ref.CASES]),
               case_shapes=np.array([c[1:] for c in lpips_ref.CASES], np.int64), kinds=np.array(["noise", "near"]))
    for j in range(5):
        v = lin["lin%d.model.1.weight" % j].numpy()
        assert (v >= 0).all()
        out["lin%d" % j] = v.reshape(-1)
    worst = worst_taps = 0.0
    for i, case in enumerate(lpips_ref.CASES):
        for kind in ("noise", "near"):
            pred, ref = lpips_ref.case_inputs(i, kind)
            d32, t32 = reference_forward(net, pred, ref, torch.float32)
            d64, t64 = reference_forward(net, pred, ref, torch.float64)
            rel_d, rel_t = np.abs(d32 - d64) / d64, np.abs(t32 - t64) / t64
            worst, worst_taps = max(worst, float(rel_d.max())), max(worst_taps, float(rel_t.max()))
            print("%-8s %-5s dist %s  fp32 rel err: dist %.3g, taps %.3g" % (case[0], kind, d64, rel_d.max(), rel_t.max()))
            key = "%s_%s" % (case[0], kind)
            out[key + "_dist_fp64"], out[key + "_taps_fp64"] = d64, t64
            out[key + "_dist_fp32"], out[key + "_taps_fp32"] = d32, t32
    # each quantity has its own yardstick, as features and theta have in hmr_golden.npz: the distances theirs (the smaller figure:
    # five terms' errors average out in their sum), the per-layer terms theirs
    out["ref_fp32_rel_err"] = np.float64(worst)
    out["ref_fp32_rel_err_taps"] = np.float64(worst_taps)
    return out


if __name__ == "__main__":
    data = compute()
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes); ref_fp32_rel_err %.3g" % (OUT, os.path.getsize(OUT), float(data["ref_fp32_rel_err"])))
