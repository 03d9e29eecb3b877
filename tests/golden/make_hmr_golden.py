#!/usr/bin/env python
"""Writes tests/golden/hmr_golden.npz from the LIVE reference (networks/hmr.py through oracle.reference_loader):

    python tests/golden/make_hmr_golden.py

The reference's ResNet-50 + ThetaRegressor under `synthetic.hmr_state_dict(seed)` on a batch of two seeded images, run by the
reference's own `HumanModelRecovery.forward` in fp32 (its arithmetic) and in fp64 (the yardstick both the reference's fp32
forward and the device kernels are measured against).  Data only: seeds, thetas, features, per-stage absmax.
"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from impersonator_amd.utils import synthetic  # noqa: E402
from oracle import reference_loader  # noqa: E402

SEED, INPUT_SEED, BATCH = 0, 5, 2
OUT = os.path.join(ROOT, "tests", "golden", "hmr_golden.npz")


def golden_input(input_seed=INPUT_SEED, batch=BATCH):
    return torch.from_numpy(synthetic.smooth_image(input_seed, (batch, 3, 224, 224)))


def reference_module(seed=SEED, num_blocks=(3, 4, 6, 3)):
    """The reference's regressor without its SMPL pickle: an nn.Module carrying the reference's own `resnet` and `regressor`,
    which is all `HumanModelRecovery.forward` (hmr.py:276-300) touches.  -> (module, reference networks.hmr)."""
    reference_loader.load()
    ref_hmr = importlib.import_module("networks.hmr")
    m = nn.Module()
    m.resnet = ref_hmr.PreActResNet(ref_hmr.PreActBottleneck, list(num_blocks))
    m.regressor = ref_hmr.ThetaRegressor(2048 + 85, 85, 3)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.hmr_state_dict(seed, num_blocks).items()})
    return m.eval(), ref_hmr


def reference_forward(m, ref_hmr, x):
    """-> (thetas, features, {stage: absmax}) by the reference's forward, the stages re-run module by module."""
    with torch.no_grad():
        thetas = ref_hmr.HumanModelRecovery.forward(m, x)
        features = m.resnet(x)
        stages = {}
        out = m.resnet.conv1(x)
        stages["stem"] = out
        out = torch.nn.functional.max_pool2d(out, kernel_size=3, stride=2, ceil_mode=True)
        stages["maxpool"] = out
        for name in ("layer1", "layer2", "layer3", "layer4"):
            out = getattr(m.resnet, name)(out)
            stages[name] = out
        stages["features"] = features
        stages["theta"] = thetas
    return thetas, features, {k: float(v.abs().max()) for k, v in stages.items()}


def compute():
    m, ref_hmr = reference_module()
    x = golden_input()
    t32, f32, _ = reference_forward(m, ref_hmr, x)
    m = m.double()
    t64, f64, stages = reference_forward(m, ref_hmr, x.double())
    for k, v in stages.items():
        assert np.isfinite(v) and v > 0, "stage %s has absmax %r" % (k, v)
    return dict(seed=np.int64(SEED), input_seed=np.int64(INPUT_SEED), theta_fp32=t32.numpy(), features_fp32=f32.numpy(),
                theta_fp64=t64.numpy(), features_fp64=f64.numpy(), stage_names=np.array(list(stages)),
                stage_absmax=np.array([stages[k] for k in stages], np.float64))


if __name__ == "__main__":
    data = compute()
    np.savez_compressed(OUT, **data)
    f32, f64, t32, t64 = data["features_fp32"], data["features_fp64"], data["theta_fp32"], data["theta_fp64"]
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    print("stages:", dict(zip(data["stage_names"].tolist(), data["stage_absmax"].tolist())))
    print("fp32 vs fp64: features rel L2 %.3g, theta max abs %.3g" % (
        np.linalg.norm(f32 - f64) / np.linalg.norm(f64), np.abs(t32 - t64).max()))
