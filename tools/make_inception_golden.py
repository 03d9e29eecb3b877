#!/usr/bin/env python
"""Writes tests/golden/inception_synth.npz on the CPU: for the whole-network cases of tests/inception_ref.py (seeded weights,
seeded frames), the fp64 features of the restated module and the restated fp32 module's own relative L2 error against them
(`ref_fp32_rel_err`, per case, worst frame) -- the yardstick the device is held to (4 x).  Reads nothing outside the repository.

    python tools/make_inception_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd.utils import synthetic  # noqa: E402
from tests import inception_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "inception_synth.npz")


def rel_l2(a, b):
    """worst frame of |a - b|_2 / |b|_2"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max())


@torch.no_grad()
def main():
    torch.manual_seed(0)
    sd = synthetic.inception_state_dict(inception_ref.SEED)
    net64 = inception_ref.build(sd, torch.float64)
    net32 = inception_ref.build(sd, torch.float32)
    out = {"seed": np.int64(inception_ref.SEED), "case_names": np.array([c[0] for c in inception_ref.CASES]),
           "case_shapes": np.array([c[1:] for c in inception_ref.CASES], np.int64)}
    errs = []
    for index, (name, _, _, _, size) in enumerate(inception_ref.CASES):
        frames = torch.from_numpy(inception_ref.case_frames(index))
        f64 = net64(inception_ref.preprocess(frames.double(), size)).numpy()
        f32 = net32(inception_ref.preprocess(frames, size)).numpy()
        err = rel_l2(f32, f64)
        errs.append(err)
        out[name + "_features_fp64"] = f64
        print("%-14s features %s, |f| %.3g, zeros %d, restated fp32 vs fp64 rel L2 %.3g" % (
            name, f64.shape, float(np.abs(f64).mean()), int((f64 == 0).sum()), err))
    out["ref_fp32_rel_err"] = np.asarray(errs, np.float64)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
