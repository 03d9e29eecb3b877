"""evaluate.py with --lpips_alex / --lpips_lin in a child process: the synthetic sequence in the default arithmetic scored against
the exact-fp32 generator, LPIPS included.  The value itself is not asserted (nobody has measured what bf16x3 frames against fp32
frames give; profiles/lpips.md records it): the test catches a broken wiring only."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from impersonator_amd.utils import synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    return subprocess.run([sys.executable, "evaluate.py", "--synthetic", "--num_frames", "8", "--batch_size", "4"] + args, cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)


@pytest.fixture(scope="module")
def weight_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lpips")
    alex, lin = synthetic.lpips_state_dicts(0)
    paths = str(d / "alex.pth"), str(d / "lin.pth")
    torch.save({k: torch.from_numpy(v) for k, v in alex.items()}, paths[0])
    torch.save({k: torch.from_numpy(v) for k, v in lin.items()}, paths[1])
    return paths


def test_evaluate_synthetic_with_lpips(weight_files, tmp_path):
    out_dir = str(tmp_path / "out")
    p = _run(["--output_dir", out_dir, "--lpips_alex", weight_files[0], "--lpips_lin", weight_files[1]])
    assert p.returncode == 0, "%s\n%s" % (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    print(lines[0])
    assert res["frames"] == 8 and res["ground_truth"] == "fp32 generator"
    assert math.isfinite(res["lpips"]) and res["lpips"] >= 0
    assert math.isfinite(res["lpips_max"]) and res["lpips_max"] >= res["lpips"]
    assert 0.99 < res["ssim"] <= 1.0 and "sspe" not in res
    with open(os.path.join(out_dir, "metrics.json")) as fh:
        assert fh.read().strip() == lines[0]


@pytest.mark.parametrize("flag", ["--lpips_alex", "--lpips_lin"])
def test_one_flag_alone_is_refused(weight_files, flag):
    p = _run([flag, weight_files[0 if flag == "--lpips_alex" else 1]])
    assert p.returncode != 0
    assert "--lpips_alex" in p.stderr and "--lpips_lin" in p.stderr and not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
