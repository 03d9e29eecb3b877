"""evaluate.py end to end in a child process: the synthetic sequence in the default arithmetic scored against the exact-fp32
generator.  The two bounds only catch a broken wiring (frames paired wrongly, the wrong mode, ground truth not on the device's
side of the comparison); the values themselves are recorded in profiles/eval.md."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evaluate_synthetic_against_fp32(tmp_path):
    out_dir = str(tmp_path / "out")
    cmd = [sys.executable, "evaluate.py", "--synthetic", "--num_frames", "8", "--batch_size", "4", "--output_dir", out_dir]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, text=True)
    assert p.returncode == 0, "%s\n%s" % (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    print(lines[0])
    assert res["frames"] == 8 and res["ground_truth"] == "fp32 generator" and res["quantize"] is False
    assert 0.99 < res["ssim"] <= 1.0
    assert math.isfinite(res["psnr"]) and res["psnr"] > 0
    assert "sspe" not in res                                   # no regressor checkpoint was given
    with open(os.path.join(out_dir, "metrics.json")) as fh:
        assert json.loads(fh.read()) == res
