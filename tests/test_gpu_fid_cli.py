"""evaluate.py with --inception in a child process: the synthetic sequence in the default arithmetic against the exact-fp32
generator, scored as two sets as well -- FID and Inception Score from the seeded InceptionV3 weights.  The values themselves are
not asserted (profiles/fid.md records them): the test catches a broken wiring, and that the flag changes nothing else.  The
2048 x 2048 matrix square root of the reference's method takes about 4 s on the host; that cost is accepted."""
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
SET_KEYS = ("fid", "is", "is_std")


def _run(args):
    p = subprocess.run([sys.executable, "evaluate.py", "--synthetic", "--num_frames", "16", "--batch_size", "8"] + args, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, "%s\n%s" % (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return lines[0]


@pytest.fixture(scope="module")
def weight_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("inception") / "inception.pth")
    torch.save({k: torch.from_numpy(v) for k, v in synthetic.inception_state_dict(0).items()}, path)
    return path


@pytest.fixture(scope="module")
def plain():
    return _run([])


def test_without_the_flag_none_of_the_keys_appears(plain):
    res = json.loads(plain)
    assert res["frames"] == 16 and not [k for k in SET_KEYS if k in res]


def test_evaluate_synthetic_with_fid_and_inception_score(weight_file, plain, tmp_path):
    out_dir = str(tmp_path / "out")
    line = _run(["--output_dir", out_dir, "--inception", weight_file])
    res, base = json.loads(line), json.loads(plain)
    print(line)
    assert res["frames"] == 16 and res["ground_truth"] == "fp32 generator"
    for k in SET_KEYS:
        assert math.isfinite(res[k]), k
    assert res["is"] >= 1.0 and res["is_std"] == 0.0                              # 16 frames: one batch of 32
    # every other key as without the flag, in value and in order
    assert [k for k in res if k not in SET_KEYS] == list(base) and all(res[k] == base[k] for k in base)
    with open(os.path.join(out_dir, "metrics.json")) as fh:
        assert fh.read().strip() == line
