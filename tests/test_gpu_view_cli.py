"""The novel-view command line, executed (reference: run_view.py:36-85): `run_view.py --synthetic --save_res` writes ONE image
grid of the turntable.  What lands on disk is compared byte for byte with torchvision's make_grid + save_image conversion
(written as torch CPU operations, tests/test_gpu_views.py::oracle_grid) of the views the same model computes in this process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from impersonator_amd import demo
from tests.test_gpu_views import oracle_grid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(cmd, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    assert p.returncode == 0, "%s failed (%d)\n%s\n%s" % (cmd, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_run_view_writes_the_grid_of_its_views(tmp_path):
    import run_view
    out_dir = str(tmp_path / "view")
    stdout = _run([sys.executable, "run_view.py", "--synthetic", "--save_res", "--image_size", "128", "--batch_size", "2",
                   "--num_views", "5", "--output_dir", out_dir])
    path = os.path.join(out_dir, "viewers", "synthetic.png")
    assert "Saving results to" in stdout and os.path.exists(path)
    disk = _read(path)
    assert disk.shape == (130 * 1 + 2, 130 * 5 + 2, 3) == (132, 652, 3) and disk.dtype == np.uint8

    # the same model in this process
    vw, smpl, img, bg = demo.build_synthetic_imitator(batch_size=2, image_size=128, model="viewer",
                                                      opt=demo.default_opt(batch_size=2, image_size=128))
    vw.personalize(img, src_smpl=smpl, bg_img=bg)
    rts, ts = run_view.view_schedule(run_view.parse_view_params('R=0,90,0/t=0,0,0'), 5)
    preds = vw.views(rts, ts)
    assert preds.shape == (5, 3, 128, 128)
    mine = oracle_grid(preds, nrow=8, padding=2, pad_value=0.0, normalize=True).numpy()
    assert np.array_equal(disk, mine), "the file is not save_image's uint8 grid of the views this model computes"
    assert disk[2:130, 2:130].std() > 10       # not a constant picture
    vw.generator.release()


def test_run_view_defaults_write_the_reference_layout(tmp_path):
    out_dir = str(tmp_path / "view16")
    stdout = _run([sys.executable, "run_view.py", "--synthetic", "--save_res", "--output_dir", out_dir])
    path = os.path.join(out_dir, "viewers", "synthetic.png")
    assert "Saving results to" in stdout and os.path.exists(path)
    disk = _read(path)
    assert disk.shape == (518, 2066, 3) and disk.dtype == np.uint8      # 16 views of 256 x 256, 8 per row, padding 2
    assert disk.std() > 10
