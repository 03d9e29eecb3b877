"""run_mesh.py end to end in a child process: the three kinds of picture are written and agree with each other and with the
renderer called directly on the same seeded sequence."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, BATCH, SIZE = 4, 2, 64


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB")).astype(np.float32)


def test_run_mesh_writes_mesh_masked_and_warped_pictures(tmp_path, monkeypatch):
    out_dir = str(tmp_path / "out")
    cmd = [sys.executable, "run_mesh.py", "--synthetic", "--num_frames", str(FRAMES), "--batch_size", str(BATCH), "--image_size",
           str(SIZE), "--texture_warp", "--output_dir", out_dir]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, text=True)
    assert p.returncode == 0, "%s\n%s" % (p.stdout[-2000:], p.stderr[-4000:])
    assert "wrote %d frames" % FRAMES in p.stdout
    files = sorted(os.listdir(os.path.join(out_dir, "meshes")))
    assert files == sorted("%s_%08d.jpg" % (kind, t) for kind in ("mesh", "masked", "wt") for t in range(FRAMES)), files

    # the same sequence through the renderer directly: the silhouette decides what each picture may show
    import run_mesh
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))   # parse() exports --gpu_ids: undone after
    opt =run_mesh.MeshOptions().parse(cmd[2:])
    render, verts, cams, frames = run_mesh.synthetic_sequence(opt)
    sil = render.render_silhouettes(cams, verts).cpu().numpy()                  # (n,is,is) in {0, 1/4, .., 1}
    frames = frames.cpu().numpy()
    assert 0.05 < (sil > 0).mean() < 0.9 and ((sil > 0) & (sil < 1)).any()
    for t in range(FRAMES):
        mesh, masked, wt = (_read(os.path.join(out_dir, "meshes", "%s_%08d.jpg" % (kind, t))) for kind in ("mesh", "masked", "wt"))
        assert mesh.shape == masked.shape == wt.shape == (SIZE, SIZE, 3)
        # mesh_*: white cubes under a light of at least the ambient 0.7, so a pixel of coverage a shows >= 0.7 * a * 255 >= 44
        # levels and the black background 0; a JPEG at full quality moves a level by a few units, far from the 22 between them
        lit = mesh.max(axis=2) > 22
        assert np.array_equal(lit, sil[t] > 0), (t, int((lit != (sil[t] > 0)).sum()))
        # masked_*: the frame times the silhouette
        want = np.clip(frames[t] * sil[t][None], 0, 1).transpose(1, 2, 0) * 255
        assert np.abs(masked - want).max() <= 6, (t, np.abs(masked - want).max())
        assert masked[sil[t] == 0].max() <= 6
        # wt_*: nothing outside the mesh, the source's colours inside
        assert wt[sil[t] == 0].max() <= 6 and wt[sil[t] == 1].mean() > 20
