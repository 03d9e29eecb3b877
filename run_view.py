#!/usr/bin/env python
"""Novel view synthesis entry point -- command line of the reference's run_view.py (run_view.py:15-85).

    python run_view.py --synthetic --save_res --output_dir OUT                      (seeded synthetic subject, no assets)
    python run_view.py --src_path S.jpg --load_path G.pth --save_res --output_dir OUT --view_params R=0,90,0/t=0,0,0

A turntable of `--num_views` views (16 in the reference): R[0] = R[2] = 10 degrees, R[1] = 360 / length * i, t from
`--view_params`.  The views are computed in blocks of `--batch_size` (Viewer.views) and written as ONE image grid -- what the
reference's `torchvision.utils.save_image((preds + 1) / 2, path)` writes (8 per row, 2 pixels of padding) -- to
`<output_dir>/viewers/<name of the source image>`; the grid is laid out and converted to bytes on the device.

With real assets the source's SMPL vector / background are read from `<image>.smpl.npy` / `<image>.bg.npy`; when `--hmr_model`
names a checkpoint of the HMR regressor the SMPL vector is estimated from the image as the reference does.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.options.view_options import ViewOptions  # noqa: E402
from impersonator_amd.utils import util  # noqa: E402


def parse_view_params(view_params):
    """run_view.py:15-33: 'R=x,y,z/t=x,y,z' -> {'R': (3,) float32 in RADIANS (given in degrees), 't': (3,) float32}."""
    fields = dict(segment.split('=') for segment in view_params.split('/'))
    out = {key: np.asarray([float(v) for v in text.split(',')], dtype=np.float32) for key, text in fields.items()}
    out['R'] = out['R'] / 180 * np.pi      # float32 throughout, like the reference's own conversion
    return out


def view_schedule(params, length=16):
    """run_view.py:58-69: the turntable -> (rts (length, 3) float32 radians, ts (length, 3) float32).  R[0] = R[2] = 10 degrees,
    R[1] = 360 / length * i degrees, stored into the float32 array as the reference stores them; t is carried through."""
    delta = 360 / length
    rts = np.empty((length, 3), dtype=np.float32)
    for i in range(length):
        rts[i, 0] = 10 / 180 * np.pi
        rts[i, 1] = delta * i / 180.0 * np.pi
        rts[i, 2] = 10 / 180 * np.pi
    ts = np.tile(np.asarray(params['t'], dtype=np.float32).reshape(1, 3), (length, 1))
    return rts, ts


def _optional(path):
    return np.load(path) if os.path.exists(path) else None


def main():
    opt = ViewOptions().parse()
    torch.cuda.set_device(0)
    if opt.synthetic:
        viewer, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(
            batch_size=opt.batch_size, image_size=opt.image_size, model="viewer",
            opt=demo.default_opt(batch_size=opt.batch_size, image_size=opt.image_size, front_warp=opt.front_warp,
                                 bg_replace=opt.bg_replace, align_corners=opt.align_corners, post_tune=opt.post_tune,
                                 face_model=opt.face_model))
        personalize = lambda: viewer.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
        name = 'synthetic.png'
    else:
        from impersonator_amd.models.viewer import Viewer
        viewer = Viewer(opt)
        src_smpl = _optional(opt.src_path + '.smpl.npy')
        if src_smpl is None and not hasattr(viewer.hmr, 'regressor'):
            raise FileNotFoundError("%s.smpl.npy: SMPL vector (85,) expected next to the image (or give --hmr_model a checkpoint)"
                                    % opt.src_path)
        personalize = lambda: viewer.personalize(opt.src_path, src_smpl=src_smpl, bg_img=_optional(opt.src_path + '.bg.npy'))
        name = os.path.basename(opt.src_path)
    personalize()
    if opt.post_tune:            # run_view.py:46-47 of the reference: the same adaptive personalisation as run_imitator.py
        from run_imitator import adaptive_personalize
        adaptive_personalize(opt, viewer, None)
        personalize()
    print('\n\t\t\tPersonalization: completed...')

    rts, ts = view_schedule(parse_view_params(opt.view_params), opt.num_views)
    print('\n\t\t\tSynthesizing {} novel views'.format(len(rts)))
    preds = viewer.views(rts, ts)
    if opt.save_res:
        path = os.path.join(util.mkdir(os.path.join(opt.output_dir, 'viewers')), name)
        util.save_image_grid(preds, path, normalize=True)
        print('Saving results to {}'.format(path))


if __name__ == "__main__":
    main()
