#!/usr/bin/env python
"""Appearance transfer driven by a motion sequence: the source subject follows the target poses wearing the reference subject's parts.

    python run_animate.py --synthetic --num_frames 16 --batch_size 4 --swap_part upper_body --save_res --output_dir OUT
    python run_animate.py --src_path A.jpg --ref_path B.jpg --tgt_path DIR --load_path G.pth --swap_part body --save_res ...

The frames are written to OUT/animators/pred_<name>.jpg.  With real assets `--tgt_path` is an image or a folder of images as for
run_imitator.py; SMPL vectors / backgrounds are read from `<image>.smpl.npy` / `<image>.bg.npy` as for run_swap.py, the target
SMPLs from the HMR regressor where `--hmr_model` names a checkpoint and a file is missing."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.options.animate_options import AnimateOptions  # noqa: E402
from impersonator_amd.options.jpeg_options import add_jpeg_arguments  # noqa: E402
from impersonator_amd.utils import synthetic, util  # noqa: E402
from run_imitator import _target_smpls, scan_tgt_paths  # noqa: E402


class AnimateJpegOptions(AnimateOptions):
    """AnimateOptions + the flags of the device JPEG writer (--device_jpeg, --jpeg_quality, --jpeg_subsampling)"""

    def initialize(self):
        super().initialize()
        add_jpeg_arguments(self._parser)


def main():
    opt = AnimateJpegOptions().parse()
    torch.cuda.set_device(0)
    if opt.synthetic:
        an, smpl_a, img_a, bg_a = demo.build_synthetic_imitator(
            batch_size=opt.batch_size, image_size=opt.image_size, model="animator",
            opt=demo.default_opt(batch_size=opt.batch_size, image_size=opt.image_size, front_warp=opt.front_warp,
                                 only_vis=opt.only_vis, align_corners=opt.align_corners, swap_part=opt.swap_part))
        smpl_b = demo.synthetic_smpls(8, seed=3)[5]
        img_b = synthetic.smooth_image(77, (1, 3, opt.image_size, opt.image_size))[0]
        an.animate_setup(img_a, img_b, src_smpl=smpl_a, ref_smpl=smpl_b, src_bg=bg_a, ref_bg=bg_a)
        tgt_paths, tgt_smpls = None, demo.synthetic_smpls(opt.num_frames, seed=0)
    else:
        from impersonator_amd.models.animator import Animator
        an = Animator(opt)
        load = lambda p, ext: np.load(p + ext) if os.path.exists(p + ext) else None
        an.animate_setup(opt.src_path, opt.ref_path, src_smpl=load(opt.src_path, '.smpl.npy'),
                         ref_smpl=load(opt.ref_path, '.smpl.npy'), src_bg=load(opt.src_path, '.bg.npy'),
                         ref_bg=load(opt.ref_path, '.bg.npy'))
        tgt_paths = scan_tgt_paths(opt.tgt_path, itv=1)
        tgt_smpls = _target_smpls(an, tgt_paths)
    out_dir = util.mkdir(os.path.join(opt.output_dir, 'animators')) if opt.save_res else ''
    outs = an.animate(tgt_paths, tgt_smpls=tgt_smpls, cam_strategy=opt.cam_strategy, target_part=opt.swap_part, output_dir=out_dir,
                      device_jpeg=opt.device_jpeg, jpeg_quality=opt.jpeg_quality, jpeg_subsampling=opt.jpeg_subsampling)
    if out_dir:
        print('Saving %d frames to %s' % (len(outs), out_dir))


if __name__ == "__main__":
    main()
