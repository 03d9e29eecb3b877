#!/usr/bin/env python
"""Motion imitation entry point -- command line of the reference's run_imitator.py (run_imitator.py:214-241).

    python run_imitator.py --src_path S.jpg --tgt_path DIR --load_path G.pth --output_dir OUT   (real assets)
    python run_imitator.py --synthetic --num_frames 64 --output_dir OUT                          (no assets)
    python -m torch.distributed.run --nproc-per-node 8 ... run_imitator.py --synthetic ...       (8 GPUs, frame-sharded)

    python run_imitator.py --synthetic --hmr_model H.pth --src_path S.jpg --tgt_path DIR --output_dir OUT
                                                      (synthetic body model and generator, SMPLs estimated from the images)
    python run_imitator.py ... --post_tune --pri_path DIR     (personalise by fine-tuning first: adaptive_personalize)
    python run_imitator.py ... --device_jpeg [--jpeg_quality 75] [--jpeg_subsampling 420] [--save_video OUT.avi]
                                                      (frames encoded as JPEG on the device; the streams also as one MJPG .avi)

When `--hmr_model` names a checkpoint of the HMR regressor (the reference's hmr_tf2pt.pth, or one saved from
`utils.synthetic.hmr_state_dict`), the SMPL parameters of source and targets are estimated from the images as the reference
does.  An `<image>.smpl.npy` file next to an image takes precedence; without a regressor those files are required.
"""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from impersonator_amd import demo, sharding  # noqa: E402
from impersonator_amd.options.jpeg_options import JpegOptions  # noqa: E402
from impersonator_amd.utils import cv_utils, util  # noqa: E402


def scan_tgt_paths(tgt_path, itv=20):
    """run_imitator.py:58-66."""
    if os.path.isdir(tgt_path):
        paths = sorted(glob.glob(os.path.join(tgt_path, '*')))
        paths = [p for p in paths if not p.endswith('.npy')][::itv]
    else:
        paths = [tgt_path]
    return paths


def _smpl_of(path, optional=False):
    f = path + '.smpl.npy'
    if not os.path.exists(f):
        if optional:
            return None
        raise FileNotFoundError("%s: SMPL vector (85,) expected next to the image (or give --hmr_model a checkpoint)" % f)
    return np.load(f).astype(np.float32).reshape(85)


def _target_smpls(imitator, tgt_paths):
    """(len, 85): the `.smpl.npy` files where every target has one, else the regressor's estimates."""
    have_hmr = hasattr(imitator.hmr, 'regressor')
    given = [_smpl_of(p, optional=have_hmr) for p in tgt_paths]
    if all(g is not None for g in given):
        return np.stack(given)
    return imitator._extract_smpls_batched(tgt_paths).cpu().numpy()


SYNTHETIC_PRIORS = 8     # --synthetic --post_tune: seeded prior poses (there is no --pri_path folder to scan)


def adaptive_personalize(opt, imitator, visualizer=None):
    """run_imitator.py:199-211: personalisation by fine-tuning.  The source is personalised already; the priors -- every 40th
    file of --pri_path (meta_imitate, :72), 8 seeded poses under --synthetic -- are imitated, the samples built on the device
    (models/post_tune.py: meta_samples; no pickles, no JPEGs) and the generator tuned on them (Imitator.post_personalize).
    The caller personalises again afterwards, as the reference does (:229)."""
    from impersonator_amd.models.post_tune import meta_samples
    print('\n\t\t\tPersonalization: meta imitation...')
    if opt.synthetic:
        samples = meta_samples(imitator, tgt_smpls=demo.synthetic_smpls(SYNTHETIC_PRIORS, seed=7), cam_strategy=opt.cam_strategy)
    else:
        pri_paths = scan_tgt_paths(opt.pri_path, itv=40)
        samples = meta_samples(imitator, tgt_paths=pri_paths, tgt_smpls=_target_smpls(imitator, pri_paths), cam_strategy=opt.cam_strategy)
    print('\n\t\t\tPersonalization: meta cycle finetune...')
    return imitator.post_personalize(opt.output_dir, samples, visualizer=visualizer, verbose=False)


def write_device_jpegs(opt, imitator, tgt_smpls, tgt_paths, rank, world):
    """--device_jpeg: every rank encodes its own frames on the device and writes the finished streams (no float frame comes to
    the host, nothing is gathered); named after the target files, `pred_%08d.jpg` for the synthetic sequence.  --save_video:
    rank 0 then stores the written streams, as they are, in one Motion-JPEG .avi file."""
    out_dir = util.mkdir(opt.output_dir)
    name = lambda t: 'pred_' + (imitator._jpg_name(os.path.split(tgt_paths[t])[-1]) if tgt_paths else '%.8d.jpg' % t)

    def sink(t, data):
        path = os.path.join(out_dir, name(t))
        with open(path, 'wb') as fh:
            fh.write(data)
        return path

    written = sharding.imitate_sharded(imitator, tgt_smpls, opt.batch_size, opt.cam_strategy, rank, world, jpeg_sink=sink,
                                       jpeg=dict(quality=opt.jpeg_quality, subsampling=opt.jpeg_subsampling))
    print('wrote %d frames to %s' % (len(written), out_dir) if world == 1 else
          'rank %d wrote %d frames to %s' % (rank, len(written), out_dir))
    if opt.save_video:
        sharding.barrier()
        if rank == 0:
            from impersonator_amd.utils.video import write_mjpeg_avi
            streams = []
            for t in range(len(tgt_smpls)):
                with open(os.path.join(out_dir, name(t)), 'rb') as fh:
                    streams.append(fh.read())
            write_mjpeg_avi(opt.save_video, streams, opt.fps, (opt.image_size, opt.image_size))
            print('wrote %d frames to %s' % (len(streams), opt.save_video))


def main():
    opt = JpegOptions().parse()
    rank, local_rank, world = sharding.init_process_group()
    if local_rank >= torch.cuda.device_count() and os.environ.get("LWG_DIST_BACKEND") == "gloo":
        local_rank %= torch.cuda.device_count()   # test hook: N gloo ranks sharing the visible GPU(s) (RCCL wants one each)
    torch.cuda.set_device(local_rank)
    if opt.synthetic:
        imitator, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(
            batch_size=opt.batch_size, image_size=opt.image_size,
            opt=demo.default_opt(batch_size=opt.batch_size, image_size=opt.image_size, front_warp=opt.front_warp,
                                 only_vis=opt.only_vis, align_corners=opt.align_corners,
                                 map_name=getattr(opt, 'map_name', 'uv_seg'), hmr_model=opt.hmr_model,
                                 post_tune=opt.post_tune, face_model=opt.face_model))
        if hasattr(imitator.hmr, 'regressor') and opt.src_path:
            # pictures in, pictures out: SMPLs of the source and of the targets come from the HMR regressor
            personalize = lambda: imitator.personalize(opt.src_path, bg_img=bg_img)
            personalize()
            tgt_paths = scan_tgt_paths(opt.tgt_path, itv=1) if opt.tgt_path else None
            tgt_smpls = _target_smpls(imitator, tgt_paths) if tgt_paths else demo.synthetic_smpls(opt.num_frames, seed=0)
        else:
            personalize = lambda: imitator.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
            personalize()
            tgt_smpls = demo.synthetic_smpls(opt.num_frames, seed=0)
            tgt_paths = None
    else:
        from impersonator_amd.models.imitator import Imitator
        imitator = Imitator(opt)
        bg = None
        bg_file = opt.src_path + '.bg.npy'
        if os.path.exists(bg_file):
            bg = np.load(bg_file)
        have_hmr = hasattr(imitator.hmr, 'regressor')
        personalize = lambda: imitator.personalize(opt.src_path, src_smpl=_smpl_of(opt.src_path, optional=have_hmr), bg_img=bg)
        personalize()
        tgt_paths = scan_tgt_paths(opt.tgt_path, itv=1)
        tgt_smpls = _target_smpls(imitator, tgt_paths)
    if opt.post_tune:
        adaptive_personalize(opt, imitator, None)
        personalize()            # run_imitator.py:229: once more, on the tuned weights
        print('\n\t\t\tPersonalization: completed...')

    if opt.save_video and not (opt.device_jpeg and opt.output_dir):
        raise SystemExit('--save_video stores the streams of --device_jpeg: give --device_jpeg and --output_dir too')
    if opt.device_jpeg and opt.output_dir:
        write_device_jpegs(opt, imitator, tgt_smpls, tgt_paths, rank, world)
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        return

    # frame sharding: every rank imitates its own blocks of `batch_size` frames (first_cam = frame 0's camera everywhere)
    outs = sharding.imitate_sharded(imitator, tgt_smpls, opt.batch_size, opt.cam_strategy, rank, world)
    if rank == 0 and opt.output_dir:
        out_dir = util.mkdir(opt.output_dir)
        for t, img in enumerate(outs):
            # the reference names its outputs after the target files (run_imitator.py:232, 'pred_%.8d.jpg' in
            # inference_by_smpls); the synthetic sequence has no files and is written losslessly, so that what lands on
            # disk IS the uint8 truncation of utils/cv_utils.py:31-33 (hazard H11) and can be compared as such
            name = os.path.split(tgt_paths[t])[-1] if tgt_paths else '%.8d.png' % t
            cv_utils.save_cv2_img(img, os.path.join(out_dir, 'pred_' + name), normalize=True)
        print('wrote %d frames to %s' % (len(outs), out_dir))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
