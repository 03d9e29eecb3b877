#!/usr/bin/env python
"""Paired evaluation of motion imitation -- the counterpart of the reference's evaluate.py for its paired metrics (SSIM, PSNR,
with the HMR regressor the scale-shape-pose error, with the AlexNet and LPIPS weights LPIPS), computed on the device: no float
frame goes to the host.

    python evaluate.py --synthetic --num_frames 64 --output_dir OUT                 (no assets: default arithmetic vs exact fp32)
    python evaluate.py --src_path S.jpg --tgt_path DIR --load_path G.pth --output_dir OUT        (self-imitation, real assets)
    python evaluate.py ... --quantize                (score what an 8-bit writer would have stored)
    python evaluate.py ... --hmr_model H.pth         (adds SSPE)
    python evaluate.py ... --lpips_alex A.pth --lpips_lin L.pth      (adds LPIPS v0.1 / alex: `lpips`, `lpips_max`; both or neither)
    python evaluate.py ... --inception I.pth         (adds FID and Inception Score: `fid`, `is`, `is_std`)

Ground truth: `--against fp32` runs the sequence through the exact-fp32 generator first and scores the default arithmetic
against it (the default under --synthetic, where no ground-truth pictures exist); `--against target` takes the frames of
--tgt_path, loaded and resized as run_imitator.py loads them and uploaded per batch.  One JSON line goes to stdout and to
<output_dir>/metrics.json.  A.pth is torchvision's alexnet state_dict, L.pth the LPIPS v0.1 alex.pth; without the two flags the
output carries no `lpips` key.  I.pth is torchvision's inception_v3 state_dict (or a torch.save of
utils.synthetic.inception_state_dict(0)): the predictions and the ground-truth frames the paired metrics score are also scored as
two sets -- FID between them, the Inception Score of the predictions per batch of 32 (the reference's FIDMetric and
InceptionScoreMetric, the softmax over the 2048 pool features included) -- on the host in fp64 from features computed on the device;
the 2048 x 2048 matrix square root takes a few seconds.  Without the flag the output carries none of the three keys.  Re-id and
face metrics need downloaded backbones and are not part of this.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.options.eval_options import EvalOptions  # noqa: E402
from impersonator_amd.utils import cv_utils, util  # noqa: E402
from impersonator_amd.utils.metrics import PairedEvaluator, SetEvaluator  # noqa: E402
from run_imitator import _smpl_of, _target_smpls, scan_tgt_paths  # noqa: E402


def build(opt):
    """-> (imitator, personalize(), tgt_smpls, tgt_paths or None), as run_imitator.py sets a run up"""
    if opt.synthetic:
        imitator, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(
            batch_size=opt.batch_size, image_size=opt.image_size,
            opt=demo.default_opt(batch_size=opt.batch_size, image_size=opt.image_size, front_warp=opt.front_warp,
                                 only_vis=opt.only_vis, align_corners=opt.align_corners, map_name=opt.map_name,
                                 hmr_model=opt.hmr_model, face_model=opt.face_model))
        if hasattr(imitator.hmr, 'regressor') and opt.src_path:
            personalize = lambda: imitator.personalize(opt.src_path, bg_img=bg_img)
        else:
            personalize = lambda: imitator.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
        personalize()
        tgt_paths = scan_tgt_paths(opt.tgt_path, itv=1) if opt.tgt_path else None
        tgt_smpls = _target_smpls(imitator, tgt_paths) if tgt_paths else demo.synthetic_smpls(opt.num_frames, seed=0)
        return imitator, personalize, tgt_smpls, tgt_paths
    from impersonator_amd.models.imitator import Imitator
    imitator = Imitator(opt)
    bg_file = opt.src_path + '.bg.npy'
    bg = np.load(bg_file) if os.path.exists(bg_file) else None
    have_hmr = hasattr(imitator.hmr, 'regressor')
    personalize = lambda: imitator.personalize(opt.src_path, src_smpl=_smpl_of(opt.src_path, optional=have_hmr), bg_img=bg)
    personalize()
    tgt_paths = scan_tgt_paths(opt.tgt_path, itv=1)
    return imitator, personalize, _target_smpls(imitator, tgt_paths), tgt_paths


def batches_of(imitator, tgt_smpls, opt):
    """the (chunk, t) pairs Imitator._run_batches hands to predict_batches, camera reference included"""
    smpls = torch.as_tensor(np.asarray(tgt_smpls), dtype=torch.float32).reshape(len(tgt_smpls), -1)
    if opt.cam_strategy == 'smooth':
        imitator.first_cam = smpls[0:1, 0:3].clone().cuda()
    smpls = smpls.cuda()
    bs = max(1, int(opt.batch_size))
    return ((smpls[s:s + bs], s) for s in range(0, len(smpls), bs))


def target_batch(paths, size):
    """the target pictures as run_imitator.py's loader reads them: (n,3,size,size) in [-1,1], uploaded"""
    imgs = [cv_utils.transform_img(cv_utils.read_cv2_img(p), size, transpose=True) * 2 - 1.0 for p in paths]
    return torch.from_numpy(np.ascontiguousarray(np.stack(imgs), dtype=np.float32)).cuda()


def load_lpips(opt):
    """the LPIPS model of --lpips_alex / --lpips_lin, None without them; one flag alone is refused"""
    if bool(opt.lpips_alex) != bool(opt.lpips_lin):
        raise SystemExit("LPIPS needs both --lpips_alex (torchvision's AlexNet state_dict) and --lpips_lin (the LPIPS v0.1 "
                         "alex.pth): only %s was given" % ('--lpips_alex' if opt.lpips_alex else '--lpips_lin'))
    if not opt.lpips_alex:
        return None
    from impersonator_amd.networks.lpips import LPIPS
    return LPIPS(torch.load(opt.lpips_alex, map_location='cpu'), torch.load(opt.lpips_lin, map_location='cpu'),
                 max_batch=max(1, int(opt.batch_size)), image_size=opt.image_size)


def load_inception(opt):
    """the InceptionV3 model of --inception, None without it"""
    if not opt.inception:
        return None
    from impersonator_amd.networks.inception import InceptionV3
    return InceptionV3(torch.load(opt.inception, map_location='cpu'), max_batch=max(1, int(opt.batch_size)), image_size=opt.image_size)


@torch.no_grad()
def evaluate(opt):
    lpips = load_lpips(opt)                                # a lone flag ends the run before anything is built
    inception = load_inception(opt)
    imitator, personalize, tgt_smpls, tgt_paths = build(opt)
    gen = imitator.generator
    against = opt.against or ('target' if tgt_paths else 'fp32')
    if against == 'target' and not tgt_paths:
        raise SystemExit("--against target needs --tgt_path: there are no ground-truth pictures otherwise")
    hmr = imitator.hmr if hasattr(imitator.hmr, 'regressor') else None
    names = ('ssim', 'psnr') + (('sspe',) if hmr is not None else ()) + (('lpips',) if lpips is not None else ())
    ev = PairedEvaluator(names, hmr=hmr, mode=2 if opt.quantize else 0, lpips=lpips)
    sets = SetEvaluator(inception, mode=2 if opt.quantize else 0) if inception is not None else None

    truth = {}
    if against == 'fp32':
        # the ground truth stays on the device: 3*size^2 floats per frame, read again by the kernels only
        gen.precision = 'fp32'
        personalize()
        for t, preds in imitator.predict_batches(batches_of(imitator, tgt_smpls, opt), opt.cam_strategy):
            truth[t] = preds
    gen.precision = os.environ.get('LWG_PRECISION', 'auto')      # the generator's own default policy
    personalize()                                          # the source features in the arithmetic under test
    for t, preds in imitator.predict_batches(batches_of(imitator, tgt_smpls, opt), opt.cam_strategy):
        ref = truth[t] if against == 'fp32' else target_batch(tgt_paths[t:t + preds.shape[0]], opt.image_size)
        ev.update(preds, ref)
        if sets is not None:
            sets.update(preds, ref)
    res = ev.result()                                      # the one device->host copy
    out = {'frames': res['frames'], 'ground_truth': 'fp32 generator' if against == 'fp32' else 'target frames',
           'precision': gen.precision, 'quantize': bool(opt.quantize), 'image_size': opt.image_size}
    for k in names:
        out[k] = res[k]
    out['ssim_min'] = float(res['per_frame']['ssim'].min())
    out['psnr_min'] = float(res['per_frame']['psnr'].min())
    if lpips is not None:
        out['lpips_max'] = float(res['per_frame']['lpips'].max())
    if sets is not None:
        scores = sets.result()                             # one device->host copy per feature table, then fp64 on the host
        out['fid'], out['is'], out['is_std'] = scores['fid'], scores['is'], scores['is_std']
    return out


def main():
    opt = EvalOptions().parse()
    torch.cuda.set_device(0)
    out = evaluate(opt)
    line = json.dumps(out)
    if opt.output_dir:
        with open(os.path.join(util.mkdir(opt.output_dir), 'metrics.json'), 'w') as fh:
            fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
