#!/usr/bin/env python
"""Draws the posed SMPL mesh over a sequence: the check of an SMPL estimate by eye (tools/visual_iPER.py of the reference) and
the texture-warping baseline W_T beside Liquid Warping.  Builds no generator.

    python run_mesh.py --synthetic --num_frames 16 --output_dir OUT [--texture_warp]       (seeded synthetic body, no assets)
    python run_mesh.py --tgt_path DIR --output_dir OUT [--hmr_model H.pth] [--src_path S.jpg --texture_warp]

Frames are rendered in blocks of `--batch_size`.  Written to `<output_dir>/meshes/`, pictures in [0,1] as the reference shows
them:
    mesh_%08d.jpg     the posed mesh with debug_textures() under set_ambient_light(), black background;
    masked_%08d.jpg   the frame times the mesh's silhouette;
    wt_%08d.jpg       (--texture_warp) the source's per-face texture, extracted under the source's own mesh, rendered on each
                      target pose.  The source is --src_path, or the first frame.
SMPL parameters: `--synthetic` poses synthetic.body_mesh() by synthetic.motion_verts under synthetic.cams and takes
synthetic.smooth_image(t) as frame t; otherwise every image needs an `<image>.smpl.npy` (85,) beside it, or `--hmr_model`
names a checkpoint of the HMR regressor and the vectors are estimated from the images (Imitator._extract_smpls_batched).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from impersonator_amd.options.jpeg_options import add_jpeg_arguments  # noqa: E402
from impersonator_amd.options.test_options import TestOptions  # noqa: E402
from impersonator_amd.utils import cv_utils, synthetic, util  # noqa: E402
from impersonator_amd.utils.nmr import SMPLRenderer  # noqa: E402


class MeshOptions(TestOptions):
    def initialize(self):
        super().initialize()
        self._parser.add_argument('--texture_warp', action='store_true', default=False,
                                  help="also render the source's extracted texture on every target pose (wt_*.jpg)")
        add_jpeg_arguments(self._parser)


def save_unit_image(chw, path):
    """(3,H,W) or (H,W) array in [0,1] -> JPEG at full quality (the pictures are looked at and compared, not archived)."""
    from PIL import Image
    img = np.clip(np.asarray(chw, np.float32), 0.0, 1.0) * 255.0
    img = img.transpose(1, 2, 0) if img.ndim == 3 else img
    Image.fromarray((img + 0.5).astype(np.uint8)).save(path, quality=100, subsampling=0)


def synthetic_sequence(opt):
    """-> (renderer, verts (n,nv,3), cams (n,3), frames (n,3,is,is) in [0,1]); frame 0 doubles as the source."""
    rest, faces = synthetic.body_mesh()
    render = SMPLRenderer(image_size=opt.image_size, faces=faces, map_fn=synthetic.uv_seg_map_fn(rest, faces),
                          tex_size=opt.tex_size, align_corners=opt.align_corners).cuda()
    n, s = opt.num_frames, opt.image_size
    verts = np.stack([synthetic.motion_verts(rest, t, num_frames=max(n, 1)) for t in range(n)])
    frames = np.concatenate([synthetic.smooth_image(t, (1, 3, s, s)) for t in range(n)]) * 0.5 + 0.5
    return render, torch.from_numpy(verts).cuda(), torch.from_numpy(synthetic.cams(n, seed=0)).cuda(), \
        torch.from_numpy(frames.astype(np.float32)).cuda()


def asset_sequence(opt):
    """Real assets: the frames of --tgt_path (--src_path first when given), their SMPL vectors from `.smpl.npy` files or from
    the HMR regressor, posed by the SMPL model."""
    from run_imitator import _target_smpls, scan_tgt_paths
    from impersonator_amd.models.imitator import Imitator
    paths = ([opt.src_path] if opt.src_path else []) + scan_tgt_paths(opt.tgt_path, itv=1)
    stub = Imitator.__new__(Imitator)          # the SMPL / HMR wiring of Imitator without its generator
    stub._opt = opt
    stub.hmr = stub._create_hmr().cuda()
    smpls = torch.from_numpy(np.asarray(_target_smpls(stub, paths), np.float32)).cuda()
    render = SMPLRenderer(uv_map_path=opt.uv_mapping, map_name=opt.map_name, image_size=opt.image_size, tex_size=opt.tex_size,
                          align_corners=opt.align_corners).cuda()
    verts, cams = [], []
    for s in range(0, len(paths), max(1, opt.batch_size)):
        info = stub.hmr.get_details(smpls[s:s + max(1, opt.batch_size)])
        verts.append(info['verts'])
        cams.append(info['cam'])
    frames = np.stack([cv_utils.transform_img(cv_utils.read_cv2_img(p), opt.image_size, transpose=True) for p in paths])
    return render, torch.cat(verts), torch.cat(cams), torch.from_numpy(frames.astype(np.float32)).cuda()


def main(args=None):
    opt = MeshOptions().parse(args)
    torch.cuda.set_device(0)
    render, verts, cams, frames = synthetic_sequence(opt) if opt.synthetic else asset_sequence(opt)
    first = 1 if (not opt.synthetic and opt.src_path) else 0          # frames before `first` are the source only
    render.set_ambient_light()
    render.set_bgcolor((0, 0, 0))
    white = render.debug_textures().cuda()
    src_tex = render.extract_tex_from_image(frames[0:1], cams[0:1], verts[0:1]) if opt.texture_warp else None
    out_dir = util.mkdir(os.path.join(opt.output_dir, 'meshes'))
    bs = max(1, opt.batch_size)
    for s in range(first, verts.shape[0], bs):
        cam, v, img = cams[s:s + bs].contiguous(), verts[s:s + bs].contiguous(), frames[s:s + bs]
        mesh, _ = render.render(cam, v, white)
        masked = img * render.render_silhouettes(cam, v)[:, None]
        outs = {'mesh': mesh, 'masked': masked}
        if src_tex is not None:
            render.light_intensity_ambient, render.light_intensity_directional = 1, 0     # the texture carries its own shading
            outs['wt'] = render.render(cam, v, src_tex)[0]
            render.set_ambient_light()
        for kind, batch in outs.items():
            if opt.device_jpeg:
                # encoded on the device: the pictures as [-1,1] images, truncated to uint8 as the other drivers' frames are
                streams = util.jpeg_bytes(batch.clamp(0, 1) * 2 - 1, quality=opt.jpeg_quality, subsampling=opt.jpeg_subsampling)
                for k, data in enumerate(streams):
                    with open(os.path.join(out_dir, '%s_%08d.jpg' % (kind, s - first + k)), 'wb') as fh:
                        fh.write(data)
                continue
            batch = batch.cpu().numpy()
            for k in range(batch.shape[0]):
                save_unit_image(batch[k], os.path.join(out_dir, '%s_%08d.jpg' % (kind, s - first + k)))
    print('wrote %d frames to %s' % (verts.shape[0] - first, out_dir))


if __name__ == '__main__':
    main()
