"""Animator (appearance transfer driven by a motion sequence) on MI355X.

The reference ships a `models/animator.py` with `animate_setup(src, ref)` / `animate(img_paths, smpls)`, but that class is dead
code: it builds `SMPLRenderer(faces=..., tex_size=..., has_front_map=True)`, calls `render.forward(..., is_uv_sampler=False,
reverse_yz=True)` and indexes ten part channels out of `encode_front_fim`, none of which its own utils/nmr.py provides, so it cannot
be run, let alone serve as an oracle.  What is kept from it are the method names and `PART_IDS`.  The semantics are those of
`Swapper.swap` (models/swapper.py:198-253) with the source's own raster maps replaced by the driven pose's:

    once per (pair, target_part)
        left_faces = faces of the parts that stay the source's
        ref_f2p    = the reference's face vertices with left_faces sent to -2          (Swapper._flow_through_kept_faces)
        src_f2p    = the source's face vertices with every OTHER face sent to -2
    per frame (a batch of n target SMPL vectors)
        theta, cam, verts  as Imitator.transfer_params_by_smpl (swap_smpl under the source's camera and shape)
        fim, wim           = render_fim_wim(cam, verts)
        cond, part         = map_fn[fim], part_fn[fim];   part_mask / left_mask = (sum of the selected / kept part channels != 0)
        T_ref, T_src       = clamp(cal_bc_transform(ref_f2p | src_f2p, fim, wim), -2, 2)
        tsf_img            = grid_sample(ref_img, T_ref) * part_mask + grid_sample(src_img, T_src) * left_mask
        pred               = generator.swap(cat(tsf_img, cond), ref feats, src feats, T_ref, T_src, bg = the source's)

so the source goes through a real flow where `Swapper.swap` uses the identity grid.  Everything after the rasteriser is ONE launch
(lwg_animate_inputs, csrc/animate.hip); `Animator(fused=False)` runs the chain of existing entries instead -- same bits, the
comparison for tests and timing.  Batching, lanes, fused launch sequences and graph replay are Imitator's (`predict_batches`,
`frame_graph`): the second flow travels through them as a named per-frame tensor (`FORWARD_KEYS`).
"""
import os

import numpy as np
import torch

from ..utils import cv_utils
from .imitator import Imitator
from .swapper import Swapper


def side_table(part_fn, selected_ids, left_ids):
    """(nf+1,) uint8, one entry per row of `part_fn` (nf+1, nparts[+1]), the background row included: bit 0 = the row's selected
    channels sum to non-zero, bit 1 = its kept channels do.  part = part_fn[fim], so these are the per-pixel part_mask / left_mask
    of models/swapper.py:206-207 looked up by face."""
    tab = np.asarray(part_fn, np.float32)
    sel = tab[:, list(selected_ids)].sum(1) != 0 if len(selected_ids) else np.zeros(tab.shape[0], bool)
    left = tab[:, list(left_ids)].sum(1) != 0 if len(left_ids) else np.zeros(tab.shape[0], bool)
    return (sel.astype(np.uint8) | (left.astype(np.uint8) << 1)).astype(np.uint8)


def left_face_flags(part_faces, left_ids, nf):
    """(nf,) uint8: 1 for the faces of the kept parts (left_faces of models/swapper.py:208 as one byte per face)."""
    keep = np.zeros(nf, np.uint8)
    for i in left_ids:
        keep[np.asarray(part_faces[i], np.int64)] = 1
    return keep


class Animator(Swapper):
    PART_IDS = {
        'body': [1, 2, 3, 4, 5, 6, 7, 8, 9],
        'upper_body': [1, 2, 3, 4, 9],
        'lower_body': [4, 5],
        'torso': [9],
        'all': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    }
    PER_FRAME_KEYS = Imitator.PER_FRAME_KEYS + ('T_ref',)
    FORWARD_KEYS = ('T_ref',)

    def __init__(self, opt, fused=True, **kwargs):
        """`fused=False`: the per-frame geometry as the chain of existing liblwg entries plus the mask-and-compose expression in
        torch instead of lwg_animate_inputs (same values, bit for bit)."""
        super().__init__(opt, **kwargs)
        self._name = 'Animator'
        self.fused = bool(fused)
        self.ref_info = None
        self.target_part = getattr(opt, 'swap_part', 'body')
        self._pair_cache = {}

    # ------------------------------------------------------------------ once per pair
    @torch.no_grad()
    def animate_setup(self, src_path, ref_path, src_smpl=None, ref_smpl=None, output_dir='', src_bg=None, ref_bg=None):
        """Personalises both subjects exactly as Swapper.personalize does: `src_info` is the person who moves (camera, shape,
        background, the kept parts), `ref_info` the one whose parts are put on."""
        self._pair_cache = {}
        out = lambda name: os.path.join(output_dir, name) if output_dir else ''
        self.src_info = self.personalize(src_path, src_smpl, output_path=out('src.jpg'), bg_img=src_bg)
        self.ref_info = self.personalize(ref_path, ref_smpl, output_path=out('ref.jpg'), bg_img=ref_bg)
        self.tsf_info = None

    def set_target_part(self, target_part):
        assert target_part in self.PART_IDS.keys()
        self.target_part = target_part

    def _pair_tables(self, target_part):
        """dict(selected_ids, left_ids, side, ref_f2p, src_f2p) of the personalised pair and `target_part`, built once."""
        from .. import _lib
        if target_part not in self._pair_cache:
            if self.src_info is None or self.ref_info is None:
                raise RuntimeError("Animator: animate_setup a source and a reference first")
            lib = _lib.load()
            selected_ids = self.PART_IDS[target_part]
            left_ids = [i for i in self.PART_IDS['all'] if i not in selected_ids]
            keep = left_face_flags(self.part_faces, left_ids, self.render.nf)
            dev = self.src_info['img'].device
            tables = dict(selected_ids=selected_ids, left_ids=left_ids,
                          side=torch.from_numpy(side_table(self.part_fn.cpu().numpy(), selected_ids, left_ids)).to(dev))
            for name, info, drop in (('ref_f2p', self.ref_info, keep), ('src_f2p', self.src_info, 1 - keep)):
                p2v = info.get('p2verts_c')
                if p2v is None:
                    p2v = info['p2verts'].float().contiguous()
                out = torch.empty_like(p2v)
                flags = torch.from_numpy(np.ascontiguousarray(drop, np.uint8)).to(dev)
                _lib.check(lib.lwg_mask_faces(_lib.ptr(p2v), _lib.ptr(flags), p2v.shape[1], 6, _lib.ptr(out), _lib.stream_ptr()))
                tables[name] = out
            self._pair_cache[target_part] = tables
        return self._pair_cache[target_part]

    # ------------------------------------------------------------------ per frame
    def _chain_inputs(self, fim, wim, tab):
        """The per-frame geometry as the chain lwg_animate_inputs replaces: encode_fim x2, the two masks, cal_bc_transform x2,
        clamp x2, grid_sample x2, compose, cat."""
        from .. import _lib
        lib, r = _lib.load(), self.render
        cond = r._lookup(fim, r.map_fn, True)
        part = r._lookup(fim, self.part_fn, True)
        part_mask = (torch.sum(part[:, tab['selected_ids']], dim=1, keepdim=True) != 0).float()
        left_mask = (torch.sum(part[:, tab['left_ids']], dim=1, keepdim=True) != 0).float()
        flows = []
        for f2p in (tab['ref_f2p'], tab['src_f2p']):
            T = r.cal_bc_transform(f2p, fim, wim)
            _lib.check(lib.lwg_clamp(_lib.ptr(T), T.numel(), -2.0, 2.0, _lib.stream_ptr()))
            flows.append(T)
        T_ref, T_src = flows
        tsf_img = r.grid_sample(self.ref_info['img'], T_ref) * part_mask + r.grid_sample(self.src_info['img'], T_src) * left_mask
        return dict(cond=cond, T_src=T_src, T_ref=T_ref, tsf_img=tsf_img, tsf_inputs=torch.cat([tsf_img, cond], dim=1))

    @torch.no_grad()
    def transfer_params_by_smpl(self, tgt_smpl, cam_strategy='smooth', t=0):
        """One frame (85,) or a batch (n,85): sets self.tsf_info (the Imitator keys; 'T' is T_src, 'T_ref' is added), returns
        tsf_inputs."""
        tab = self._pair_tables(self.target_part)
        tsf_info = self._posed_details(tgt_smpl, cam_strategy, t)
        _, fim, wim = self.render.render_fim_wim(tsf_info['cam'], tsf_info['verts'])
        if self.fused:
            out = self.render.animate_inputs(fim, wim, tab['side'], tab['src_f2p'], tab['ref_f2p'], self.src_info['img'],
                                             self.ref_info['img'])
        else:
            out = self._chain_inputs(fim, wim, tab)
        tsf_info['fim'] = fim
        tsf_info['wim'] = wim
        tsf_info['cond'] = out['cond']
        tsf_info['tsf_img'] = out['tsf_img']
        tsf_info['T'] = out['T_src']
        tsf_info['T_ref'] = out['T_ref']
        self.tsf_info = tsf_info
        return out['tsf_inputs']

    @torch.no_grad()
    def forward(self, tsf_inputs, *args, generator=None, T_ref=None):
        """forward(tsf_inputs, T, generator=None, T_ref=None) -> preds: the two-stream generator over the reference's and the
        source's cached features with the blend onto the source's background fused; T is T_src, T_ref defaults to
        tsf_info['T_ref'] (what `frame_graph` relies on).  With Swapper.forward's six positional arguments (what the inherited
        `swap` passes) it is Swapper.forward."""
        if len(args) == 5:
            return Swapper.forward(self, tsf_inputs, *args)
        (T,) = args
        generator = self.generator if generator is None else generator
        T_ref = self.tsf_info['T_ref'] if T_ref is None else T_ref
        ref_enc, ref_res = self.ref_info['feats']
        src_enc, src_res = self.src_info['feats']
        preds, _, mask = generator.swap(tsf_inputs, ref_enc, src_enc, ref_res, src_res, T_ref, T, bg_img=self.src_info['bg'])
        if self._opt.front_warp:
            preds = Imitator.warp_front(self, preds, mask)
        return preds

    @torch.no_grad()
    def transfer(self, tgt_smpl, cam_strategy='smooth', t=0):
        """One batch of target SMPL vectors -> preds (n,3,is,is), with `self.target_part`."""
        tsf_inputs = self.transfer_params_by_smpl(tgt_smpl, cam_strategy, t)
        return self.forward(tsf_inputs, self.tsf_info['T'])

    @torch.no_grad()
    def animate(self, tgt_paths, tgt_smpls=None, cam_strategy='smooth', target_part='body', output_dir='', visualizer=None,
                device_jpeg=False, jpeg_quality=75, jpeg_subsampling='4:2:0'):
        """-> list of (H,W,3) float arrays in [-1,1], like Imitator.inference: the frames in batches of `opt.batch_size` through
        `predict_batches`.  Without `tgt_smpls` the SMPL vectors come from the HMR regressor (needs an --hmr_model checkpoint)."""
        self.set_target_part(target_part)
        if tgt_smpls is None:
            if not self._has_regressor():
                raise NotImplementedError("estimating SMPL from target images needs the HMR regressor; pass tgt_smpls")
            tgt_smpls = self._extract_smpls_batched(list(tgt_paths))

        def sink(t, pred, pred_dev):
            if visualizer is not None:
                visualizer.vis_named_img('pred_' + cam_strategy, pred_dev)
            if output_dir:
                filename = os.path.split(tgt_paths[t])[-1] if tgt_paths and tgt_paths[t] else '%.8d.jpg' % t
                cv_utils.save_cv2_img(pred, os.path.join(output_dir, 'pred_' + filename), normalize=True)

        if device_jpeg and output_dir:
            # the frames are encoded on the device and written under the same names; the written paths are returned
            name = lambda t: 'pred_' + (self._jpg_name(os.path.split(tgt_paths[t])[-1]) if tgt_paths and tgt_paths[t]
                                        else '%.8d.jpg' % t)
            return self._run_batches(tgt_smpls, cam_strategy, None, self._jpeg_sink(output_dir, name, visualizer, cam_strategy),
                                     dict(quality=jpeg_quality, subsampling=jpeg_subsampling))
        return self._run_batches(tgt_smpls, cam_strategy, sink)
