"""Personalisation by fine-tuning on MI355X: the cycle fine-tune of the reference's Imitator.post_personalize
(models/imitator.py:344-472) and the samples it trains on (run_imitator.py:21-163, data/dataset.py:249-324).

`PostTuner` restates the loop body -- two generator passes over ONE parameter set, the second fed with the first's
output image, four loss terms, Adam -- on what models/generator_trainer.py states once for both trainers: the parameter
store (GeneratorParams: device layout, flat parameter / gradient / moment buffers, `first_write`), the two-stream pass
with its hand-written backward over the op-level HIP kernels of liblwg (_TwoStream) and the L1 / BCE loss pieces.
What is new underneath is the data gradient of the 7x7 stems (include/lwg.h, lwg_conv2d_backward_data's few-channel
case): the cycle pass's stems read an image the first pass produced, so the gradient has to go through them.

`meta_samples` builds the training samples on the device, from an Imitator whose source is personalised."""
import torch

from .. import ops
from ..utils import util
from .generator_trainer import GeneratorParams, _TwoStream, _bce, _l1, _nhwc, head_rect


class PostTuner(GeneratorParams):
    """models/imitator.py:344-472 on the device.

        tuner = PostTuner(generator, bg, render)
        for epoch in range(5):
            for sample in samples:
                terms = tuner.optimize(sample)
        generator.load_state_dict(tuner.state_dict())

    `bg` (1,3,H,W): the personalised source's background, a constant (:347).  `render`: its `encode_front_fim` gives the
    front mask (`front_warp`, :378-382) and the back-of-head mask of the structure term (:441).  The optimiser is the
    reference's (:415-417): Adam, lr 2e-4, betas (0.5, 0.999), constant over the five epochs, over ALL generator parameters --
    bg_model.* get no gradient (BGNet does not run), which torch's Adam skips and this one leaves bit-unchanged.
    `face` (networks.facenet.SphereFaceLoss, optional): the `fid` term as a READOUT.  In the reference it carries no gradient:
    FaceLoss.compute_loss detaches its second argument (networks/networks.py:273-286) and post_personalize passes the
    generated image second (:445-446).  It is computed forward-only, when `face` is given, and is not part of `total`'s gradient.

    No BGNet pass, no discriminator, no all-reduce: personalisation runs on one device.
    """

    LR, BETAS, EPS, EPOCHS = 0.0002, (0.5, 0.999), 1e-8, 5       # :415-417; torch.optim.Adam's default eps
    W_CYCLE, W_STRUCT, W_MASK = 10.0, 10.0, 5.0                  # :452

    def __init__(self, generator, bg, render, front_warp=False, conv_precision="fp32", face=None):
        super().__init__(generator, conv_precision)
        self.lr, self.betas, self.eps, self.t = self.LR, self.BETAS, self.EPS, 0
        self.render, self.front_warp, self.face = render, bool(front_warp), face
        dev = self.flat_p.device
        self.bg = _nhwc(torch.as_tensor(bg, dtype=torch.float32).to(dev).reshape((-1, 3) + tuple(bg.shape[-2:])))
        self.first, self.cycle = _TwoStream(self, True), _TwoStream(self, False)
        # the slice of the flat buffers Adam steps on: everything but bg_model.* (a contiguous tail of the state_dict's order)
        tuned = [(k, lo, hi) for k, lo, hi in self._ranges if not (k.startswith("bg_model.") or k == "heads:bg")]
        self._lo = tuned[0][1]
        if [k for k, lo, _ in self._ranges if lo >= self._lo] != [k for k, _, _ in tuned]:
            raise RuntimeError("PostTuner: bg_model's parameters are expected in front of the two streams'")

    # ------------------------------------------------------------------ forward (:350-406)
    @torch.no_grad()
    def forward(self, sample):
        """`sample`: the reference's keys (data/dataset.py:306-322 + preds, run_imitator.py:151), CPU or CUDA tensors.
        -> (fake_src, fake_tsf, cycle_tsf, fake_src_mask, fake_tsf_mask) NCHW."""
        dev = self.flat_p.device
        s = {k: torch.as_tensor(v).to(dev) for k, v in sample.items() if k in (
            "images", "pseudo_masks", "j2d", "T", "T_cycle", "src_inputs", "tsf_inputs", "src_fim", "tsf_fim", "preds")}
        f32 = lambda t: t.float().contiguous()
        self.s = s
        self.src_in, self.tsf_in = _nhwc(f32(s["src_inputs"]), 8), _nhwc(f32(s["tsf_inputs"]), 8)
        self.T, self.T_cycle = f32(s["T"]), f32(s["T_cycle"])
        self.src_real = _nhwc(f32(s["images"][:, 0]))                                  # :429 (images[:, 1] is not read by the loss)
        self.preds = _nhwc(f32(s["preds"]))
        self.pseudo = _nhwc(f32(torch.cat([s["pseudo_masks"][:, 0], s["pseudo_masks"][:, 1]], dim=0)))   # :362-363
        mask_of = lambda fim, front: _nhwc(self.render.encode_front_fim(fim, transpose=True, front_fn=front).float())
        self.back_head = 1 - mask_of(s["tsf_fim"], False)                              # :441
        bg = self.bg
        # first pass (:385-392)
        self.s_img, self.s_mask, self.t_img, self.t_mask = self.first.forward(self.src_in, self.tsf_in, self.T)
        self.fake_src = self.s_mask * bg + (1 - self.s_mask) * self.s_img
        self.fake_tsf = self.t_mask * bg + (1 - self.t_mask) * self.t_img
        if self.front_warp:
            self.fm_t, self.fm_s = mask_of(s["tsf_fim"], True), mask_of(s["src_fim"], True)
            self.fake_tsf = (1 - self.fm_t) * self.fake_tsf + self.tsf_in[..., 0:3] * self.fm_t * (1 - self.t_mask)
        # cycle inputs (:368-376); images travel as 4-channel NHWC through the warp (its kernels take C % 4 == 0)
        self.cyc_warp = ops.grid_sample_nhwc(torch.nn.functional.pad(self.fake_tsf, (0, 1)).contiguous(), self.T_cycle, self.align)[..., 0:3]
        zeros2 = self.fake_tsf.new_zeros(self.fake_tsf.shape[:-1] + (2,))
        cyc_src_in = torch.cat([self.fake_tsf * self.tsf_in[..., 5:6], self.tsf_in[..., 3:6], zeros2], dim=-1).contiguous()
        cyc_tsf_in = torch.cat([self.cyc_warp, self.src_in[..., 3:6], zeros2], dim=-1).contiguous()
        # cycle pass (:397-404)
        _, _, self.c_img, self.c_mask = self.cycle.forward(cyc_src_in, cyc_tsf_in, self.T_cycle)
        self.cyc_tsf = self.c_mask * bg + (1 - self.c_mask) * self.c_img
        if self.front_warp:   # :404: the FIRST pass's source mask
            self.cyc_tsf = (1 - self.fm_s) * self.cyc_tsf + self.src_in[..., 0:3] * self.fm_s * (1 - self.s_mask)
        nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
        return nchw(self.fake_src), nchw(self.fake_tsf), nchw(self.cyc_tsf), nchw(self.s_mask), nchw(self.t_mask)

    # ------------------------------------------------------------------ loss (:433-452) and its gradient
    @torch.no_grad()
    def backward(self):
        """-> the loss terms (device scalars): cycle, struct, mask (unweighted, as the reference logs them), fid when there is a
        face network, and total = 10 cycle + 10 struct + 5 mask (+ fid, a constant as far as the gradient goes)."""
        self.zero_grads()
        bg, bh = self.bg, self.back_head
        # cycle reconstruction (:434)
        c1, d_fake_src = _l1(self.fake_src, self.src_real, self.W_CYCLE)
        c2, d_cyc_tsf = _l1(self.cyc_tsf, self.src_real, self.W_CYCLE)
        # structure (:437-443): the prior's image, and the warped-back body without the back of the head
        body = 1 - self.src_in[..., 5:6]
        s1, d_fake_tsf = _l1(self.fake_tsf, self.preds, self.W_STRUCT)
        s2, d_warp = _l1(self.cyc_warp * bh, self.src_real * body * bh, 2 * self.W_STRUCT)
        d_warp = d_warp * bh
        # masks (:450)
        masks = torch.cat([self.s_mask, self.t_mask], dim=0)
        m_term, d_masks = _bce(masks, self.pseudo, self.W_MASK)
        n = self.s_mask.shape[0]
        d_s_mask, d_t_mask = d_masks[:n], d_masks[n:]
        terms = dict(cycle=(c1 + c2) / self.W_CYCLE, struct=(s1 + s2) / self.W_STRUCT, mask=m_term)
        terms["total"] = c1 + c2 + s1 + s2 + self.W_MASK * m_term
        if self.face is not None:
            terms["fid"] = self._fid()
            terms["total"] = terms["total"] + terms["fid"]
        # --- the cycle pass: blend (and front warp) of its transfer image, then its two streams down to their inputs
        if self.front_warp:
            d_s_mask = d_s_mask - (d_cyc_tsf * self.src_in[..., 0:3] * self.fm_s).sum(-1, keepdim=True)
            d_cyc_tsf = d_cyc_tsf * (1 - self.fm_s)
        dx_src, dx_tsf = self.cycle.backward(None, None, d_cyc_tsf * (1 - self.c_mask),
                                             (d_cyc_tsf * (bg - self.c_img)).sum(-1, keepdim=True), need_dx=True)
        # --- what reaches the first pass's transfer image: the cycle source input's masked copy (:370), the warp (:373, :440)
        d_fake_tsf = d_fake_tsf + dx_src[..., 0:3] * self.tsf_in[..., 5:6]
        d_warp4 = torch.nn.functional.pad(d_warp + dx_tsf[..., 0:3], (0, 1)).contiguous()
        d_fake_tsf = d_fake_tsf + ops.grid_sample_backward(d_warp4, self.T_cycle, tuple(d_warp4.shape), self.align)[..., 0:3]
        if self.front_warp:
            d_t_mask = d_t_mask - (d_fake_tsf * self.tsf_in[..., 0:3] * self.fm_t).sum(-1, keepdim=True)
            d_fake_tsf = d_fake_tsf * (1 - self.fm_t)
        # --- the first pass: blends, then its streams (their inputs are data: no gradient through the stems)
        d_s_mask = d_s_mask + (d_fake_src * (bg - self.s_img)).sum(-1, keepdim=True)
        d_t_mask = d_t_mask + (d_fake_tsf * (bg - self.t_img)).sum(-1, keepdim=True)
        self.first.backward(d_fake_src * (1 - self.s_mask), d_s_mask, d_fake_tsf * (1 - self.t_mask), d_t_mask, need_dx=False)
        self.terms = terms
        return terms

    def _fid(self):
        """:445-446, forward only: the head rectangles are FaceLoss.find_head_rect's (networks/networks.py:336-364) of j2d[:, 0]
        (source) and j2d[:, 1] (prior)."""
        h, w = self.fake_src.shape[1:3]
        j2d = self.s["j2d"].float()
        a = self.face.loss_and_grad(self.cyc_tsf.contiguous(), self.src_real, head_rect(j2d[:, 0], h, w))[0]
        b = self.face.loss_and_grad(self.fake_tsf.contiguous(), self.preds, head_rect(j2d[:, 1], h, w))[0]
        return a + b

    # ------------------------------------------------------------------ Adam (:417, :453-455)
    @torch.no_grad()
    def step(self):
        """One Adam step on the two streams' slice of the flat buffers; bg_model.* (no gradient: torch's Adam skips them) is
        not touched.  No all-reduce: personalisation runs on one device."""
        self.t += 1
        lo = self._lo
        ops.adam_update(self.flat_p[lo:], self.flat_g[lo:], self.flat_m[lo:], self.flat_v[lo:], self.t, self.lr, self.betas, self.eps)

    def optimize(self, sample):
        """forward + loss + backward + Adam (:430-455) -> the terms as floats"""
        self.forward(sample)
        terms = self.backward()
        self.step()
        return {k: float(v) for k, v in terms.items()}

    def gradients(self):
        """Gradients of the last backward pass in the state_dict's layout: the two streams' tensors (bg_model.* has none)."""
        return {k: v for k, v in super().gradients().items() if not k.startswith("bg_model.")}


@torch.no_grad()
def meta_samples(imitator, tgt_paths=None, tgt_smpls=None, cam_strategy='smooth'):
    """The training samples of post_personalize, built on the device from an Imitator whose source is personalised: what the
    reference's meta_imitate + write_pair_info write to pickles and JPEGs (run_imitator.py:21-95) and MetaCycleDataSet /
    PairSampleDataset.preprocess read back (run_imitator.py:98-163, data/dataset.py:249-324).

    One prior frame per entry of `tgt_paths` (pictures; SMPLs from `tgt_smpls` or the HMR regressor) or of `tgt_smpls` alone.
    Per frame, as the reference: `transfer_params(_by_smpl)` + `forward` at t = 0 (meta_imitate calls `inference` with one frame,
    run_imitator.py:81) -> preds; T_cycle = cal_bc_transform(the posed mesh's p2verts with y negated, source fim, source wim)
    (:40-45); pseudo_masks = the two ft_ks erosions (dataset.py:281,287,304); src_inputs / tsf_inputs as `personalize` /
    `transfer` form them (dataset.py:282,293).  -> list of batches of min(len, opt.batch_size) samples, the rest dropped
    (drop_last, run_imitator.py:189-194), every tensor on the device, keys and shapes of the reference's loader.

    Two deviations: `preds` are the device's float images, not JPEGs written and read back (8-bit, lossy); `images[:, 1]` is
    the target picture when there is one, else the source (no loss term reads it, imitator.py:429)."""
    if imitator.src_info is None:
        raise RuntimeError("meta_samples: personalize a source first")
    opt, src, render = imitator._opt, imitator.src_info, imitator.render
    n = len(tgt_paths) if tgt_paths else len(tgt_smpls)
    src_crop = util.morph(src['cond'][:, -1:, :, :], ks=opt.ft_ks, mode='erode')
    rows = []
    for t in range(n):
        path = tgt_paths[t] if tgt_paths else None
        smpl = None if tgt_smpls is None else tgt_smpls[t]
        if path:
            tsf_inputs = imitator.transfer_params(path, smpl, cam_strategy=cam_strategy, t=0)
        else:
            tsf_inputs = imitator.transfer_params_by_smpl(smpl, cam_strategy=cam_strategy, t=0)
        tsf = imitator.tsf_info
        preds = imitator.forward(tsf_inputs, tsf['T'])
        f2verts, _, _ = render.render_fim_wim(tsf['cam'], tsf['verts'])
        T_cycle = render.cal_bc_transform(render.source_p2verts(f2verts), src['fim'], src['wim'])
        tsf_crop = util.morph(tsf['cond'][:, -1:, :, :], ks=opt.ft_ks, mode='erode')
        tgt_img = imitator._load_image(path, opt.image_size)[0] if path else src['img']
        rows.append(dict(images=torch.stack([src['img'][0], tgt_img[0]]), pseudo_masks=torch.stack([src_crop[0], tsf_crop[0]]),
                         j2d=torch.cat([src['j2d'], tsf['j2d']], dim=0), T=tsf['T'][0], T_cycle=T_cycle[0],
                         src_inputs=src['src_inputs'][0], tsf_inputs=tsf_inputs[0], src_fim=src['fim'][0].float(),
                         tsf_fim=tsf['fim'][0].float(), preds=preds[0]))
    bs = min(n, max(1, int(opt.batch_size)))
    return [{k: torch.stack([r[k] for r in rows[i:i + bs]]).contiguous() for k in rows[0]} for i in range(0, n - bs + 1, bs)]
