"""Personalisation by fine-tuning on MI355X: the cycle fine-tune of the reference's Imitator.post_personalize
(models/imitator.py:344-472) and the samples it trains on (run_imitator.py:21-163, data/dataset.py:249-324).

`PostTuner` restates the loop body -- two generator passes over ONE parameter set, the second fed with the first's
output image, four loss terms, Adam -- on what models/generator_trainer.py states once for both trainers: the parameter
store (GeneratorParams: device layout, flat parameter / gradient / moment buffers, `first_write`), the two-stream pass
with its hand-written backward over the op-level HIP kernels of liblwg (_TwoStream) and the L1 / BCE loss pieces.
What is new underneath is the data gradient of the 7x7 stems (include/lwg.h, lwg_conv2d_backward_data's few-channel
case): the cycle pass's stems read an image the first pass produced, so the gradient has to go through them.

`meta_samples` builds the training samples on the device, from an Imitator whose source is personalised.

`SwapTuner` is the Swapper's fine-tune (models/swapper.py:273-476) on the same two passes and the same backward: a background per
sample, no back-of-head mask, its own face pairs, and 50 iterations on ONE batch of two with a decaying learning rate.  Step
count, rate table and loss history live on the device (ops.adam_update_scheduled), so the iteration is captured once as a HIP
graph and replayed.  `swap_samples` builds that batch from a Swapper after swap_setup."""
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
    # what `load` leaves on the tuner: one batch in device layout, everything the two passes and the loss read besides the parameters
    DATA = ("src_in", "tsf_in", "T", "T_cycle", "src_real", "preds", "pseudo", "j2d", "back_head", "fm_t", "fm_s")

    @torch.no_grad()
    def load(self, sample):
        """`sample`: the reference's keys (data/dataset.py:306-322 + preds, run_imitator.py:151), CPU or CUDA tensors -> the
        `DATA` attributes: NHWC float32 on the device, the masks looked up through the renderer."""
        dev = self.flat_p.device
        s = {k: torch.as_tensor(v).to(dev) for k, v in sample.items() if k in (
            "images", "pseudo_masks", "j2d", "T", "T_cycle", "src_inputs", "tsf_inputs", "src_fim", "tsf_fim", "preds")}
        f32 = lambda t: t.float().contiguous()
        self.src_in, self.tsf_in = _nhwc(f32(s["src_inputs"]), 8), _nhwc(f32(s["tsf_inputs"]), 8)
        self.T, self.T_cycle = f32(s["T"]), f32(s["T_cycle"])
        self.src_real = _nhwc(f32(s["images"][:, 0]))                                  # :429 (images[:, 1] is not read by the loss)
        self.preds = _nhwc(f32(s["preds"]))
        self.pseudo = _nhwc(f32(torch.cat([s["pseudo_masks"][:, 0], s["pseudo_masks"][:, 1]], dim=0)))   # :362-363
        self.j2d = f32(s["j2d"])
        mask_of = lambda fim, front: _nhwc(self.render.encode_front_fim(fim, transpose=True, front_fn=front).float())
        self.back_head = self._back_head(mask_of, s)
        self.fm_t, self.fm_s = (mask_of(s["tsf_fim"], True), mask_of(s["src_fim"], True)) if self.front_warp else (None, None)

    def _back_head(self, mask_of, s):
        """the mask of the structure term's second half (:441), or None for no mask"""
        return 1 - mask_of(s["tsf_fim"], False)

    @torch.no_grad()
    def passes(self):
        """The two generator passes over the loaded batch -> (fake_src, fake_tsf, cycle_tsf, fake_src_mask, fake_tsf_mask) NCHW."""
        bg = self.bg
        # first pass (:385-392)
        self.s_img, self.s_mask, self.t_img, self.t_mask = self.first.forward(self.src_in, self.tsf_in, self.T)
        self.fake_src = self.s_mask * bg + (1 - self.s_mask) * self.s_img
        self.fake_tsf = self.t_mask * bg + (1 - self.t_mask) * self.t_img
        if self.front_warp:   # :378-382
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

    def forward(self, sample):
        """`load(sample)` + `passes()` -> (fake_src, fake_tsf, cycle_tsf, fake_src_mask, fake_tsf_mask) NCHW."""
        self.load(sample)
        return self.passes()

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
        if bh is None:
            s2, d_warp = _l1(self.cyc_warp, self.src_real * body, 2 * self.W_STRUCT)
        else:
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
        a = self.face.loss_and_grad(self.cyc_tsf.contiguous(), self.src_real, head_rect(self.j2d[:, 0], h, w))[0]
        b = self.face.loss_and_grad(self.fake_tsf.contiguous(), self._fid_prior(), head_rect(self.j2d[:, 1], h, w))[0]
        return a + b

    def _fid_prior(self):
        """what the transfer image is compared with in the face term (:446): the prior's image"""
        return self.preds

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


class SwapTuner(PostTuner):
    """models/swapper.py:273-476 on the device: PostTuner's two passes, loss and backward, with the Swapper's differences.

        tuner = SwapTuner(generator, bg, render, batch_size=opt.batch_size)
        tuner.load(swap_samples(swapper))
        history = tuner.run()
        generator.load_state_dict(tuner.state_dict())

    `bg` (2,3,H,W) = [src_info['bg'], tsf_info['bg']] (:277): a background per sample.  The structure term has no back-of-head
    mask (:436-442).  `fid` (:444-445), a readout as in PostTuner, compares (src_imgs, cycle_tsf; j2d[:, 0]) and
    (tsf_inputs[:, 0:3], fake_tsf; j2d[:, 1]): the WARPED source, not the prior's image.  At bs == 1 the reference crops with row
    0's key points whichever sample runs (`j2ds[:, 0]` of the whole batch, :444); here the running sample's own row is used.
    Batch rule (:275, :409-428): bs = 2 if batch_size > 1 else 1; at bs == 1 step s trains on sample s % 2 with
    pseudo_masks[i:4:2].

    The learning rate (:391-395, :473-474) is `lr_schedule`, a table on the device next to Adam's step count; the four terms of
    every step go to row `step count` of `history` (total, 4) before the Adam step.  Nothing about a step is host state that a
    kernel reads, so `optimize_graphed` captures ONE iteration and replays it through all rate changes; `optimize` is the same
    iteration launched eagerly, without a float read-back.  `terms_history()` is the one read-back, after the loop."""

    TOTAL, FIX, LR_FINAL = 50, 25, 0.00001                       # :391-395
    TERMS = ("cycle", "struct", "mask", "total")                # columns of `history`
    # run(): the eager loop.  Replays measured 0-2 % SLOWER at 256x256 (profiles/swap_tune.md: 20-60 ms of kernels per iteration,
    # not launch-bound)
    GRAPH = False

    def __init__(self, generator, bg, render, front_warp=False, conv_precision="fp32", face=None, batch_size=2, total=TOTAL, fix=FIX):
        super().__init__(generator, bg, render, front_warp=front_warp, conv_precision=conv_precision, face=face)
        if self.bg.shape[0] != 2:
            raise ValueError("SwapTuner: bg is (2,3,H,W), the two subjects' backgrounds")
        dev = self.flat_p.device
        self.bs, self.total, self.bg_pair = (2 if int(batch_size) > 1 else 1), int(total), self.bg   # :275
        self.lr_table = torch.tensor(self.lr_schedule(total, fix, self.LR, self.LR_FINAL), dtype=torch.float32, device=dev)
        self.step_state = ops.adam_step_state(0, self.betas, dev)
        self.history = torch.zeros((self.total, len(self.TERMS)), device=dev)
        self.fids, self.rows = [], None
        self._graph = self._graph_terms = self._static = None
        self._graph_failed, self._graph_warm, self.captures, self.replays = False, 0, 0, 0

    @staticmethod
    def lr_schedule(total=TOTAL, fix=FIX, init=0.0002, final=0.00001):
        """The rate each step USES, by the reference's own repeated subtraction: the rate drops by (init - final) / fix after
        every step > fix (:473-474, :382-389).  50 steps: 2e-4 for steps 0..26, 1.924e-4 at 27, ... 2.52e-5 at 49."""
        cur, rates = init, []
        for step in range(int(total)):
            rates.append(cur)
            if step > fix:
                cur -= (init - final) / fix
        return rates

    def _back_head(self, mask_of, s):
        return None                                              # :441-442: the whole warped-back body

    def _fid_prior(self):
        return self.tsf_in[..., 0:3].contiguous()                # :445

    # ------------------------------------------------------------------ the batch (:402-428)
    @torch.no_grad()
    def load(self, sample):
        """The batch of two (`swap_samples`) in device layout, and the rows the steps train on: the batch itself at bs == 2, its
        two samples in turn at bs == 1 (:409-421)."""
        self.bg = self.bg_pair
        super().load(sample)
        if self.src_in.shape[0] != 2:
            raise ValueError("SwapTuner trains on the batch of two subjects, got %d samples" % self.src_in.shape[0])
        whole = {k: getattr(self, k) for k in self.DATA + ("bg",) if getattr(self, k) is not None}
        if self.bs == 2:
            self.rows = [whole]
        else:   # pseudo is cat([source masks, transfer masks]): sample i's pair is rows i and 2 + i (:421)
            self.rows = [{k: (v[i:4:2] if k == "pseudo" else v[i:i + 1]).contiguous() for k, v in whole.items()} for i in (0, 1)]
        self._use(self.rows[0])

    def _use(self, row):
        for k, v in row.items():
            setattr(self, k, v)

    def _next_row(self):
        if self.rows is None:
            raise RuntimeError("SwapTuner: load(sample) first")
        if self.t >= self.total:
            raise RuntimeError("SwapTuner: the learning-rate table has %d entries and %d steps are taken" % (self.total, self.t))
        return self.rows[self.t % len(self.rows)]

    # ------------------------------------------------------------------ one iteration (:429-455)
    @torch.no_grad()
    def step(self):
        """Adam with step count and rate on the device; bg_model.* is not touched"""
        lo = self._lo
        ops.adam_update_scheduled(self.flat_p[lo:], self.flat_g[lo:], self.flat_m[lo:], self.flat_v[lo:], self.step_state, self.lr_table,
                                  self.betas, self.eps)

    @torch.no_grad()
    def _iteration(self):
        self.passes()
        terms = self.backward()
        # row = the count BEFORE this step's advance, read on the device
        self.history.index_copy_(0, self.step_state[0:1], torch.stack([terms[k] for k in self.TERMS]).reshape(1, -1))
        self.step()
        return terms

    def optimize(self, sample=None):
        """One eager iteration -> the terms as device scalars (no read-back)."""
        if sample is not None:
            self.load(sample)
        self._use(self._next_row())
        terms = self._iteration()
        if "fid" in terms:
            self.fids.append(terms["fid"])
        self.t += 1
        return terms

    def optimize_graphed(self, warmup=2, strict=False):
        """`optimize()` as one launch: the first `warmup` calls run eagerly (every lazily created buffer, handle and kernel attribute
        exists afterwards), the next captures the iteration in a HIP graph and every call from then on replays it.  The graph reads
        PRIVATE static copies of the row; at bs == 1 the next sample is copied into them before each replay (one graph, not two).
        A failed capture falls back to eager iterations for good, with a warning; `strict` (or env LWG_GRAPH_STRICT=1) re-raises.
        With a face readout (host-side crops) every call is eager."""
        import os
        if self.face is not None or self._graph_failed:
            return self.optimize()
        if self._graph is None:
            if self._graph_warm < warmup:
                self._graph_warm += 1
                return self.optimize()
            row = self._next_row()
            try:
                self._static = {k: v.detach().clone() for k, v in row.items()}
                self._use(self._static)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    terms = self._iteration()
                failed = None
            except RuntimeError as e:   # what a capture can trip over is reported as RuntimeError (LwgError is one)
                failed = e
            if failed is not None:
                if strict or os.environ.get("LWG_GRAPH_STRICT") == "1":
                    raise failed
                import warnings
                warnings.warn("SwapTuner.optimize_graphed: capture failed (%s: %s); continuing with eager iterations"
                              % (type(failed).__name__, failed))
                self._graph_failed, self._static = True, None
                torch.cuda.synchronize()
                return self.optimize()
            self._graph, self._graph_terms = graph, terms
            self.captures += 1
        row = self._next_row()
        if len(self.rows) > 1:
            for k, v in row.items():
                self._static[k].copy_(v)
        self._graph.replay()
        self.replays += 1
        self.t += 1
        return self._graph_terms

    def run(self, graphed=None, on_step=None):
        """The remaining steps -> `terms_history()`.  `graphed` (default GRAPH) takes `optimize_graphed`; a face readout forces the
        eager loop.
        `on_step(step, tuner)` is called after every step (the images of that step are the tuner's attributes)."""
        graphed = (self.GRAPH if graphed is None else bool(graphed)) and self.face is None
        while self.t < self.total:
            step = self.t
            if graphed:
                self.optimize_graphed()
            else:
                self.optimize()
            if on_step is not None:
                on_step(step, self)
        return self.terms_history()

    def terms_history(self):
        """The terms of the steps taken so far as floats: one read-back of `history` (and of the fid readouts)."""
        out = [dict(zip(self.TERMS, r)) for r in self.history[:self.t].cpu().tolist()]
        if self.fids:
            for o, f in zip(out, torch.stack(self.fids).cpu().tolist()):
                o["fid"] = f
        return out


@torch.no_grad()
def swap_samples(swapper):
    """The batch Swapper.post_personalize trains on, built on the device from a Swapper after swap_setup: the reference's
    set_inputs / initialize (models/swapper.py:279-329) in the keys and layout PostTuner.load reads, plus 'bg' (:277).

    Sample 0: src is the source, tsf the target pose; sample 1: the roles exchanged.  Per sample T = cal_bc_transform(source
    p2verts, target fim, target wim), tsf_img = transform(source img, T), tsf_inputs = cat(tsf_img, target cond), preds =
    inference(source feats, tsf_inputs, T) blended with the source's bg (through Swapper.warp under --front_warp); T_cycle is T
    with the rows exchanged; pseudo_masks are the ft_ks erosions of the last channel of src_inputs / tsf_inputs; j2d = [own,
    other's].  images[:, 1] is the other subject's picture (no loss term reads it)."""
    a, b = swapper.src_info, swapper.tsf_info
    if a is None or b is None or 'src_inputs' not in b:
        raise RuntimeError("swap_samples: swap_setup first")
    opt, render, gen = swapper._opt, swapper.render, swapper.generator

    def initialize(src, tsf):                                                            # :280-300
        p2v = src.get('p2verts_c')
        if p2v is None:
            p2v = src['p2verts'].float().contiguous()
        T = render.cal_bc_transform(p2v, tsf['fim'], tsf['wim'])
        tsf_img = gen.transform(src['img'], T)
        tsf_inputs = torch.cat([tsf_img, tsf['cond'].float()], dim=1)
        enc, res = src['feats']
        preds, _, mask = gen.inference(enc, res, tsf_inputs, T, bg_img=src['bg'])
        if opt.front_warp:
            preds = swapper.warp(preds, tsf_img, tsf['fim'], mask)
        return preds, T, tsf_inputs

    pa, Ta, ia = initialize(a, b)
    pb, Tb, ib = initialize(b, a)
    pair = lambda k: torch.cat([a[k], b[k]], dim=0).float()
    both = lambda t: torch.stack([t, t.flip(0)], dim=1)                                  # [own, other's]
    T, src_inputs, tsf_inputs, fim = torch.cat([Ta, Tb], dim=0), pair('src_inputs'), torch.cat([ia, ib], dim=0), pair('fim')
    erode = lambda x: util.morph(x[:, -1:], ks=opt.ft_ks, mode='erode')                  # :324-325
    return dict(images=both(pair('img')), pseudo_masks=torch.stack([erode(src_inputs), erode(tsf_inputs)], dim=1),
                j2d=both(pair('j2d')), T=T, T_cycle=T.flip(0).contiguous(), src_inputs=src_inputs, tsf_inputs=tsf_inputs,
                src_fim=fim, tsf_fim=fim.flip(0).contiguous(), preds=torch.cat([pa, pb], dim=0), bg=pair('bg'))


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
