"""CPU autograd restatement of ONE iteration of the reference's Imitator.post_personalize (models/imitator.py:344-472),
composed from oracle.torch_ref -- what the device's PostTuner (impersonator_amd/models/post_tune.py) is held to.  Helper
module, no tests of its own (tests/test_post_tune_oracle.py checks it, tests/test_gpu_post_tune.py uses it).

The masks the reference looks up through its renderer (`encode_front_fim`, utils/nmr.py:343-352) come in as tensors:
`back_head` = 1 - encode_front_fim(tsf_fim, front_fn=False) (imitator.py:441), `front` = the pair of front masks of
tsf_fim and src_fim (imitator.py:379) or None without --front_warp."""
import torch
import torch.nn.functional as F

from oracle import torch_ref


def find_head_rect(kps, height, width):
    """networks/networks.py:336-365."""
    kps = (kps + 1) / 2.0                                                        # :339
    zeros, ones = torch.zeros_like(kps[:, 12, 0]), torch.ones_like(kps[:, 12, 0])   # :341-343
    min_x = torch.max(torch.min(kps[:, 12:, 0] - 0.05, dim=1)[0], zeros)         # :346-347
    max_x = torch.min(torch.max(kps[:, 12:, 0] + 0.05, dim=1)[0], ones)          # :349-350
    min_y = torch.max(torch.min(kps[:, 12:, 1] - 0.05, dim=1)[0], zeros)         # :353-354
    max_y = torch.min(torch.max(kps[:, 12:, 1], dim=1)[0], ones)                 # :356-357
    return torch.stack(((min_x * width).long(), (max_x * width).long(), (min_y * height).long(), (max_y * height).long()), dim=1)   # :359-365


def face_term(fsd, imgs1, imgs2, kps):
    """FaceLoss.forward with kps1 = kps2 (networks/networks.py:243-261) + compute_loss (:273-286): the SECOND argument is
    detached (:284)."""
    rects = find_head_rect(kps, imgs1.shape[2], imgs1.shape[3])                  # :321
    f1 = torch_ref.sphere20a_features(fsd, torch_ref.crop_head_bbox(imgs1, rects))   # :324-330, :280
    f2 = torch_ref.sphere20a_features(fsd, torch_ref.crop_head_bbox(imgs2, rects))
    return sum(F.l1_loss(a, b.detach()) for a, b in zip(f1, f2))                 # :282-284


def preprocess(images, fims_enc, T, ft_ks=3):
    """PairSampleDataset.preprocess (data/dataset.py:269-304) for one pair, the fields post_personalize reads: images (2,3,h,w),
    fims_enc (2,3,h,w) (the last channel is the background mask), T (h,w,2) -> dict(src_inputs, tsf_inputs, pseudo_masks)."""
    src_fim, src_img = fims_enc[0], images[0]                                    # :274-275
    src_crop = torch_ref.morph(src_fim[None, -1:], ft_ks, "erode")[0]            # :276, :281
    src_inputs = torch.cat([src_img * (1 - src_crop), src_fim])                  # :282
    tsf_fim = fims_enc[1]                                                        # :285
    tsf_crop = torch_ref.morph(tsf_fim[None, -1:], ft_ks, "erode")[0]            # :286-287
    warp = torch_ref.grid_sample(src_img[None], T[None])[0]                      # :290
    tsf_inputs = torch.cat([warp, tsf_fim], dim=0)                               # :293
    return dict(src_inputs=src_inputs, tsf_inputs=tsf_inputs, pseudo_masks=torch.stack([src_crop, tsf_crop], dim=0))   # :304


def step_loss(sd, sample, bg, back_head, front=None, cut_cycle=False, fsd=None, align_corners=False):
    """imitator.py:424-452 -> (total, terms, images).  `cut_cycle`: fake_tsf detached in both cycle inputs -- NOT the
    reference, the counterfactual that shows whether a gradient went through the cycle pass."""
    src_inputs, tsf_inputs, T, T_cycle = sample["src_inputs"], sample["tsf_inputs"], sample["T"], sample["T_cycle"]   # :351-355
    images = torch.cat([sample["images"][:, 0], sample["images"][:, 1]], dim=0)                       # :360
    pseudo_masks = torch.cat([sample["pseudo_masks"][:, 0], sample["pseudo_masks"][:, 1]], dim=0)     # :362-363
    init_preds, j2ds = sample["preds"], sample["j2d"]                                                 # :358, :351
    bs = tsf_inputs.shape[0]                                                                          # :428
    src_imgs = images[0:bs]                                                                           # :429

    def warp(preds, tsf, front_mask, mask):                                                           # :378-382
        return (1 - front_mask) * preds + tsf * front_mask * (1 - mask)

    fake_src_color, fake_src_mask, fake_tsf_color, fake_tsf_mask = torch_ref.generator_infer_front(
        sd, src_inputs, tsf_inputs, T, align_corners)                                                 # :385-386
    fake_src_imgs = fake_src_mask * bg + (1 - fake_src_mask) * fake_src_color                         # :388
    fake_tsf_imgs = fake_tsf_mask * bg + (1 - fake_tsf_mask) * fake_tsf_color                         # :389
    if front is not None:
        fake_tsf_imgs = warp(fake_tsf_imgs, tsf_inputs[:, 0:3], front[0], fake_tsf_mask)              # :391-392
    fed = fake_tsf_imgs.detach() if cut_cycle else fake_tsf_imgs
    cycle_src_inputs = torch.cat([fed * tsf_inputs[:, -1:], tsf_inputs[:, 3:]], dim=1)                # :370
    cycle_tsf_inputs = torch.cat([torch_ref.grid_sample(fed, T_cycle, align_corners), src_inputs[:, 3:]], dim=1)   # :373-374
    _, _, cycle_tsf_color, cycle_tsf_mask = torch_ref.generator_infer_front(
        sd, cycle_src_inputs, cycle_tsf_inputs, T_cycle, align_corners)                               # :397-398
    cycle_tsf_imgs = cycle_tsf_mask * bg + (1 - cycle_tsf_mask) * cycle_tsf_color                     # :401
    if front is not None:
        cycle_tsf_imgs = warp(cycle_tsf_imgs, src_inputs[:, 0:3], front[1], fake_src_mask)            # :403-404

    cycle_loss = F.l1_loss(src_imgs, fake_src_imgs) + F.l1_loss(src_imgs, cycle_tsf_imgs)             # :434
    body_mask = 1 - src_inputs[:, -1:]                                                                # :437-438
    str_src_imgs = src_imgs * body_mask                                                               # :439
    cycle_warp_imgs = torch_ref.grid_sample(fake_tsf_imgs, T_cycle, align_corners)                    # :440
    struct_loss = F.l1_loss(init_preds, fake_tsf_imgs) + \
        2 * F.l1_loss(str_src_imgs * back_head, cycle_warp_imgs * back_head)                          # :442-443
    mask_loss = F.binary_cross_entropy(torch.cat([fake_src_mask, fake_tsf_mask], dim=0), pseudo_masks)   # :450
    terms = dict(cycle=cycle_loss, struct=struct_loss, mask=mask_loss)
    total = 10 * cycle_loss + 10 * struct_loss + 5 * mask_loss                                        # :452
    if fsd is not None:
        terms["fid"] = face_term(fsd, src_imgs, cycle_tsf_imgs, j2ds[:, 0]) + \
            face_term(fsd, init_preds, fake_tsf_imgs, j2ds[:, 1])                                     # :445-446
        total = total + terms["fid"]
    terms["total"] = total
    return total, terms, dict(fake_src=fake_src_imgs, fake_tsf=fake_tsf_imgs, cyc_tsf=cycle_tsf_imgs,
                              src_mask=fake_src_mask, tsf_mask=fake_tsf_mask)


def steps(sd, samples, bg, back_heads, fronts=None, n_steps=None, **kw):
    """`len(samples)` iterations with the reference's optimiser (:415-417, :453-455): torch.optim.Adam over every generator
    parameter, lr 2e-4, betas (0.5, 0.999).  -> (per-step terms as floats, the first step's gradients (None where a parameter
    got none), the final parameters)."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    optim = torch.optim.Adam(list(params.values()), lr=0.0002, betas=(0.5, 0.999))                    # :415-417
    hist, first = [], None
    for i, sample in enumerate(samples):
        total, terms, _ = step_loss(params, sample, bg, back_heads[i], None if fronts is None else fronts[i], **kw)
        optim.zero_grad()                                                                             # :453
        total.backward()                                                                              # :454
        if first is None:
            first = {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in params.items()}
        optim.step()                                                                                  # :455
        hist.append({k: float(v.detach()) for k, v in terms.items()})
    return hist, first, {k: v.detach().clone() for k, v in params.items()}


class TableRender(object):
    """Stand-in for SMPLRenderer.encode_front_fim (utils/nmr.py:343-352): two face -> {0,1} tables, the last row the
    background's (fim == -1 wraps to it)."""

    def __init__(self, nf, seed):
        g = torch.Generator().manual_seed(seed)
        self.front = (torch.rand(nf + 1, 1, generator=g) > 0.5).float()
        self.back = (torch.rand(nf + 1, 1, generator=g) > 0.5).float()
        self.front[-1] = self.back[-1] = 0.0

    def encode_front_fim(self, fim, transpose=True, front_fn=True):
        table = (self.front if front_fn else self.back).to(fim.device)
        enc = table[fim.long()]
        return enc.permute(0, 3, 1, 2) if transpose else enc


def sample_batch(seed=5, n=2, size=64, nf=40):
    """Seeded stand-in for one batch of MetaCycleDataSet (run_imitator.py:129-153): flows with an out-of-range patch (-2, what
    cal_bc_transform leaves outside the body), random face maps, binary pseudo masks."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    flow = lambda: torch.rand(n, size, size, 2, generator=g) * 2.4 - 1.2
    T, T_cycle = flow(), flow()
    T[0, size // 4:size // 2, size // 8:size // 3] = -2
    T_cycle[n - 1, size // 3:size // 2, size // 2:] = -2
    cond = lambda: torch.cat([r(n, 2, size, size), (torch.rand(n, 1, size, size, generator=g) > 0.5).float()], dim=1)
    fim = lambda: torch.randint(-1, nf, (n, size, size), generator=g).float()
    return dict(images=r(n, 2, 3, size, size), pseudo_masks=(torch.rand(n, 2, 1, size, size, generator=g) > 0.5).float(),
                j2d=r(n, 2, 19, 2) * 0.8, T=T, T_cycle=T_cycle, src_inputs=torch.cat([r(n, 3, size, size), cond()], dim=1),
                tsf_inputs=torch.cat([r(n, 3, size, size), cond()], dim=1), src_fim=fim(), tsf_fim=fim(), preds=r(n, 3, size, size))
