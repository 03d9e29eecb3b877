"""CPU autograd restatement of the loop of the reference's Swapper.post_personalize (models/swapper.py:273-476) -- what the
device's SwapTuner (impersonator_amd/models/post_tune.py) is held to.  Helper module, no tests of its own
(tests/test_swap_tune_oracle.py checks it, tests/test_gpu_swap_tune.py uses it).

The loss is tests/post_tune_ref.step_loss with back_head = 1 (no back-of-head mask, :436-442) and a background per sample
(:277), apart from `fid`; this module adds only the swap `fid` pairs (:444-445), the loop with the reference's learning-rate
updates (:391-398, :473-474), the bs == 1 row selection (:409-421) and a restatement of set_inputs / initialize (:279-329)."""
import torch

from oracle import torch_ref
from tests import post_tune_ref as ref


def step_loss(sd, sample, bg, front=None, cut_cycle=False, fsd=None, align_corners=False):
    """:429-451 -> (total, terms, images): post_tune_ref.step_loss without a back-of-head mask; `fid` (when `fsd` is given)
    compares (src_imgs, cycle_tsf; j2d[:, 0]) and (tsf_inputs[:, 0:3], fake_tsf; j2d[:, 1]) (:444-445)."""
    total, terms, images = ref.step_loss(sd, sample, bg, 1, front, cut_cycle=cut_cycle, align_corners=align_corners)
    if fsd is not None:
        src_imgs, j2ds = sample["images"][:, 0], sample["j2d"]
        terms["fid"] = ref.face_term(fsd, src_imgs, images["cyc_tsf"], j2ds[:, 0]) + \
            ref.face_term(fsd, sample["tsf_inputs"][:, 0:3], images["fake_tsf"], j2ds[:, 1])                      # :444-445
        total = total + terms["fid"]
        terms["total"] = total
    return total, terms, images


def lr_transcription(total_iters=50, fix_iters=25, init_lr=0.0002, final_lr=0.00001):
    """The rate every step of the loop runs with: :391-395 and :473-474 with update_learning_rate (:382-389), literally."""
    cur_lr = init_lr                                                                                              # :392
    used = []
    for step in range(total_iters):                                                                               # :408
        used.append(cur_lr)                       # what optimizer.step() (:454) sees
        if step > fix_iters:                                                                                      # :473
            lr_decay = (init_lr - final_lr) / fix_iters                                                           # :384
            cur_lr -= lr_decay                                                                                    # :385
    return used


def select(sample, bg, i):
    """:409-421, the bs == 1 rule: sample i of the batch of two as a batch of one (with its background).  pseudo_masks keeps
    the loader's (n, 2, ...) layout: row i holds sample i's source and transfer mask, the reference's flat pseudo_masks[i:4:2]."""
    return {k: v[i:i + 1] for k, v in sample.items()}, bg[i:i + 1]


def steps(sd, sample, bg, total_iters, fix_iters, front=None, bs=2, n_steps=None, **kw):
    """`n_steps` (default: all `total_iters`) iterations of :408-474 on the batch `sample` (n = 2): torch.optim.Adam over every
    parameter, betas (0.5, 0.999), the rate updated after the step as the reference does.  bs == 1: step s trains on sample s % 2.
    -> (per-step terms as floats, the first step's gradients (None where a parameter got none), the final parameters)."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    init_lr, final_lr = 0.0002, 0.00001                                                                           # :391-393
    cur_lr = init_lr
    optim = torch.optim.Adam(list(params.values()), lr=init_lr, betas=(0.5, 0.999))                               # :398
    hist, first = [], None
    for step in range(total_iters if n_steps is None else n_steps):
        if bs == 1:
            i = step % 2                                                                                          # :410
            s, b = select(sample, bg, i)
            f = None if front is None else tuple(m[i:i + 1] for m in front)
        else:
            s, b, f = sample, bg, front
        total, terms, _ = step_loss(params, s, b, f, **kw)
        optim.zero_grad()                                                                                         # :452
        total.backward()                                                                                          # :453
        if first is None:
            first = {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in params.items()}
        optim.step()                                                                                              # :454
        hist.append({k: float(v.detach()) for k, v in terms.items()})
        if step > fix_iters:                                                                                      # :473-474
            cur_lr -= (init_lr - final_lr) / fix_iters
            for group in optim.param_groups:
                group['lr'] = cur_lr
    return hist, first, {k: v.detach().clone() for k, v in params.items()}


def set_inputs(sd, src_info, tsf_info, front_fn=None, ft_ks=3):
    """:279-329 on CPU tensors, in the loader's layout (what PostTuner.load reads).  `src_info` / `tsf_info`: dicts with
    'p2verts' (1,nf,3,2), 'fim', 'wim', 'cond', 'img', 'bg', 'src_inputs', 'j2d' and 'feats' = (encoder outs, resnet outs).
    `front_fn`: fim -> front mask (1,1,H,W) for --front_warp (Swapper.warp, :255-259), None without."""
    def initialize(src, tsf):                                                                                     # :280-300
        T = torch_ref.cal_bc_transform(src['p2verts'], tsf['fim'], tsf['wim'])                                    # :288
        tsf_img = torch_ref.grid_sample(src['img'], T)                                                            # :289
        tsf_inputs = torch.cat([tsf_img, tsf['cond']], dim=1)                                                     # :290
        enc, res = src['feats']
        preds, _, mask = torch_ref.imitator_forward(sd, enc, res, src['bg'], tsf_inputs, T)                       # :292-295
        if front_fn is not None:                                                                                  # :297-298, :255-259
            front_mask = front_fn(tsf['fim'])
            preds = (1 - front_mask) * preds + tsf_img * front_mask * (1 - mask)
        return preds, T, tsf_inputs

    pa, Ta, ia = initialize(src_info, tsf_info)                                                                   # :304
    pb, Tb, ib = initialize(tsf_info, src_info)                                                                   # :305
    pair = lambda k: torch.cat([src_info[k], tsf_info[k]], dim=0)
    riap = lambda k: torch.cat([tsf_info[k], src_info[k]], dim=0)
    src_inputs, tsf_inputs = pair('src_inputs'), torch.cat([ia, ib], dim=0)                                       # :315, :322
    src_mask = torch_ref.morph(src_inputs[:, -1:], ft_ks, "erode")                                                # :324
    tsf_mask = torch_ref.morph(tsf_inputs[:, -1:], ft_ks, "erode")                                                # :325
    return dict(images=torch.stack([pair('img'), riap('img')], dim=1),                                            # :312
                pseudo_masks=torch.stack([src_mask, tsf_mask], dim=1),                                            # :327
                j2d=torch.stack([pair('j2d'), riap('j2d')], dim=1),                                               # :307-309
                T=torch.cat([Ta, Tb], dim=0), T_cycle=torch.cat([Tb, Ta], dim=0),                                 # :313-314
                src_inputs=src_inputs, tsf_inputs=tsf_inputs, src_fim=pair('fim').float(), tsf_fim=riap('fim').float(),   # :316-317
                preds=torch.cat([pa, pb], dim=0), bg=pair('bg'))                                                  # :311, :277
