#!/usr/bin/env python
"""Writes tests/golden/global_local_golden.npz from the LIVE reference (networks/discriminator.py through oracle.reference_loader):

    python tests/golden/make_global_local_golden.py

The reference's own `GlobalLocalDiscriminator` (discriminator.py:60-96) as the augmented trainer builds it
(impersonator_trainer_aug.py:220-222), its LSGAN loss (`_optimize_D` / `_compute_loss_D`, :405-425), the generator's adversarial
term (:378-381), torch autograd and one torch.optim.Adam step, on seeded weights, inputs and three body boxes.  Run in fp64 (the
yardstick) and in fp32 (the reference's own arithmetic, whose distance from fp64 is recorded per group and must stay below a
quarter of the bound the tests apply).  Data only: names, shapes, maps, losses, norms and strided samples.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import reference_loader  # noqa: E402
from tests import helpers  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "global_local_golden.npz")
INPUT_NC, NDF, N_LAYERS, S, N = 6, 64, 4, 64, 3
SEED_GLOBAL, SEED_LOCAL, SEED_INPUT = 7, 8, 1
# a box touching the right and bottom edges, a 2x2 corner, a one-pixel-wide column: (min_x, max_x, min_y, max_y), exclusive ends
RECTS = [[10, 50, 4, 64], [0, 2, 0, 2], [31, 32, 5, 60]]
LR, BETAS = 2e-4, (0.5, 0.999)
INPUT_STRIDE = 13
# the bounds tests/test_gpu_global_local.py applies (fp32), per group
BOUNDS = {"forward": 1e-4, "loss": 1e-5, "param_grad": 2e-3, "input_grad": 1e-3}


def state_dict():
    sd = {"global_model." + k: v for k, v in helpers.discriminator_state_dict(seed=SEED_GLOBAL, input_nc=4).items()}
    sd.update({"local_model." + k: v for k, v in helpers.discriminator_state_dict(seed=SEED_LOCAL, input_nc=INPUT_NC).items()})
    return sd


def inputs():
    """-> real_global (4 ch), real_local (6 ch), fake_global, fake_local, drawn in this order; and the rects tensor."""
    gen = torch.Generator().manual_seed(SEED_INPUT)
    xs = [torch.rand(N, c, S, S, generator=gen) * 2 - 1 for c in (4, INPUT_NC, 4, INPUT_NC)]
    return xs, torch.tensor(RECTS, dtype=torch.int64)


def normed_bias_keys():
    """Biases of the convs in front of an InstanceNorm: their gradient is analytically zero."""
    idx = [2 + 3 * k for k in range(N_LAYERS)]
    return {"%s.model.%d.bias" % (b, i) for b in ("global_model", "local_model") for i in idx}


def reference_model(dtype):
    ref = reference_loader.load()
    D = ref.discriminator.GlobalLocalDiscriminator(input_nc=INPUT_NC, ndf=NDF, n_layers=N_LAYERS, norm_type='instance',
                                                   use_sigmoid=False)
    D.load_state_dict(state_dict())
    return D.to(dtype)


def reference_forward_and_loss(dtype=torch.float64):
    """-> (D(real), D(fake), loss_D) by the reference's own forward."""
    D = reference_model(dtype)
    (rg, rl, fg, fl), rects = inputs()
    with torch.no_grad():
        d_real = D(rg.to(dtype), rl.to(dtype), rects)
        d_fake = D(fg.to(dtype), fl.to(dtype), rects)
        loss = torch.mean((d_real - 1) ** 2) + torch.mean((d_fake + 1) ** 2)
    return d_real, d_fake, loss


def run(dtype):
    D = reference_model(dtype)
    (rg, rl, fg, fl), rects = [[x.to(dtype) for x in inputs()[0]], inputs()[1]]
    out = {}
    with torch.no_grad():
        out["d_real"], out["d_fake"] = D(rg, rl, rects), D(fg, fl, rects)
    # the generator's adversarial term on the fake pair (impersonator_trainer_aug.py:378-381), target 0
    xg, xl = fg.clone().requires_grad_(True), fl.clone().requires_grad_(True)
    g_loss = torch.mean((D(xg, xl, rects) - 0) ** 2)
    g_loss.backward()
    out["g_loss"], out["d_global"], out["d_local"] = g_loss.detach(), xg.grad.detach(), xl.grad.detach()
    # the discriminator update (:405-422, :371-373)
    opt = torch.optim.Adam(D.parameters(), lr=LR, betas=BETAS)
    opt.zero_grad()
    loss = torch.mean((D(rg, rl, rects) - 1) ** 2) + torch.mean((D(fg, fl, rects) + 1) ** 2)
    loss.backward()
    out["loss"] = loss.detach()
    out["grads"] = {k: p.grad.detach().clone() for k, p in D.named_parameters()}
    opt.step()
    out["params"] = {k: p.detach().clone() for k, p in D.named_parameters()}
    return out


def param_stride(numel):
    """Stride of a parameter's sample: dense for the small tensors, about a thousand entries of the large ones."""
    return 389 if numel > 4096 else 7


def _rel(a, b):
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def compute():
    r64, r32 = run(torch.float64), run(torch.float32)
    zero = normed_bias_keys()
    err = {
        "forward": max(_rel(r32["d_real"], r64["d_real"]), _rel(r32["d_fake"], r64["d_fake"])),
        "loss": max(abs(float(r32[k]) - float(r64[k])) / abs(float(r64[k])) for k in ("loss", "g_loss")),
        "param_grad": max(_rel(r32["grads"][k], g) for k, g in r64["grads"].items() if k not in zero),
        "input_grad": max(_rel(r32["d_global"], r64["d_global"]), _rel(r32["d_local"], r64["d_local"])),
    }
    for k in zero:
        assert float(r64["grads"][k].abs().max()) < 1e-10, (k, float(r64["grads"][k].abs().max()))
    keys = list(r64["grads"])
    out = dict(keys=np.array(keys), shapes=np.array([",".join(str(d) for d in r64["grads"][k].shape) for k in keys]),
               strides=np.array([param_stride(r64["grads"][k].numel()) for k in keys], np.int64), rects=np.array(RECTS, np.int64), d_real=r64["d_real"].numpy(), d_fake=r64["d_fake"].numpy(),
               loss=np.array([float(r64["loss"])]), g_loss=np.array([float(r64["g_loss"])]),
               ref_fp32_err_names=np.array(list(err)), ref_fp32_err=np.array([err[k] for k in err], np.float64))
    for name in ("d_global", "d_local"):
        g = r64[name]
        out["inorm/" + name] = np.array([g.abs().sum().item(), (g * g).sum().sqrt().item(), g.abs().max().item()])
        out["isample/" + name] = g.flatten()[::INPUT_STRIDE].numpy().copy()
    for k in keys:
        g = r64["grads"][k]
        out["gnorm/" + k] = np.array([g.abs().sum().item(), (g * g).sum().sqrt().item(), g.abs().max().item()])
        out["gsample/" + k] = g.flatten()[::param_stride(g.numel())].numpy().copy()
        out["psample/" + k] = r64["params"][k].flatten()[::param_stride(g.numel())].numpy().copy()
    return out, err


if __name__ == "__main__":
    data, err = compute()
    for k, e in err.items():
        print("reference fp32 vs fp64, %-10s %.3g  (test bound %.1g)" % (k, e, BOUNDS[k]))
    bad = [k for k, e in err.items() if e > BOUNDS[k] / 4]
    if bad:
        sys.exit("not written: the reference's own fp32 is further from fp64 than a quarter of the test bound for %s; "
                 "pick another seed" % bad)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes), loss %.9f, g_loss %.9f" % (OUT, os.path.getsize(OUT), data["loss"][0], data["g_loss"][0]))
