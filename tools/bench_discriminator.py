"""Secondary measurement (NOT the bench.py contract): one PatchGAN discriminator update on an MI355X.

    python tools/bench_discriminator.py [--batch 8] [--image-size 256] [--steps 20]

Prints one JSON line: ms per update (forward of 2N images + backward + Adam), algorithmic conv TFLOP/s
(forward + data gradient + weight gradient of the six 4x4 convs), under torch.distributed.run also with the gradient
all-reduce (RCCL) between backward and Adam.

    python tools/bench_discriminator.py --global-local [--rounds 5]

times one GlobalLocalDiscriminator update (N + N images per branch, body crop on the device) against the two plain PatchGAN
updates (4 and 6 channels) it is made of, at the same shapes in the same process, alternating; prints one JSON line and writes
the table to profiles/global_local.md."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from impersonator_amd import sharding  # noqa: E402
from impersonator_amd import ops  # noqa: E402
from impersonator_amd.networks.discriminator import GlobalLocalDiscriminator, PatchDiscriminator  # noqa: E402


def conv_flops(image_size, n_layers=4, input_nc=6, ndf=64):
    """fwd + dgrad (all but the first layer) + wgrad FLOPs per image."""
    H, cin, total = image_size, input_nc, 0.0
    chans = [ndf] + [ndf * min(2 ** n, 8) for n in range(1, n_layers)] + [ndf * min(2 ** n_layers, 8), 1]
    for l, cout in enumerate(chans):
        Ho = H // 2 if l < n_layers else H - 1
        f = 2.0 * Ho * Ho * cout * 16 * cin
        total += f * (2 if l == 0 else 3)
        H, cin = Ho, cout
    return total


def _timed(fn, steps):
    """ms per call: a host clock around `steps` calls that end in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def global_local(args):
    """One global-local update vs the two plain PatchGAN updates of the same shapes, and the crop passes on their own."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n, size = args.batch, args.image_size
    kw = dict(ndf=64, n_layers=4, norm_type='instance', use_sigmoid=False, image_size=size, max_batch=n)
    GL = GlobalLocalDiscriminator(6, **kw)
    P4, P6 = PatchDiscriminator(4, **kw), PatchDiscriminator(6, **kw)
    for m in (GL, P4, P6):
        m.init_weights()
        m.to(dev)
    gen = torch.Generator().manual_seed(0)
    rg, rl, fg, fl = [(torch.rand(n, c, size, size, generator=gen) * 2 - 1).to(dev) for c in (4, 6, 4, 6)]
    # body boxes of the size cal_body_bbox returns for a standing person, a different one per sample
    q = size // 16
    boxes = torch.tensor([[(3 + i % 3) * q, (12 + i % 4) * q, (i % 2) * q, size - (i % 3) * q] for i in range(n)],
                         dtype=torch.int64).to(dev)

    def update_gl():
        GL.optimize_D(rg, rl, fg, fl, boxes)

    def update_plain():
        P4.optimize_D(rg, fg)
        P6.optimize_D(rl, fl)

    def crops():
        ops.crop_resize(rl, boxes)
        ops.crop_resize(fl, boxes)

    def crop_back():
        ops.crop_resize_backward(rl, boxes)

    fns = dict(global_local=update_gl, two_patchgans=update_plain, crop_forward_x2=crops, crop_backward=crop_back)
    for fn in fns.values():
        for _ in range(5):
            fn()
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):            # alternate the two, so that drift of the box hits both alike
        for k, fn in fns.items():
            runs[k].append(_timed(fn, args.steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    crop_mb = n * 6 * size * size * 4 * 2 / 1e6
    res = {"metric": "global-local discriminator update", "batch": n, "image_size": size, "steps": args.steps, "rounds": args.rounds,
           "ms_global_local": round(med["global_local"], 3), "ms_two_patchgans": round(med["two_patchgans"], 3),
           "ratio": round(med["global_local"] / med["two_patchgans"], 4),
           "ms_crop_forward_x2": round(med["crop_forward_x2"], 4), "ms_crop_backward": round(med["crop_backward"], 4),
           "crop_pass_mb": round(crop_mb, 1),
           "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in runs.items()}, "dtype": "f32"}
    print(json.dumps(res))
    if args.profile_out:
        rows = [("GlobalLocalDiscriminator.optimize_D (%d+%d images, crop on the device)" % (n, n), "global_local"),
                ("two PatchDiscriminator.optimize_D calls (4 and 6 channels, no crop)", "two_patchgans"),
                ("ops.crop_resize x 2 (real and fake, %.1f MB read + written each)" % crop_mb, "crop_forward_x2"),
                ("ops.crop_resize_backward x 1 (the generator's adversarial term)", "crop_backward")]
        with open(args.profile_out, "w") as fh:
            fh.write("# Global-local discriminator update vs two plain PatchGAN updates\n\n"
                     "`python tools/bench_discriminator.py --global-local --batch %d --image-size %d --steps %d --rounds %d`, fp32, one "
                     "MI355X, host clock around %d calls ending in a device synchronise, %d alternating rounds, median.\n\n"
                     "| what | ms (median) | min .. max |\n|---|---|---|\n" % (n, size, args.steps, args.rounds, args.steps, args.rounds))
            for label, k in rows:
                fh.write("| %s | %.3f | %.3f .. %.3f |\n" % (label, med[k], min(runs[k]), max(runs[k])))
            fh.write("\nglobal-local / two PatchGANs = %.3f.  The second row is what the tree could already do before the "
                     "global-local discriminator existed; the difference is the two crop passes, the loss scale costs nothing.\n"
                     % (med["global_local"] / med["two_patchgans"]))
    for m in (GL, P4, P6):
        m.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--global-local", action="store_true", help="time the global-local update against two plain PatchGAN updates")
    ap.add_argument("--rounds", type=int, default=5, help="--global-local: alternating rounds (median reported)")
    ap.add_argument("--profile-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "global_local.md"), help="--global-local: where the table goes ('' = nowhere)")
    args = ap.parse_args()
    if args.global_local:
        return global_local(args)
    rank, local_rank, world = sharding.init_process_group()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    D = PatchDiscriminator(6, 64, 4, 'instance', False, image_size=args.image_size, max_batch=args.batch)
    D.init_weights()
    D = D.to(dev)
    gen = torch.Generator().manual_seed(rank)
    real = (torch.rand(args.batch, 6, args.image_size, args.image_size, generator=gen) * 2 - 1).to(dev)
    fake = (torch.rand(args.batch, 6, args.image_size, args.image_size, generator=gen) * 2 - 1).to(dev)
    for _ in range(5):
        D.optimize_D(real, fake)
    sharding.barrier(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = D.optimize_D(real, fake)
    sharding.barrier(dev)
    dt = sharding.max_over_ranks(time.perf_counter() - t0, dev if world > 1 else "cpu")
    if rank == 0:
        fl = conv_flops(args.image_size) * 2 * args.batch
        print(json.dumps({"metric": "PatchGAN discriminator update", "ms_per_update": round(dt / args.steps * 1e3, 3),
                          "images_per_s": round(world * args.batch * args.steps / dt, 1), "n_gpus": world,
                          "batch_per_gpu": args.batch, "image_size": args.image_size,
                          "conv_gflop_per_update": round(fl / 1e9, 1),
                          "conv_tflops": round(fl * args.steps / dt / 1e12, 2), "dtype": "f32",
                          "grad_allreduce_mb": round(sum(p.numel() for p in D.parameters()) * 4 / 1e6, 1) if world > 1 else 0,
                          "last_loss": float(loss)}))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
