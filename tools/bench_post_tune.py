"""Timing of personalisation by fine-tuning (impersonator_amd/models/post_tune.py, csrc/train.hip) on one GPU:

    python tools/bench_post_tune.py [--iters 20] [--out profiles/post_tune.md]

1. One iteration (two generator passes, loss, backward through both, Adam) at 256x256, batch 4, on samples built from the
   synthetic Imitator (meta_samples), conv_precision fp32 and bf16x3 alternating, three rounds, device events.
2. The stems' data gradient (lwg_conv2d_backward_data: dy (4,256,256,64), w (64,8,7,7) -> dx (4,256,256,8)) on its own kernel,
   next to the route today's other ops allow: ops.conv2d_forward of dy with the flipped, transposed filter padded to 64 output
   rows (what networks/vgg.py does for its first layer), 8 x the products.  Alternating, three rounds; the two results are
   compared first.
3. The gradient's distance from float64 autograd on the GPU test's batch, both precisions (tests/test_gpu_post_tune.py bounds the
   bf16x3 one at 1.5 x this figure).
No GPU: it fails."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd import demo, ops  # noqa: E402
from impersonator_amd.models.post_tune import PostTuner, meta_samples  # noqa: E402

SIZE, BATCH = 256, 4


def time_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def rounds(fns, iters, n=3):
    """{name: [ms per round]}: the candidates alternate inside every round"""
    out = {k: [] for k in fns}
    for fn in fns.values():
        fn()                  # every shape warm
    for _ in range(n):
        for k, fn in fns.items():
            out[k].append(time_ms(fn, iters))
    return out


def fmt(ms):
    return " / ".join("%.3f" % v for v in ms)


def gradient_distances():
    """whole-gradient relative L2 of the device gradient from float64 CPU autograd on the batch of tests/test_gpu_post_tune.py"""
    from oracle import torch_ref
    from tests import helpers
    from tests import post_tune_ref as ref
    from impersonator_amd.networks.generator import ImpersonatorGenerator
    gsd = torch_ref.state_dict_from_numpy(helpers.generator_state_dict(seed=2, affine="random"))
    G = ImpersonatorGenerator(bg_dim=4, src_dim=6, tsf_dim=6, repeat_num=6, image_size=128, max_batch=2)
    G.load_state_dict(gsd)
    sample = ref.sample_batch(seed=5, n=2, size=64, nf=40)
    bg = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1
    render = ref.TableRender(40, seed=3)
    bh = 1 - render.encode_front_fim(sample["tsf_fim"], front_fn=False)
    g64 = ref.steps({k: v.double() for k, v in gsd.items()}, [{k: v.double() for k, v in sample.items()}], bg.double(), [bh.double()])[1]
    g32 = ref.steps(gsd, [sample], bg, [bh])[1]

    def dist(g):
        num = sum(float(((g[k].double() - v) ** 2).sum()) for k, v in g64.items() if v is not None)
        return (num / sum(float((v ** 2).sum()) for v in g64.values() if v is not None)) ** 0.5

    out = {"CPU float32 autograd": dist(g32)}
    for precision in ("fp32", "bf16x3"):
        t = PostTuner(G, bg, render, conv_precision=precision)
        t.forward(sample)
        t.backward()
        out["device, conv_precision=%s" % precision] = dist(t.gradients())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_post_tune: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    lines = ["# Personalisation by fine-tuning on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_post_tune.py --iters %d`: device events around warm calls, the candidates of a table alternating "
             "in one process, three rounds each." % args.iters, ""]

    # ---- 1. the iteration
    opt = demo.default_opt(batch_size=BATCH, image_size=SIZE, post_tune=True)
    im, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(batch_size=BATCH, image_size=SIZE, opt=opt)
    im.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
    sample = meta_samples(im, tgt_smpls=demo.synthetic_smpls(BATCH, seed=7))[0]
    tuners = {p: PostTuner(im.generator, im.src_info["bg"], im.render, conv_precision=p) for p in ("fp32", "bf16x3")}
    res = rounds({p: (lambda t=t: t.optimize(sample)) for p, t in tuners.items()}, max(3, args.iters // 4))
    lines += ["## One iteration at %dx%d, batch %d" % (SIZE, SIZE, BATCH), "",
              "Two generator passes, the four loss terms, the backward pass through both, Adam (`PostTuner.optimize`; the float "
              "read-back of the terms included).", "", "| conv_precision | ms per iteration (3 rounds) |", "|---|---|"]
    lines += ["| %s | %s |" % (p, fmt(ms)) for p, ms in res.items()]
    del tuners

    # ---- 2. the stems' data gradient
    g = torch.Generator().manual_seed(1)
    w = torch.randn(64, 8, 7, 7, generator=g) * 0.05
    w[:, 6:] = 0
    dy = torch.randn(BATCH, SIZE, SIZE, 64, generator=g).cuda()
    # dx = conv(dy, w') with w'[ci][co][ky][kx] = w[co][ci][6-ky][6-kx], its 8 output rows padded to the 64 the GEMM kernels produce
    w_pad = torch.zeros(64, 64, 7, 7)
    w_pad[:8] = w.flip(2, 3).permute(1, 0, 2, 3)
    w, w_pad = w.cuda(), w_pad.contiguous().cuda()
    new = lambda: ops.conv2d_backward_data(dy, w, (BATCH, SIZE, SIZE, 8), 1, 3)
    padded = lambda: ops.conv2d_forward(dy, w_pad, None, 1, 3)
    a, b = new(), padded()[..., :8]
    err = float((a - b).abs().max()) / float(b.abs().max())
    res = rounds({"stem_dgrad_kernel (new)": new, "padded to 64 rows, fp32 implicit GEMM": padded}, args.iters)
    macs = BATCH * SIZE * SIZE * 49 * 64 * 8
    t_new, t_pad = min(res["stem_dgrad_kernel (new)"]), min(res["padded to 64 rows, fp32 implicit GEMM"])
    lines += ["", "## The stems' data gradient: dy (%d,%d,%d,64), w (64,8,7,7) -> dx (%d,%d,%d,8)" % ((BATCH, SIZE, SIZE) * 2), "",
              "%.2f GMAC needed; the padded route computes 8 x that.  The two results agree to %.2g of the largest entry.  Each call "
              "includes its filter re-layout and workspace allocation, as the tuner pays them." % (macs / 1e9, err), "",
              "| route | ms per call (3 rounds) | TFLOP/s on the needed products (best round) |", "|---|---|---|"]
    lines += ["| %s | %s | %.1f |" % (k, fmt(ms), 2 * macs / (min(ms) * 1e-3) / 1e12) for k, ms in res.items()]
    lines += ["", "New kernel / padded route: %.2f of its time (expected from the product count: well under a quarter).%s" % (
        t_new / t_pad, "" if t_new < t_pad else "  **The new kernel is NOT faster than the padded route.**")]

    # ---- 3. gradient distances
    lines += ["", "## Whole-gradient relative L2 distance from float64 autograd (64x64, batch 2, the GPU test's batch)", "",
              "| gradient | distance |", "|---|---|"]
    lines += ["| %s | %.3g |" % kv for kv in gradient_distances().items()]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
