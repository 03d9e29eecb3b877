"""Timing of LPIPS (networks/lpips.py, csrc/lpips.hip) on one GPU: 256 x 256, 1 and 8 pairs, synthetic weights.

    python tools/bench_lpips.py [--iters 50] [--frames 256] [--rounds 5] [--out profiles/lpips.md]

Measurements, in one process, warmed up:
  (a) one forward (pred and ref as one batch of 2n images) of the device path against the SAME network as torch-ROCm eager
      ops on the same GPU, timed with device events over `--iters` forwards, the two alternating, three rounds;
  (b) in a run of its own under the torch profiler, the device path's kernel times by stage (the launch order is fixed) with
      the FLOPs of each convolution from the shapes (3.47 GFLOP per pair) and the achieved share of the 157.3 TFLOP/s fp32 MFMA
      peak of the MI355X;
  (c) frames/s of the imitation loop (Imitator.predict_batches over `--frames` frames) with `PairedEvaluator.update` carrying
      (ssim, psnr) and carrying (ssim, psnr, lpips), and without it; host clock around the loop ending in a synchronise, the
      forms alternating, median of `--rounds` (min .. max); and the LPIPS of the bf16x3 frames against the exact-fp32 frames.
No time here is a pass/fail gate.  No GPU: it fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.networks import lpips as lpips_net  # noqa: E402
from impersonator_amd.utils import metrics, synthetic  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
SIZE, BATCH = 256, 8
STRIDE_PAD = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))


def stage_plan(size=SIZE):
    """[(stage, FLOPs per IMAGE or 0)] in launch order: conv, distance, [pool] per layer, then the sum of the taps"""
    plan, h = [], size
    for j, ((_, cout, cin, k), (s, p)) in enumerate(zip(lpips_net.CONVS, STRIDE_PAD)):
        h = (h + 2 * p - k) // s + 1
        plan += [("conv%d" % (j + 1), 2.0 * h * h * cout * cin * k * k), ("distance%d" % (j + 1), 0.0)]
        if j < 2:
            plan.append(("maxpool%d" % (j + 1), 0.0))
            h = (h - 3) // 2 + 1
    plan.append(("sum of taps", 0.0))
    return plan


class Eager(object):
    """the same network as torch ops in fp32 on the GPU (what a second framework would run)"""

    def __init__(self, alex, lin):
        t = lambda v: torch.from_numpy(np.asarray(v)).cuda()
        self.w = [(t(alex["features.%d.weight" % i]), t(alex["features.%d.bias" % i])) for i, _, _, _ in lpips_net.CONVS]
        self.lin = [t(lin["lin%d.model.1.weight" % j]) for j in range(5)]
        self.shift = torch.tensor([-.030, -.088, -.188], device="cuda").view(1, 3, 1, 1)
        self.scale = torch.tensor([.458, .448, .450], device="cuda").view(1, 3, 1, 1)

    @torch.no_grad()
    def __call__(self, pred, ref):
        n = pred.shape[0]
        x = (torch.cat([pred, ref]) - self.shift) / self.scale
        val = 0
        for j, ((w, b), (s, p)) in enumerate(zip(self.w, STRIDE_PAD)):
            if j in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w, b, stride=s, padding=p))
            f = x / (torch.sqrt((x ** 2).sum(dim=1, keepdim=True)) + 1e-10)
            val = val + F.conv2d((f[:n] - f[n:]) ** 2, self.lin[j]).mean(dim=(2, 3))
        return val.view(n)


def time_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    alex, lin = synthetic.lpips_state_dicts(0)
    model = lpips_net.LPIPS(alex, lin, max_batch=BATCH, image_size=SIZE)
    eager = Eager(alex, lin)
    plan = stage_plan()
    flops_pair = 2 * sum(f for _, f in plan)
    lines = ["# LPIPS (AlexNet, v0.1) on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_lpips.py --iters %d --frames %d --rounds %d`: %d x %d, synthetic weights, one process; "
             "%.2f GFLOP per pair in the convolutions." % (args.iters, args.frames, args.rounds, SIZE, SIZE, flops_pair / 1e9), "",
             "## One forward: the device path against eager torch", "",
             "Warm forwards timed with device events, the two alternating.", "",
             "| pairs | liblwg ms (3 rounds) | eager torch ms (3 rounds) | liblwg / eager | liblwg us per pair | share of fp32 MFMA peak |",
             "|---|---|---|---|---|---|"]
    rs = np.random.RandomState(1)
    for n in (1, BATCH):
        a = torch.from_numpy(synthetic.smooth_image(3, (n, 3, SIZE, SIZE))).cuda()
        b = torch.from_numpy(np.clip(a.cpu().numpy() + 0.1 * rs.uniform(-1, 1, a.shape), -1, 1).astype(np.float32)).cuda()
        out = torch.empty((n,), dtype=torch.float64, device="cuda")
        dev = lambda: model(a, b, out=out)
        eag = lambda: eager(a, b)
        for fn in (dev, eag):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        d, e = [], []
        for _ in range(3):
            d.append(time_ms(dev, args.iters))
            e.append(time_ms(eag, args.iters))
        rel = float(((model(a, b) - eager(a, b).double()).abs() / model(a, b)).max())
        lines.append("| %d | %s | %s | %.2f | %.1f | %.3f |" % (n, " ".join("%.3f" % v for v in d), " ".join("%.3f" % v for v in e),
                                                            min(d) / min(e), min(d) * 1e3 / n, flops_pair * n / (min(d) * 1e-3) / PEAK_FP32_MFMA))
        print(lines[-1], "  max relative |device - eager| = %.3g" % rel, flush=True)

        # kernel times by stage: a run of its own under the profiler
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        reps = 5
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                dev()
            torch.cuda.synchronize()
        ev = sorted((k for k in prof.events() if k.device_type == DeviceType.CUDA), key=lambda k: k.time_range.start)
        assert len(ev) == reps * len(plan), "expected %d kernels per forward, the profiler saw %d in %d forwards" % (len(plan), len(ev), reps)
        s_lines = ["", "%d pair%s, kernel time by stage (mean of %d profiled forwards):" % (n, "" if n == 1 else "s", reps), "",
                   "| stage | GFLOP | us | TFLOP/s | share of 157.3 TFLOP/s |", "|---|---|---|---|---|"]
        total = 0.0
        for k, (name, flops) in enumerate(plan):
            us = sum(ev[r * len(plan) + k].time_range.elapsed_us() for r in range(reps)) / reps
            total += us
            rate = 2 * n * flops / (us * 1e-6)
            s_lines.append("| %s | %s | %.1f | %s | %s |" % (name, "%.3f" % (2 * n * flops / 1e9) if flops else "-", us,
                                                         "%.1f" % (rate / 1e12) if flops else "-", "%.3f" % (rate / PEAK_FP32_MFMA) if flops else "-"))
        s_lines.append("| all kernels | %.3f | %.1f | %.1f | %.3f |" % (flops_pair * n / 1e9, total, flops_pair * n / (total * 1e-6) / 1e12,
                                                                     flops_pair * n / (total * 1e-6) / PEAK_FP32_MFMA))
        stage_lines = s_lines if n == 1 else stage_lines + s_lines
        print("\n".join(s_lines), flush=True)
    lines += stage_lines

    # the imitation loop
    imitator, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(batch_size=BATCH, image_size=SIZE)
    smpls = torch.as_tensor(demo.synthetic_smpls(args.frames, seed=0)).float().cuda()
    batches = lambda: ((smpls[s:s + BATCH], s) for s in range(0, args.frames, BATCH))

    def sequence(precision):
        imitator.generator.precision = precision
        imitator.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
        imitator.first_cam = smpls[0:1, 0:3].clone()
        return {t: p for t, p in imitator.predict_batches(batches(), 'smooth')}

    truth = sequence("fp32")
    seq = sequence("bf16x3")
    ev = metrics.PairedEvaluator(("ssim", "psnr", "lpips"), lpips=model)
    for t in sorted(seq):
        ev.update(seq[t], truth[t])
    r = ev.result()
    del seq

    def region(names):
        ev = metrics.PairedEvaluator(names, lpips=model) if names else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t, preds in imitator.predict_batches(batches(), 'smooth'):
            if ev is not None:
                ev.update(preds, truth[t])
        if ev is not None:
            assert ev.result()["frames"] == args.frames
        torch.cuda.synchronize()
        return args.frames / (time.perf_counter() - t0)

    forms = ((), ("ssim", "psnr"), ("ssim", "psnr", "lpips"))
    for names in forms:
        region(names)
    fps = {names: [] for names in forms}
    for _ in range(args.rounds):
        for names in forms:
            fps[names].append(region(names))
    cell = lambda v: "%.0f (%.0f .. %.0f)" % (statistics.median(v), min(v), max(v))
    med = {names: statistics.median(v) for names, v in fps.items()}
    lines += ["", "## The imitation loop (bf16x3) with and without `PairedEvaluator.update`", "",
              "frames/s over %d frames in batches of %d, host clock around `predict_batches` ending in a synchronise (with the "
              "evaluator: in `result()`), forms alternating, median of %d (min .. max)." % (args.frames, BATCH, args.rounds), "",
              "| imitation only | + `update` (ssim, psnr) | + `update` (ssim, psnr, lpips) | lpips form / imitation only |", "|---|---|---|---|",
              "| %s | %s | %s | %.3f |" % (cell(fps[forms[0]]), cell(fps[forms[1]]), cell(fps[forms[2]]), med[forms[2]] / med[forms[0]]), "",
              "What carrying `lpips` adds per frame, from the medians: %.1f us over the (ssim, psnr) form, %.1f us over the bare loop."
              % (1e6 / med[forms[2]] - 1e6 / med[forms[1]], 1e6 / med[forms[2]] - 1e6 / med[forms[0]]), "",
              "## Value: the bf16x3 sequence against the exact-fp32 generator (synthetic AlexNet and lin weights)", "",
              "| frames | LPIPS mean | LPIPS max | 1 - SSIM | PSNR (dB) |", "|---|---|---|---|---|",
              "| %d | %.3g | %.3g | %.3g | %.2f |" % (r["frames"], r["lpips"], r["per_frame"]["lpips"].max(), 1 - r["ssim"], r["psnr"])]
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
