"""Timing of the InceptionV3 feature network behind FID and Inception Score (networks/inception.py, csrc/inception.hip) on one GPU:
256 x 256 frames resized to 299 x 299, 1, 8 and 32 frames, synthetic weights.

    python tools/bench_fid.py [--iters 20] [--frames 128] [--rounds 5] [--out profiles/fid.md]

Measurements, in one process, warmed up:
  (a) one forward of the device path against the SAME network as torch-ROCm eager ops on the same GPU (the restated module of
      tests/inception_ref.py in fp32, preprocessing included), timed with device events over `--iters` forwards, the two
      alternating, three rounds;
  (b) at 8 frames, stage by stage: the device path's kernel times under the torch profiler in a run of its own (the launch order
      is fixed) and the eager module's stages between device events, with the FLOPs of each stage's convolutions and the achieved
      share of the 157.3 TFLOP/s fp32 MFMA peak of the MI355X;
  (c) frames/s of the imitation loop (Imitator.predict_batches over `--frames` frames) alone, with `SetEvaluator.update(preds)`
      and with `SetEvaluator.update(preds, refs)` in it; host clock around the loop ending in a synchronise, the forms
      alternating, median of `--rounds` (min .. max); and FID / IS of the bf16x3 frames against the exact-fp32 frames.
No time here is a pass/fail gate.  No GPU: it fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.networks import inception as inception_net  # noqa: E402
from impersonator_amd.utils import metrics, synthetic  # noqa: E402
from tests import inception_ref  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
SIZE, BATCH, NET = 256, 8, 299
# kernels per stage in launch order (after the resize kernel, before the global pool): the stem's seven, then the Mixed blocks
KERNELS = [1] * 7 + [8, 8, 8, 5, 11, 11, 11, 11, 7, 10, 10]


def stage_flops():
    """FLOPs per IMAGE of each of the 18 stages at a 299 x 299 input, from the convolution table and the stage shapes"""
    shapes = inception_net.stage_shapes(NET, NET)
    flops = [0.0] * len(inception_net.STAGES)
    for name, cin, cout, (kh, kw), stride, (ph, pw) in inception_net.CONVS:
        stage = inception_net.STAGES.index(name.split(".")[0])
        h, w = shapes[stage - 1][:2] if stage else (NET, NET)     # every convolution of a block runs at the block's input size
        ho, wo = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
        flops[stage] += 2.0 * ho * wo * cout * cin * kh * kw
    return flops


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fid: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    sd = synthetic.inception_state_dict(0)
    model = inception_net.InceptionV3(sd, max_batch=BATCH, image_size=SIZE)
    net = inception_ref.build(sd, torch.float32, "cuda")
    flops = stage_flops()
    total_flops = sum(flops)

    @torch.no_grad()
    def eager(x):
        return net(inception_ref.preprocess(x, NET))

    lines = ["# InceptionV3 features for FID / Inception Score on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_fid.py --iters %d --frames %d --rounds %d`: %d x %d frames in [0,1] resized to %d x %d, synthetic "
             "weights, one process; %.2f GFLOP per frame in the 94 convolutions." % (args.iters, args.frames, args.rounds, SIZE, SIZE, NET, NET,
                                                                                  total_flops / 1e9), "",
             "## One forward: the device path against eager torch", "",
             "Warm forwards timed with device events, the two alternating.  The device path runs at most %d frames per launch "
             "sequence (32 frames: four sequences)." % BATCH, "",
             "| frames | liblwg ms (3 rounds) | eager torch ms (3 rounds) | liblwg / eager | liblwg ms per frame | share of fp32 MFMA peak | rel L2 device vs eager |",
             "|---|---|---|---|---|---|---|"]
    for n in (1, BATCH, 32):
        x = torch.from_numpy(((synthetic.smooth_image(3, (n, 3, SIZE, SIZE)) + 1) / 2).astype(np.float32)).cuda()
        out = torch.empty((n, 2048), device="cuda")
        dev = lambda: model(x, mode=1, out=out)
        eag = lambda: eager(x)
        for fn in (dev, eag):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        d, e = [], []
        for _ in range(3):
            d.append(time_ms(dev, args.iters))
            e.append(time_ms(eag, args.iters))
        a, b = model(x, mode=1).double(), eager(x).double()
        rel = float(((a - b).norm(dim=1) / b.norm(dim=1)).max())
        lines.append("| %d | %s | %s | %.2f | %.3f | %.3f | %.2g |" % (
            n, " ".join("%.3f" % v for v in d), " ".join("%.3f" % v for v in e), statistics.median(d) / statistics.median(e),
            statistics.median(d) / n, total_flops * n / (statistics.median(d) * 1e-3) / PEAK_FP32_MFMA, rel))
        print(lines[-1], flush=True)

    # stage by stage at 8 frames
    n = BATCH
    x = torch.from_numpy(((synthetic.smooth_image(3, (n, 3, SIZE, SIZE)) + 1) / 2).astype(np.float32)).cuda()
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    reps, per_forward = 5, 1 + sum(KERNELS) + 1
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            model(x, mode=1)
        torch.cuda.synchronize()
    ev = sorted((k for k in prof.events() if k.device_type == DeviceType.CUDA), key=lambda k: k.time_range.start)
    ev = [k for k in ev if "lwg" in k.name]
    assert len(ev) == reps * per_forward, "expected %d kernels per forward, the profiler saw %d in %d forwards" % (per_forward, len(ev), reps)
    us = [sum(ev[r * per_forward + k].time_range.elapsed_us() for r in range(reps)) / reps for k in range(per_forward)]
    dev_us, k = [], 1
    for count in KERNELS:
        dev_us.append(sum(us[k:k + count]))
        k += count

    @torch.no_grad()
    def eager_stages():
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(inception_ref.STAGES) + 3)]
        marks[0].record()
        y = inception_ref.preprocess(x, NET)
        marks[1].record()
        for j, name in enumerate(inception_ref.STAGES):
            y = torch.nn.functional.max_pool2d(y, 3, 2) if name.startswith("maxpool") else getattr(net, name)(y)
            marks[j + 2].record()
        torch.nn.functional.adaptive_avg_pool2d(y, 1)
        marks[-1].record()
        torch.cuda.synchronize()
        return [marks[j].elapsed_time(marks[j + 1]) * 1e3 for j in range(len(marks) - 1)]

    eager_stages()
    runs = [eager_stages() for _ in range(reps)]
    eag_us = [statistics.median(r[j] for r in runs) for j in range(len(runs[0]))]
    lines += ["", "## Stage by stage at %d frames" % n, "",
              "liblwg: kernel time under the torch profiler, mean of %d forwards in a run of their own.  eager torch: device events "
              "between the stages of the module (launch gaps included), median of %d." % (reps, reps), "",
              "| stage | output | kernels | GFLOP | liblwg us | TFLOP/s | share of 157.3 TFLOP/s | eager us | liblwg / eager |", "|---|---|---|---|---|---|---|---|---|",
              "| mode + resize | %dx%dx3 | 1 | - | %.1f | - | - | %.1f | %.2f |" % (NET, NET, us[0], eag_us[0], us[0] / eag_us[0])]
    shapes = inception_net.stage_shapes(NET, NET)
    for j, name in enumerate(inception_net.STAGES):
        f = flops[j] * n
        rate = f / (dev_us[j] * 1e-6)
        lines.append("| %s | %dx%dx%d | %d | %s | %.1f | %s | %s | %.1f | %.2f |" % (
            name, shapes[j][0], shapes[j][1], shapes[j][2], KERNELS[j], "%.3f" % (f / 1e9) if f else "-", dev_us[j],
            "%.1f" % (rate / 1e12) if f else "-", "%.3f" % (rate / PEAK_FP32_MFMA) if f else "-", eag_us[j + 1], dev_us[j] / eag_us[j + 1]))
    lines.append("| global pool | 2048 | 1 | - | %.1f | - | - | %.1f | %.2f |" % (us[-1], eag_us[-1], us[-1] / eag_us[-1]))
    tot = sum(us)
    lines.append("| all | | %d | %.3f | %.1f | %.1f | %.3f | %.1f | %.2f |" % (
        per_forward, total_flops * n / 1e9, tot, total_flops * n / (tot * 1e-6) / 1e12, total_flops * n / (tot * 1e-6) / PEAK_FP32_MFMA,
        sum(eag_us), tot / sum(eag_us)))
    print("\n".join(lines[-24:]), flush=True)
    del net

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
    ev = metrics.SetEvaluator(model)
    for t in sorted(seq):
        ev.update(seq[t], truth[t])
    t0 = time.perf_counter()
    r = ev.result()
    host_s = time.perf_counter() - t0
    del seq

    def region(form):
        ev = metrics.SetEvaluator(model) if form else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t, preds in imitator.predict_batches(batches(), 'smooth'):
            if form == 1:
                ev.update(preds)
            elif form == 2:
                ev.update(preds, truth[t])
        if ev is not None:
            assert len(ev.features()[0]) == args.frames     # the device->host copies; the host-side sqrtm is timed apart
        torch.cuda.synchronize()
        return args.frames / (time.perf_counter() - t0)

    forms = (0, 1, 2)
    for form in forms:
        region(form)
    fps = {form: [] for form in forms}
    for _ in range(args.rounds):
        for form in forms:
            fps[form].append(region(form))
    cell = lambda v: "%.0f (%.0f .. %.0f)" % (statistics.median(v), min(v), max(v))
    med = {form: statistics.median(v) for form, v in fps.items()}
    lines += ["", "## The imitation loop (bf16x3) with and without `SetEvaluator.update`", "",
              "frames/s over %d frames in batches of %d, host clock around `predict_batches` ending in a synchronise (with the "
              "evaluator: after the feature tables' device->host copies), forms alternating, median of %d (min .. max)."
              % (args.frames, BATCH, args.rounds), "",
              "| imitation only | + `update(preds)` | + `update(preds, refs)` | preds form / imitation only |", "|---|---|---|---|",
              "| %s | %s | %s | %.3f |" % (cell(fps[0]), cell(fps[1]), cell(fps[2]), med[1] / med[0]), "",
              "What `update` adds per frame, from the medians: %.0f us for the predictions, %.0f us for predictions and references.  "
              "The host side of `result()` (fp64: mean, covariance, the 2048 x 2048 `sqrtm`, the per-batch Inception Score) took "
              "%.1f s, once per sequence." % (1e6 / med[1] - 1e6 / med[0], 1e6 / med[2] - 1e6 / med[0], host_s), "",
              "## Value: the bf16x3 sequence against the exact-fp32 generator (synthetic InceptionV3 weights)", "",
              "| frames | FID | IS (preds) | IS std | IS (refs) |", "|---|---|---|---|---|",
              "| %d | %.4g | %.6g | %.3g | %.6g |" % (r["frames"], r["fid"], r["is"], r["is_std"], r["is_ref"])]
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
