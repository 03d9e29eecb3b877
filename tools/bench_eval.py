"""Timing of the paired evaluation (csrc/eval.hip, utils/metrics.py) on one GPU: 256 x 256, batch 8, both conv arithmetics, the
synthetic sequence; and the SSIM / PSNR of each arithmetic against the exact-fp32 generator.

    python tools/bench_eval.py [--frames 256] [--rounds 5] [--out profiles/eval.md]

Measurements, in one process, warmed up:
  (a) `lwg_eval_pair_stats` alone on one batch (metrics.pair_stats: both kernels, the stats and workspace allocations from
      PyTorch's caching allocator included), device events over back-to-back calls, the three pixel modes; `lwg_resize_bilinear`
      256 -> 224 likewise;
  (b) frames/s of the imitation loop (Imitator.predict_batches over `--frames` frames) with and without
      `PairedEvaluator.update` in it, host clock around the loop ending in a synchronise (with the evaluator: in `result()`'s one
      copy), the two forms alternating, median of `--rounds` (min .. max);
  (c) the host route the evaluator replaces: the float frames copied to the host and scored by the numpy/scipy formulation of
      tests/metrics_ref.py, frames/s over 16 frames of ready device tensors (no imitation in the window);
  (d) the values: SSIM / PSNR of the sequence in each arithmetic against the exact-fp32 frames, as they are and through the
      8-bit quantiser.
No GPU: it fails."""
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
from impersonator_amd.utils import metrics  # noqa: E402
from tests import metrics_ref  # noqa: E402

SIZE, BATCH = 256, 8


def call_us(fn, iters=200):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "eval.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    imitator, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(batch_size=BATCH, image_size=SIZE)
    smpls = torch.as_tensor(demo.synthetic_smpls(args.frames, seed=0)).float().cuda()
    batches = lambda: ((smpls[s:s + BATCH], s) for s in range(0, args.frames, BATCH))

    def sequence(precision):
        imitator.generator.precision = precision
        imitator.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
        imitator.first_cam = smpls[0:1, 0:3].clone()
        return {t: p for t, p in imitator.predict_batches(batches(), 'smooth')}

    truth = sequence("fp32")
    lines = ["# Paired evaluation on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_eval.py --frames %d --rounds %d`: %d x %d, batch %d, the synthetic sequence, one process."
             % (args.frames, args.rounds, SIZE, SIZE, BATCH), ""]
    k_lines = ["## The kernels alone", "",
               "One batch of %d frames against the exact-fp32 frames; us per call from device events over 200 back-to-back calls "
               "(launches and allocations included)." % BATCH, "",
               "| call | us per batch | us per frame |", "|---|---|---|"]
    v_lines = ["## Values: the sequence against the exact-fp32 generator", "",
               "Means over %d frames (the worst frame in brackets); `quantize` = both sides through the truncating 8-bit "
               "round trip (mode 2)." % args.frames, "",
               "| arithmetic | mode | 1 - SSIM | PSNR (dB) | largest per-frame MSE |", "|---|---|---|---|---|"]
    l_lines = ["## The imitation loop with and without `PairedEvaluator.update`", "",
               "frames/s over %d frames, host clock around `predict_batches` ending in a synchronise (with the evaluator: in "
               "`result()`), forms alternating, median of %d (min .. max)." % (args.frames, args.rounds), "",
               "| arithmetic | imitation only | + `update(preds, truth)` (ssim, psnr) | ratio |", "|---|---|---|---|"]

    cost = {}
    a, b = sequence("bf16x3")[0], truth[0]
    for mode in (0, 1, 2):
        us = call_us(lambda: metrics.pair_stats(a, b, mode=mode))
        k_lines.append("| `pair_stats` mode %d | %.1f | %.1f |" % (mode, us, us / BATCH))
        print(k_lines[-1], flush=True)
    us = call_us(lambda: metrics.resize_bilinear(a, (224, 224)))
    k_lines.append("| `resize_bilinear` 256 -> 224 | %.1f | %.1f |" % (us, us / BATCH))
    print(k_lines[-1], flush=True)

    for precision in ("bf16x3", "fp32"):
        seq = sequence(precision)
        for mode, name in ((0, "as emitted"), (2, "quantize")):
            ev = metrics.PairedEvaluator(("ssim", "psnr"), mode=mode)
            for t in sorted(seq):
                ev.update(seq[t], truth[t])
            r = ev.result()
            pf = r["per_frame"]
            v_lines.append("| %s | %s | %.3g (%.3g) | %.2f (%.2f) | %.3g |" % (precision, name, 1 - r["ssim"], 1 - pf["ssim"].min(),
                                                                            r["psnr"], pf["psnr"].min(), pf["mse"].max()))
            print(v_lines[-1], flush=True)
        del seq

        def region(with_eval):
            ev = metrics.PairedEvaluator(("ssim", "psnr"))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t, preds in imitator.predict_batches(batches(), 'smooth'):
                if with_eval:
                    ev.update(preds, truth[t])
            if with_eval:
                assert ev.result()["frames"] == args.frames
            torch.cuda.synchronize()
            return args.frames / (time.perf_counter() - t0)

        for flag in (False, True):
            region(flag)
        fps = {False: [], True: []}
        for _ in range(args.rounds):
            for flag in (False, True):
                fps[flag].append(region(flag))
        cell = lambda v: "%.0f (%.0f .. %.0f)" % (statistics.median(v), min(v), max(v))
        l_lines.append("| %s | %s | %s | %.3f |" % (precision, cell(fps[False]), cell(fps[True]),
                                                    statistics.median(fps[True]) / statistics.median(fps[False])))
        print(l_lines[-1], flush=True)
        cost[precision] = 1e6 / statistics.median(fps[True]) - 1e6 / statistics.median(fps[False])
    l_lines += ["", "What `update` adds per frame, from the medians: %s.  `pair_stats` runs on the stream the frames are handed over on, after "
                "the generator lanes' kernels, so the loop pays at most the kernels' own time (first table); the spread between "
                "rounds is of the same size as the difference."
                % ", ".join("%.1f us (%s)" % (cost[k], k) for k in cost)]

    # the host route: float copy + numpy/scipy, on frames that are already there
    n_host = 16
    pa, pb = torch.cat([a, a]), torch.cat([b, b])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ha, hb = pa.cpu().numpy(), pb.cpu().numpy()
    t_copy = time.perf_counter() - t0
    host = metrics_ref.pair_stats(ha, hb, 0)
    t_host = time.perf_counter() - t0
    dev = metrics.pair_stats(pa, pb).cpu().numpy()
    h_lines = ["## The host route it replaces", "",
               "%d frames that are ready on the device: `.cpu()` of both float batches (%.1f MB), then `tests/metrics_ref.pair_stats` "
               "(numpy fp64, `scipy.ndimage.uniform_filter`), one host thread pool as the machine gives it." % (n_host, 2 * pa.numel() * 4 / 1e6), "",
               "| copy (ms per frame) | copy + numpy/scipy (ms per frame) | frames/s | largest abs difference of mssim to the device |",
               "|---|---|---|---|",
               "| %.3f | %.2f | %.1f | %.3g |" % (t_copy * 1e3 / n_host, t_host * 1e3 / n_host, n_host / t_host,
                                                float(np.abs(host[:, 0] - dev[:, 0]).max()))]
    print(h_lines[-1], flush=True)
    text = "\n".join(lines + k_lines + [""] + l_lines + [""] + h_lines + [""] + v_lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
