"""Timing of the device JPEG encoder (csrc/jpeg.hip) and of the frame writers on one GPU: 256 x 256, batch 8, both conv
arithmetics, the synthetic sequence.

    python tools/bench_jpeg.py [--frames 256] [--rounds 5] [--out profiles/jpeg.md]

Two measurements, in one process, warmed up:
  (a) `lwg_jpeg_encode` alone on one batch of generator output (util.jpeg_encode: the launch sequence, its output and workspace
      allocations from PyTorch's caching allocator included), device events over back-to-back calls: quality 75 and 95, 4:2:0
      and 4:4:4; with the bytes of the streams and of the float frames they replace;
  (b) frames/s of `Imitator.inference_by_smpls(output_dir=tmp)` over `--frames` frames with and without `device_jpeg`: a host
      clock around the whole call (the files are written when it returns), the two forms alternating, median of `--rounds`
      (min .. max).  The output directory is a fresh temporary one (the machine's default temporary directory).
No GPU: it fails."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.utils import util  # noqa: E402

SIZE, BATCH = 256, 8


def encode_us(preds, quality, subsampling, iters=200):
    for _ in range(5):
        util.jpeg_encode(preds, quality=quality, subsampling=subsampling)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        util.jpeg_encode(preds, quality=quality, subsampling=subsampling)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "jpeg.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    imitator, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(batch_size=BATCH, image_size=SIZE)
    smpls = demo.synthetic_smpls(args.frames, seed=0)
    lines = ["# Device JPEG encoder on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_jpeg.py --frames %d --rounds %d`: %d x %d, batch %d, the synthetic sequence, one process."
             % (args.frames, args.rounds, SIZE, SIZE, BATCH), ""]
    enc_lines = ["## `lwg_jpeg_encode` alone", "",
                 "One batch of %d generator outputs (frames 0..%d of the sequence); us per call from device events over 200 "
                 "back-to-back calls of `util.jpeg_encode` (launches and allocations included); bytes per frame that cross to the "
                 "host (`util.jpeg_bytes`) against the %d bytes of the float32 frame." % (BATCH, BATCH - 1, 3 * SIZE * SIZE * 4), "",
                 "| arithmetic | quality | subsampling | us per batch | us per frame | stream bytes per frame (mean) | float bytes / stream bytes |",
                 "|---|---|---|---|---|---|---|"]
    e2e_lines = ["## Writing %d frames: `inference_by_smpls(output_dir=...)`" % args.frames, "",
                 "frames/s, host clock around the whole call (files written), forms alternating, median of %d (min .. max)." % args.rounds,
                 "", "| arithmetic | host writer (float copy, numpy, PIL) | `device_jpeg=True` | ratio |", "|---|---|---|---|"]
    for precision in ("bf16x3", "fp32"):
        imitator.generator.precision = precision
        imitator.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
        imitator.first_cam = torch.as_tensor(smpls[0:1, 0:3]).float().cuda()
        preds = imitator.forward(imitator.transfer_params_by_smpl(torch.as_tensor(smpls[:BATCH]).float().cuda(), 'smooth', t=1),
                                 imitator.tsf_info['T']).clone()
        for quality, sub in ((75, '4:2:0'), (95, '4:2:0'), (75, '4:4:4'), (95, '4:4:4')):
            us = encode_us(preds, quality, sub)
            nbytes = statistics.mean(len(s) for s in util.jpeg_bytes(preds, quality=quality, subsampling=sub))
            enc_lines.append("| %s | %d | %s | %.1f | %.1f | %.0f | %.0f |" % (precision, quality, sub, us, us / BATCH, nbytes,
                                                                              3 * SIZE * SIZE * 4 / nbytes))
            print(enc_lines[-1], flush=True)

        def region(device_jpeg):
            out = tempfile.mkdtemp(prefix="bench_jpeg_")
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = imitator.inference_by_smpls(smpls, cam_strategy='smooth', output_dir=out, device_jpeg=device_jpeg)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert len(res) == args.frames and len(os.listdir(out)) == args.frames
            finally:
                shutil.rmtree(out, ignore_errors=True)
            return args.frames / dt

        for flag in (False, True):          # warm: every shape, both writers
            region(flag)
        fps = {False: [], True: []}
        for _ in range(args.rounds):
            for flag in (False, True):
                fps[flag].append(region(flag))
        cell = lambda v: "%.0f (%.0f .. %.0f)" % (statistics.median(v), min(v), max(v))
        e2e_lines.append("| %s | %s | %s | %.2f |" % (precision, cell(fps[False]), cell(fps[True]),
                                                    statistics.median(fps[True]) / statistics.median(fps[False])))
        print(e2e_lines[-1], flush=True)
    text = "\n".join(lines + enc_lines + [""] + e2e_lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
