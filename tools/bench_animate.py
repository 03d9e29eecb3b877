"""Timing of motion-driven appearance transfer (models/animator.py) on one GPU: 256 x 256, batch 8, one personalised pair.

    python tools/bench_animate.py [--frames 256] [--rounds 5] [--out profiles/animate.md]

Four forms in one process, alternating, warmed up, both conv arithmetics (bf16x3, fp32):
  (a) `Imitator.predict_batches` on the same box, same source and poses -- context: what one source costs;
  (b) `Animator.predict_batches`, per-frame geometry fused (lwg_animate_inputs);
  (c) the same with `Animator(fused=False)`: the chain of existing entries plus the mask-and-compose expression in torch;
  (d) `Animator.frame_graph(batch=1)` replays with every frame awaited (a device synchronise per frame).
A timed region is `--frames` frames (at least 256) under a host clock and ends in a device synchronise; the figure of a form is the
median of `--rounds` regions, the spread (min .. max) is printed with it.  Before anything is timed, (b) and (c) are compared bit
for bit over the frames of a region.  Also: the fused kernel alone at 32 frames (device events, bytes computed from the shapes).
No GPU: it fails."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.utils import synthetic  # noqa: E402

SIZE, BATCH, PART = 256, 8, "upper_body"


def region_ms_per_frame(fn, frames):
    """host clock around one call of fn (`frames` frames), closed by a device synchronise -> ms per frame"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256, help="frames per timed region (at least 256)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "animate.md"))
    args = ap.parse_args()
    if args.frames < 256 or args.frames % BATCH:
        raise SystemExit("bench_animate: a timed region is at least 256 frames and a multiple of the batch (%d)" % BATCH)
    if not torch.cuda.is_available():
        raise SystemExit("bench_animate: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    n = args.frames
    opt = lambda: demo.default_opt(batch_size=BATCH, image_size=SIZE)
    an, smpl_a, img_a, bg_a = demo.build_synthetic_imitator(batch_size=BATCH, image_size=SIZE, model="animator", opt=opt())
    im, _, _, _ = demo.build_synthetic_imitator(batch_size=BATCH, image_size=SIZE, model="imitator", opt=opt())
    smpl_b = demo.synthetic_smpls(8, seed=3)[5]
    img_b = synthetic.smooth_image(77, (1, 3, SIZE, SIZE))[0]
    smpls = torch.from_numpy(demo.synthetic_smpls(n, seed=0)).cuda()
    chunks = lambda: ((smpls[s:s + BATCH], s) for s in range(0, n, BATCH))

    lines = ["# Motion-driven appearance transfer on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_animate.py --frames %d --rounds %d`: %d x %d, batch %d, `target_part='%s'`, one personalised synthetic "
             "pair, one process.  ms per frame; a timed region is %d frames under a host clock and ends in a device synchronise; the "
             "forms alternate; median of %d regions (min .. max).  (b) and (c) were compared bit for bit over the %d frames before "
             "timing." % (n, args.rounds, SIZE, SIZE, BATCH, PART, n, args.rounds, n), "",
             "| arithmetic | (a) `Imitator` | (b) `Animator`, fused | (c) `Animator(fused=False)` | (c)/(b) | (b)/(a) "
             "| (d) `frame_graph` replays, every frame awaited |",
             "|---|---|---|---|---|---|---|"]
    verdicts = []
    for precision in ("bf16x3", "fp32"):
        an.generator.precision = im.generator.precision = precision
        an.animate_setup(img_a, img_b, src_smpl=smpl_a, ref_smpl=smpl_b, src_bg=bg_a, ref_bg=bg_a)
        an.set_target_part(PART)
        im.personalize(img_a, src_smpl=smpl_a, bg_img=bg_a)
        an.first_cam = im.first_cam = smpls[0:1, 0:3].clone()

        def batches(model, fused=True, keep=None):
            def fn():
                if hasattr(model, 'fused'):
                    model.fused = fused
                for _, preds in model.predict_batches(chunks(), "smooth"):
                    if keep is not None:
                        keep.append(preds.clone())
            return fn

        # (b) == (c) bit for bit at the timed size, before anything is timed
        fused_out, chain_out = [], []
        batches(an, True, fused_out)()
        batches(an, False, chain_out)()
        torch.cuda.synchronize()
        assert len(fused_out) == len(chain_out) == n // BATCH
        for k, (p, q) in enumerate(zip(fused_out, chain_out)):
            assert torch.equal(p, q), "%s: fused and chain differ in batch %d by %g" % (precision, k, float((p - q).abs().max()))
        del fused_out, chain_out

        an.fused = True
        run = an.frame_graph(batch=1)

        def awaited_graph():
            for k in range(n):
                run(smpls[k], t=k)
                torch.cuda.synchronize()

        forms = [("imitator", batches(im)), ("fused", batches(an, True)), ("chain", batches(an, False)), ("graph", awaited_graph)]
        for _, fn in forms:
            for _ in range(2):
                fn()
        ms = {name: [] for name, _ in forms}
        for _ in range(args.rounds):
            for name, fn in forms:
                ms[name].append(region_ms_per_frame(fn, n))
        cell = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("| %s | %s | %s | %s | %.3f | %.3f | %s |" % (
            precision, cell(ms["imitator"]), cell(ms["fused"]), cell(ms["chain"]), med["chain"] / med["fused"],
            med["fused"] / med["imitator"], cell(ms["graph"])))
        print(lines[-1], flush=True)
        # the fused form against the chain, judged against the spread recorded in the same run
        if med["fused"] <= med["chain"]:
            apart = min(ms["chain"]) > max(ms["fused"])
            verdicts.append("%s: fused is %.1f %% faster than the chain (medians)%s." % (
                precision, 100 * (med["chain"] / med["fused"] - 1), "; the min..max ranges do not overlap" if apart else
                "; the min..max ranges overlap, so the difference is inside the spread"))
        else:
            beyond = min(ms["fused"]) > max(ms["chain"])
            verdicts.append("%s: fused does NOT win: %.1f %% slower than the chain (medians), %s." % (
                precision, 100 * (med["fused"] / med["chain"] - 1), "beyond the min..max spread" if beyond else
                "inside the min..max spread"))
        del run
        an.fused = True

    # the fused kernel alone at 32 frames
    frames = 32
    tab = an._pair_tables(PART)
    an.transfer_params_by_smpl(smpls[:frames], "smooth", t=1)
    fim, wim = an.tsf_info["fim"], an.tsf_info["wim"]
    call = lambda: an.render.animate_inputs(fim, wim, tab["side"], tab["src_f2p"], tab["ref_f2p"], an.src_info["img"], an.ref_info["img"])
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    iters = 200
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        call()
    stop.record()
    torch.cuda.synchronize()
    us = start.elapsed_time(stop) * 1e3 / iters
    nc = an.render.map_fn.shape[1]
    # per pixel: fim 4 + wim 12 in; two flows 16, cond 4 nc, tsf_img 12, the NHWC8 pixel 32 out.  The two 24-byte face gathers of a
    # covered pixel, its side byte and the image taps hit tables and images that stay in cache and are not counted.
    per_pixel = 4 + 12 + 16 + 4 * nc + 12 + 32
    total = frames * SIZE * SIZE * per_pixel
    covered = float((fim >= 0).float().mean())
    lines += ["", "; ".join(verdicts), "",
              "`lwg_animate_inputs` alone, %d frames of %d x %d (%.0f %% of the pixels covered): %.1f us per call (device events over "
              "%d back-to-back calls, launch included); %d B per pixel computed from the shapes (16 in, %d out; face gathers and "
              "image taps come from cache and are not counted) = %.1f MB, %.0f GB/s -- back-to-back calls on the same buffers, whose bytes fit the "
              "256 MiB last-level cache: a rate of the cache hierarchy, not of HBM."
              % (frames, SIZE, SIZE, 100 * covered, us, iters, per_pixel, per_pixel - 16, total / 1e6, total / (us * 1e-6) / 1e9)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
