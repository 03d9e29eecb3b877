"""Timing of novel view synthesis (models/viewer.py) on one GPU: a 16-view turntable at 256 x 256, one personalised source.

    python tools/bench_view.py [--turns 20] [--rounds 5] [--out profiles/view.md]

Three forms of the same computation (bit-identical results, tests/test_gpu_views.py), in one process, alternating, warmed up:
  (a) a loop of `Viewer.view`            -- one view per call at batch 1, launched kernel by kernel from Python;
  (b) a loop of `Viewer.view_graph` replays -- one view per call, one graph launch;
  (c) `Viewer.views` at batch_size 8 and 16 -- blocks of views per launch sequence.
A timed region is `--turns` turntables (16 * turns views) under a host clock and ends in a device synchronise; the figure of a
form is the median of `--rounds` regions, the spread (min .. max) is printed with it.  (a) and (b) are also timed with every view
awaited (a device synchronise per view: a caller that consumes each picture before asking for the next, as the reference's loop
does).  Both conv arithmetics (bf16x3, fp32) are measured.  Also: `image_grid_u8` of the 16 views alone (device events) and the one device->host copy of its bytes.
No GPU: it fails."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import run_view  # noqa: E402
from impersonator_amd import demo  # noqa: E402
from impersonator_amd.utils import util  # noqa: E402

VIEWS, SIZE = 16, 256


def region_ms_per_view(fn, turns):
    """host clock around `turns` calls of fn (each one turntable), closed by a device synchronise -> ms per view"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(turns):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (turns * VIEWS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=20, help="turntables of 16 views per timed region")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "view.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_view: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    rts, ts = run_view.view_schedule(run_view.parse_view_params('R=0,90,0/t=0,0,0'), VIEWS)
    vw, smpl, img, bg = demo.build_synthetic_imitator(batch_size=16, image_size=SIZE, model="viewer",
                                                      opt=demo.default_opt(batch_size=16, image_size=SIZE))
    lines = ["# Novel views on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_view.py --turns %d --rounds %d`: a %d-view turntable at %d x %d from one personalised synthetic "
             "source, one process.  ms per view; a timed region is %d views under a host clock and ends in a device synchronise; "
             "the forms alternate; median of %d regions (min .. max)." % (args.turns, args.rounds, VIEWS, SIZE, SIZE,
                                                                           args.turns * VIEWS, args.rounds), "",
             "| arithmetic | (a) loop of `view` | (b) `view_graph` replays | (c) `views`, batch 8 | (c) `views`, batch 16 | (a)/(b) | (a)/(c16) "
             "| (a) every view awaited | (b) every view awaited |",
             "|---|---|---|---|---|---|---|---|---|"]
    preds = None
    for precision in ("bf16x3", "fp32"):
        vw.generator.precision = precision
        vw.personalize(img, src_smpl=smpl, bg_img=bg)
        run = vw.view_graph(batch=1)

        def loop_view():
            for k in range(VIEWS):
                vw.view(rts[k], ts[k])

        def loop_graph():
            for k in range(VIEWS):
                run(rts[k], ts[k])

        def awaited(step):
            """every view awaited before the next is issued: the regime of a caller that consumes each picture (the reference's loop)"""
            def fn():
                for k in range(VIEWS):
                    step(rts[k], ts[k])
                    torch.cuda.synchronize()
            return fn

        def views_at(bs):
            def fn():
                vw._opt.batch_size = bs
                return vw.views(rts, ts)
            return fn

        forms = [("view", loop_view), ("graph", loop_graph), ("views8", views_at(8)), ("views16", views_at(16)),
                 ("view_awaited", awaited(vw.view)), ("graph_awaited", awaited(run))]
        # the forms compute the same pictures: checked here at the timed size before anything is timed
        single = torch.cat([vw.view(rts[k], ts[k]) for k in range(VIEWS)])
        replay = torch.cat([run(rts[k], ts[k]).clone() for k in range(VIEWS)])
        preds = views_at(16)()
        for name, other in (("view_graph", replay), ("views at batch 16", preds), ("views at batch 8", views_at(8)())):
            assert torch.equal(single, other), "%s (%s) differs from the loop of view by %g" % (
                name, precision, float((single - other).abs().max()))
        for _, fn in forms:
            for _ in range(2):
                fn()
        ms = {name: [] for name, _ in forms}
        for _ in range(args.rounds):
            for name, fn in forms:
                ms[name].append(region_ms_per_view(fn, args.turns))
        cell = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("| %s | %s | %s | %s | %s | %.2f | %.2f | %s | %s |" % (
            precision, cell(ms["view"]), cell(ms["graph"]), cell(ms["views8"]), cell(ms["views16"]), med["view"] / med["graph"],
            med["view"] / med["views16"], cell(ms["view_awaited"]), cell(ms["graph_awaited"])))
        print(lines[-1], flush=True)
        del run

    # the image grid of the 16 views: the kernel alone, and the one copy of its bytes to the host
    grid = util.image_grid_u8(preds, normalize=True)
    torch.cuda.synchronize()
    iters = 200
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        util.image_grid_u8(preds, normalize=True)
    stop.record()
    torch.cuda.synchronize()
    grid_us = start.elapsed_time(stop) * 1e3 / iters
    copies = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid.cpu()
        copies.append((time.perf_counter() - t0) * 1e6)
    in_bytes, out_bytes = preds.numel() * 4, grid.numel()
    lines += ["", "`image_grid_u8` of the %d views (%d x %d x 3 bytes out, %.1f MB read + %.1f MB written): %.1f us per call "
              "(device events over %d back-to-back calls, launch included), %.0f GB/s.  The one device->host copy of the bytes "
              "(pageable host memory, synchronous): median %.0f us (min %.0f)."
              % (VIEWS, grid.shape[0], grid.shape[1], in_bytes / 1e6, out_bytes / 1e6, grid_us, iters,
                 (in_bytes + out_bytes) / (grid_us * 1e-6) / 1e9, statistics.median(copies), min(copies))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
