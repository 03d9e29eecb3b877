"""Timing and observed errors of the textured-rendering half of SMPLRenderer (utils/nmr.py, csrc/render.hip) on one GPU:

    python tools/bench_render.py [--iters 100] [--out profiles/render.md]

At 256 x 256, batch 8, the SMPL-sized synthetic mesh (6890 / 13776), tex_size 3: ms per call of `render` (anti-aliasing on and
off), `render_silhouettes` and `extract_tex_from_image`, with `render_fim_wim` on the same box as the yardstick -- warm calls timed
with device events, three rounds each.  Then, in a run of its own under the torch profiler, the kernel times of one anti-aliased
`render` and the shading kernel's achieved bytes/s over its compulsory traffic (the maps it reads once and the picture it writes;
the gathered texels, lights and face depths are reused through the caches and not counted).  Last, the observed distance of
`render` from the float64 restatement on the CPU oracle rasteriser's maps, on the inputs of tests/test_gpu_render.py.
Numbers are recorded, not gated.  No GPU: it fails.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd.utils import synthetic  # noqa: E402
from impersonator_amd.utils.nmr import SMPLRenderer  # noqa: E402

PEAK_HBM = 8.0e12       # bytes/s, MI355X
SIZE, BATCH, TEX = 256, 8, 3


def time_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def shade_bytes(bs, image_size, anti_aliasing):
    """compulsory traffic of lwg_shade_resolve: fim + wim + depth (4 + 12 + 4 B per sub-pixel) in, three floats per pixel out"""
    S = image_size * (2 if anti_aliasing else 1)
    return bs * S * S * 20 + bs * image_size * image_size * 12


def observed_errors():
    from oracle import raster as oracle_raster
    from tests import render_ref as rr
    rows = []
    for image_size in (64, 100):
        sc = rr.scene(image_size)
        bs, nf = sc["f2verts"].shape[:2]
        cam, verts = torch.from_numpy(sc["cam"]).cuda(), torch.from_numpy(sc["verts"]).cuda()
        for aa in (True, False):
            S = image_size * (2 if aa else 1)
            maps = oracle_raster.rasterize_fim_wim(sc["f2verts"], S, 0.1, 25.0)
            for ts in (3, 2):
                for light in ("default", "ambient"):
                    r = SMPLRenderer(image_size=image_size, faces=sc["faces"], map_fn=np.zeros((nf + 1, 3), np.float32),
                                     anti_aliasing=aa, tex_size=ts, background_color=(0.2, -0.3, 0.5)).cuda()
                    if light == "ambient":
                        r.set_ambient_light()
                    tex = rr.random_textures(bs, nf, ts, seed=ts)
                    img, _ = r.render(cam, verts, torch.from_numpy(tex).cuda())
                    want = rr.render(sc["f2verts"], sc["raw"], *maps, tex, (0.2, -0.3, 0.5), ts, aa,
                                     light=rr.AMBIENT_LIGHT if light == "ambient" else rr.DEFAULT_LIGHT)
                    rows.append((image_size, aa, ts, light, float(np.abs(img.cpu().numpy().astype(np.float64) - want).max())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    rest, faces = synthetic.body_mesh()
    map_fn = synthetic.uv_seg_map_fn(rest, faces)
    verts = torch.from_numpy(np.stack([synthetic.motion_verts(rest, 100 * t) for t in range(BATCH)])).cuda()
    cam = torch.from_numpy(synthetic.cams(BATCH, seed=5)).cuda()
    frames = torch.from_numpy(synthetic.smooth_image(3, (BATCH, 3, SIZE, SIZE))).cuda()
    aa_r = SMPLRenderer(image_size=SIZE, faces=faces, map_fn=map_fn, tex_size=TEX, anti_aliasing=True).cuda()
    no_r = SMPLRenderer(image_size=SIZE, faces=faces, map_fn=map_fn, tex_size=TEX, anti_aliasing=False).cuda()
    for r in (aa_r, no_r):
        r.set_ambient_light()
    tex = aa_r.extract_tex_from_image(frames, cam, verts)
    calls = [("render, anti-aliasing on", lambda: aa_r.render(cam, verts, tex)),
             ("render, anti-aliasing off", lambda: no_r.render(cam, verts, tex)),
             ("render_silhouettes (anti-aliasing on)", lambda: aa_r.render_silhouettes(cam, verts)),
             ("extract_tex_from_image", lambda: aa_r.extract_tex_from_image(frames, cam, verts)),
             ("render_fim_wim (yardstick)", lambda: aa_r.render_fim_wim(cam, verts))]
    variant = "four lanes per pixel (measurement build, LWG_LIB=exp LWG_SHADE=quad)" \
        if os.environ.get("LWG_LIB") == "exp" and os.environ.get("LWG_SHADE", "").startswith("q") else "one lane per output pixel"
    lines = ["# Textured rendering on %s" % torch.cuda.get_device_name(0), "", "Shading kernel's thread mapping: %s." % variant, "",
             "`python tools/bench_render.py --iters %d`: %d x %d, batch %d, %d vertices / %d faces, tex_size %d; warm calls timed "
             "with device events, the calls taking turns, three rounds." % (args.iters, SIZE, SIZE, BATCH, rest.shape[0],
                                                                           faces.shape[0], TEX), "",
             "| call | ms per call (3 rounds) |", "|---|---|"]
    for _, fn in calls:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name, _ in calls}
    for _ in range(3):
        for name, fn in calls:
            rounds[name].append(time_ms(fn, args.iters))
    for name, _ in calls:
        lines.append("| %s | %s |" % (name, " ".join("%.3f" % v for v in rounds[name])))

    # kernel times of one anti-aliased render: a run of its own under the profiler
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    reps = 10
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            aa_r.render(cam, verts, tex)
        torch.cuda.synchronize()
    us = {}
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            key = next((k for k in ("project_faces", "raster_setup", "raster_tile", "face_light", "shade_resolve") if k in e.name), e.name)
            us[key] = us.get(key, 0.0) + e.time_range.elapsed_us() / reps
    lines += ["", "Kernels of one `render` (anti-aliasing on), mean of %d profiled calls:" % reps, "", "| kernel | us |", "|---|---|"]
    lines += ["| %s | %.1f |" % kv for kv in us.items()]
    nbytes = shade_bytes(BATCH, SIZE, True)
    rate = nbytes / (us["shade_resolve"] * 1e-6)
    lines += ["", "Shading kernel: %.1f MB of compulsory traffic (maps in, picture out) in %.1f us = %.2f TB/s, %.0f %% of the "
              "%.1f TB/s HBM peak.  Memory-bound gather; no matrix work." % (nbytes / 1e6, us["shade_resolve"], rate / 1e12,
                                                                           100 * rate / PEAK_HBM, PEAK_HBM / 1e12)]

    lines += ["", "Observed max |render - float64 restatement on the oracle's maps| (bound of the tests: 5e-6), inputs of "
              "tests/test_gpu_render.py:", "", "| image_size | anti-aliasing | tex_size | light | max abs error |", "|---|---|---|---|---|"]
    lines += ["| %d | %s | %d | %s | %.2e |" % (s, "on" if aa else "off", ts, light, err) for s, aa, ts, light, err in observed_errors()]
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
