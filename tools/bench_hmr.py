"""Timing of the HMR regressor (networks/hmr.py, csrc/hmr.hip) on one GPU:

    python tools/bench_hmr.py [--iters 50] [--out profiles/hmr.md]

For batch 1 and batch 8, warm: the device path (liblwg) against torch-ROCm's eager forward of the SAME module on the same GPU in
the same process (`forward_ops` on CUDA), timed with device events over `--iters` forwards, the two alternating, three rounds
(the spread is printed).  Then, in a run of its own under the torch profiler, the device path's kernel times grouped by stage
(the launch order is fixed: layout, stem, max pool, the blocks' convolutions, pool, regressor) with the FLOPs of each stage
computed from the shapes and the achieved share of the 157.3 TFLOP/s fp32 MFMA peak of the MI355X.  No GPU: it fails.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd.networks import batch_smpl  # noqa: E402
from impersonator_amd.networks import hmr as hmr_net  # noqa: E402
from impersonator_amd.utils import synthetic  # noqa: E402

PEAK_FP32_MFMA = 157.3e12


def stage_plan(num_blocks=(3, 4, 6, 3)):
    """[(stage, kernel launches, FLOPs per image)] in launch order (2 * M * N * K per convolution, padding counted)."""
    plan = [("layout+stem+maxpool", 3, 2.0 * 112 * 112 * 64 * 147)]
    H, cin = 56, 64
    for li, (p, nb) in enumerate(zip((64, 128, 256, 512), num_blocks)):
        launches, flops = 0, 0.0
        for i in range(nb):
            s = (2, 2, 2, 1)[li] if (i > 0 and i == nb - 1) else 1
            Ho = (H + 2 - 3) // s + 1
            if cin != 4 * p:
                launches += 1
                flops += 2.0 * H * H * cin * 4 * p
            launches += 3
            flops += 2.0 * H * H * cin * p + 2.0 * Ho * Ho * 9 * p * p + 2.0 * Ho * Ho * p * 4 * p
            H, cin = Ho, 4 * p
        plan.append(("layer%d" % (li + 1), launches, flops))
    plan.append(("pool+regressor", 1 + 1 + 9, 3 * 2.0 * (1024 * 2133 + 1024 * 1024 + 85 * 1024)))
    return plan


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
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hmr: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    m = hmr_net.HumanModelRecovery(smpl_params=batch_smpl.synthetic_smpl_params(0), max_batch=8).eval()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.hmr_state_dict(0).items()}
    for k, v in m.smpl.state_dict().items():
        sd["smpl." + k] = v
    m.load_state_dict(sd)
    m.cuda()
    plan = stage_plan()
    flops_img = sum(f for _, _, f in plan)
    lines = ["# HMR regressor on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_hmr.py --iters %d`: warm forwards timed with device events, device path and eager torch "
             "alternating in one process; %.2f GFLOP per image." % (args.iters, flops_img / 1e9), "",
             "| batch | liblwg ms (3 rounds) | eager torch ms (3 rounds) | liblwg / eager | liblwg share of fp32 MFMA peak |",
             "|---|---|---|---|---|"]
    with torch.no_grad():
        for bs in (1, 8):
            x = torch.from_numpy(synthetic.smooth_image(3, (bs, 3, 224, 224))).cuda()
            dev = lambda: m(x)
            eager = lambda: m.forward_ops(x)
            for fn in (dev, eager):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            d, e = [], []
            for _ in range(3):
                d.append(time_ms(dev, args.iters))
                e.append(time_ms(eager, args.iters))
            diff = float((m(x) - m.forward_ops(x)).abs().max())
            lines.append("| %d | %s | %s | %.2f | %.3f |" % (bs, " ".join("%.3f" % v for v in d), " ".join("%.3f" % v for v in e),
                                                             min(d) / min(e), flops_img * bs / (min(d) * 1e-3) / PEAK_FP32_MFMA))
            print(lines[-1], "  max |theta_device - theta_eager| = %.3g" % diff)
        # kernel times by stage: a run of its own under the profiler
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        for bs in (1, 8):
            x = torch.from_numpy(synthetic.smooth_image(3, (bs, 3, 224, 224))).cuda()
            m(x)
            torch.cuda.synchronize()
            reps = 5
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    m(x)
                torch.cuda.synchronize()
            ev = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
            per = sum(n for _, n, _ in plan)
            assert len(ev) == reps * per, "expected %d kernels per forward, the profiler saw %d in %d forwards" % (per, len(ev), reps)
            lines += ["", "Batch %d, kernel time by stage (mean of %d profiled forwards):" % (bs, reps), "",
                      "| stage | kernels | GFLOP | ms | TFLOP/s | share of 157.3 TFLOP/s |", "|---|---|---|---|---|---|"]
            k0 = 0
            for name, n, flops in plan:
                us = sum(ev[r * per + k0 + j].time_range.elapsed_us() for r in range(reps) for j in range(n)) / reps
                k0 += n
                rate = flops * bs / (us * 1e-6)
                lines.append("| %s | %d | %.3f | %.3f | %.1f | %.3f |" % (name, n, flops * bs / 1e9, us / 1e3, rate / 1e12, rate / PEAK_FP32_MFMA))
                print(lines[-1])
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
