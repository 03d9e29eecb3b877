"""Timing of the Swapper's fine-tune (impersonator_amd/models/post_tune.py: SwapTuner) on one GPU:

    python tools/bench_swap_tune.py [--rounds 3] [--out profiles/swap_tune.md]

1. The 50-step tune at 256x256 on the batch of the synthetic Swapper's two subjects (swap_samples), at bs 2 and bs 1, conv_precision
   fp32 and bf16x3: the eager loop (`optimize()`: ~1500 launches per iteration issued from Python) against the graphed one
   (`optimize_graphed()`: two eager warm-up iterations, one capture, 47 replays -- capture included), alternating in one process,
   three rounds.  A host clock around the whole loop, ending in a synchronise; every round starts from a new tuner (its
   construction is outside the clock).
2. The whole-gradient distances from float64 CPU autograd on the GPU test's batch (tests/test_gpu_swap_tune.py).
No GPU: it fails."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd import demo  # noqa: E402
from impersonator_amd.models.post_tune import SwapTuner, swap_samples  # noqa: E402
from impersonator_amd.utils import synthetic  # noqa: E402

SIZE = 256


def tune_ms(swapper, sample, precision, batch_size, graphed):
    """wall time of the 50 steps, milliseconds"""
    tuner = SwapTuner(swapper.generator, sample['bg'], swapper.render, conv_precision=precision, batch_size=batch_size)
    tuner.load(sample)
    torch.cuda.synchronize()
    start = time.perf_counter()
    tuner.run(graphed=graphed)              # ends in the read-back of the history: a synchronise
    torch.cuda.synchronize()
    ms = (time.perf_counter() - start) * 1e3
    if graphed and (tuner.captures != 1 or tuner.replays != tuner.total - 2):
        raise SystemExit("bench_swap_tune: the graphed loop fell back to eager iterations")
    return ms


def gradient_distances():
    """whole-gradient relative L2 from float64 CPU autograd on the batch of tests/test_gpu_swap_tune.py"""
    from oracle import torch_ref
    from tests import helpers
    from tests import post_tune_ref as ref
    from tests import swap_tune_ref as sref
    from impersonator_amd.networks.generator import ImpersonatorGenerator
    gsd = torch_ref.state_dict_from_numpy(helpers.generator_state_dict(seed=2, affine="random"))
    G = ImpersonatorGenerator(bg_dim=4, src_dim=6, tsf_dim=6, repeat_num=6, image_size=128, max_batch=2)
    G.load_state_dict(gsd)
    sample = ref.sample_batch(seed=5, n=2, size=64, nf=40)
    bg = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1
    render = ref.TableRender(40, seed=3)
    dbl = lambda d: {k: v.double() for k, v in d.items()}
    g64 = sref.steps(dbl(gsd), dbl(sample), bg.double(), 4, 1, n_steps=1)[1]
    g32 = sref.steps(gsd, sample, bg, 4, 1, n_steps=1)[1]
    cut = sref.steps(dbl(gsd), dbl(sample), bg.double(), 4, 1, n_steps=1, cut_cycle=True)[1]

    def dist(g):
        num = sum(float(((g[k].double() - v) ** 2).sum()) for k, v in g64.items() if v is not None)
        return (num / sum(float((v ** 2).sum()) for v in g64.values() if v is not None)) ** 0.5

    out = {"CPU float32 autograd": dist(g32), "float64 autograd, cycle inputs detached": dist(cut)}
    for precision in ("fp32", "bf16x3"):
        t = SwapTuner(G, bg, render, conv_precision=precision)
        t.forward(sample)
        t.backward()
        out["device, conv_precision=%s" % precision] = dist(t.gradients())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_swap_tune: no GPU visible; timings are taken on an MI355X only")
    torch.cuda.set_device(0)
    sw, smpl_a, img_a, bg_a = demo.build_synthetic_imitator(batch_size=1, image_size=SIZE, model="swapper",
                                                            opt=demo.default_opt(batch_size=2, image_size=SIZE, post_tune=True))
    smpl_b = demo.synthetic_smpls(8, seed=3)[5]
    img_b = synthetic.smooth_image(77, (1, 3, SIZE, SIZE))[0]
    sw.swap_setup(img_a, img_b, src_smpl=smpl_a, tgt_smpl=smpl_b, src_bg=bg_a, tgt_bg=bg_a)
    sample = swap_samples(sw)
    cases = [(p, bs) for bs in (2, 1) for p in ("fp32", "bf16x3")]
    res = {(c, g): [] for c in cases for g in (False, True)}
    for c in cases:                        # every shape and kernel variant warm before the first timed loop
        tune_ms(sw, sample, c[0], c[1], True)
    for _ in range(args.rounds):
        for c in cases:
            for g in (False, True):
                res[(c, g)].append(tune_ms(sw, sample, c[0], c[1], g))
    fmt = lambda ms: " / ".join("%.0f" % v for v in ms)
    lines = ["# The Swapper's fine-tune on %s" % torch.cuda.get_device_name(0), "",
             "`python tools/bench_swap_tune.py --rounds %d`: %d steps of `SwapTuner` at %dx%d on the synthetic Swapper's two subjects; "
             "a host clock around the whole loop, ending in a synchronise; eager and graphed loops alternate in one process.  The "
             "graphed loop is two eager warm-up iterations, one capture and %d replays, all inside the clock." % (
                 args.rounds, SwapTuner.TOTAL, SIZE, SIZE, SwapTuner.TOTAL - 2), "",
             "| bs | conv_precision | eager loop, ms (%d rounds) | graphed loop, ms (%d rounds) | graphed / eager (best rounds) | "
             "graphed faster in every round |" % (args.rounds, args.rounds), "|---|---|---|---|---|---|"]
    every = True
    for p, bs in cases:
        e, g = res[((p, bs), False)], res[((p, bs), True)]
        won = all(b < a for a, b in zip(e, g)) and max(g) < min(e)
        every = every and won
        lines.append("| %d | %s | %s | %s | %.2f | %s |" % (bs, p, fmt(e), fmt(g), min(g) / min(e), "yes" if won else "NO"))
    lines += ["", "Graph replays are faster than the eager loop in every round of every case: **%s**." % ("yes" if every else "no")]
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
