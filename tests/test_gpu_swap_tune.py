"""GPU parity of the Swapper's fine-tune (impersonator_amd/models/post_tune.py: SwapTuner, swap_samples; the reference's
Swapper.post_personalize, models/swapper.py:273-476): Adam with step count and learning rate on the device, images, loss terms
and the hand-written gradient against CPU autograd (tests/swap_tune_ref.py), the captured iteration against the eager one bit
for bit, then the task-model surface (Swapper.post_personalize, run_swap.py --post_tune).

Method and allowances are those of tests/test_gpu_post_tune.py: every allowance on a gradient or on the cycle image is a
multiple of the CPU float32 oracle's OWN distance from the float64 oracle on the same batch, computed here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref
from tests import helpers
from tests import post_tune_ref as ref
from tests import swap_tune_ref as sref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = 40          # faces of the stand-in face maps
MARGIN = 4.0     # x the CPU float32 oracle's own distance from float64 (tests/test_gpu_post_tune.py)
TOTAL, FIX = 4, 1    # the oracle's loop: rates 2e-4 x 3, 1e-5


# ------------------------------------------------------------------------------------------------ 1. scheduled Adam
@pytest.mark.parametrize("n", [10007, 1])
def test_scheduled_adam_equals_device_step_adam_bit_for_bit(n):
    """lwg_adam_update_scheduled == lwg_adam_update_device_step called with lr_table[min(t, count) - 1]: six steps over a
    4-entry table, so steps 5 and 6 clamp to the last entry."""
    from impersonator_amd import ops
    g = torch.Generator().manual_seed(n)
    table = torch.tensor([2e-4, 1.3e-4, 7e-5, 1e-5], dtype=torch.float32)
    betas = (0.5, 0.999)
    p0 = torch.randn(n, generator=g)
    a = [p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()]
    b = [p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()]
    sa, sb = ops.adam_step_state(0, betas), ops.adam_step_state(0, betas)
    table_dev = table.cuda()
    for t in range(1, 7):
        grad = (torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g))).cuda()
        ops.adam_update_scheduled(a[0], grad, a[1], a[2], sa, table_dev, betas, 1e-8)
        ops.adam_update_device_step(b[0], grad, b[1], b[2], sb, float(table[min(t, 4) - 1]), betas, 1e-8)
        for x, y, name in zip(a, b, ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(x, y), (t, name)
    assert int(sa[0]) == 6 and torch.equal(sa, sb)
    assert not torch.equal(a[0].cpu(), p0)


# ------------------------------------------------------------------------------------------------ 2. images, terms, gradient
def _dbl(d):
    return {k: v.double() for k, v in d.items()}


def _dist(a, b, scale=None):
    """relative L2 distance over the tensors of `b` that carry a gradient; `scale`: the tensors the norm is taken of"""
    num = den = 0.0
    for k, v in b.items():
        if v is None:
            continue
        e = a[k].double() - v.double()
        num += float((e * e).sum())
        den += float(((scale or b)[k].double() ** 2).sum())
    return (num / den) ** 0.5


def _generator():
    from impersonator_amd.networks.generator import ImpersonatorGenerator
    return ImpersonatorGenerator(bg_dim=4, src_dim=6, tsf_dim=6, repeat_num=6, image_size=128, max_batch=2)


def _fronts(render, sample):
    return render.encode_front_fim(sample["tsf_fim"]), render.encode_front_fim(sample["src_fim"])


def _oracle(gsd, sample, bg, render, front_warp, n_steps):
    """float32 and float64 CPU runs of `n_steps` iterations of the (TOTAL, FIX) loop on the batch, the images of the first, and
    the float64 gradient with the cycle path cut"""
    front = _fronts(render, sample) if front_warp else None
    out = {}
    for name, cast in (("32", lambda x: x), ("64", lambda x: x.double())):
        sd, s = {k: cast(v) for k, v in gsd.items()}, {k: cast(v) for k, v in sample.items()}
        fr = None if front is None else tuple(cast(f) for f in front)
        with torch.no_grad():
            out["img" + name] = sref.step_loss(sd, s, cast(bg), fr)[2]
        out["hist" + name], out["grad" + name], out["final" + name] = sref.steps(sd, s, cast(bg), TOTAL, FIX, fr, n_steps=n_steps)
    out["cut64"] = sref.steps(_dbl(gsd), _dbl(sample), bg.double(), TOTAL, FIX, None if front is None else tuple(f.double() for f in front),
                              n_steps=1, cut_cycle=True)[1]
    out["d32"] = _dist(out["grad32"], out["grad64"])
    return out


@pytest.fixture(scope="module")
def setup():
    gsd = torch_ref.state_dict_from_numpy(helpers.generator_state_dict(seed=2, affine="random"))
    G = _generator()
    G.load_state_dict(gsd)
    sample = ref.sample_batch(seed=5, n=2, size=64, nf=NF)
    bg = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1     # a background per sample
    render = ref.TableRender(NF, seed=3)
    return dict(gsd=gsd, G=G, sample=sample, bg=bg, render=render, plain=_oracle(gsd, sample, bg, render, False, TOTAL))


@pytest.fixture(scope="module")
def setup_front(setup):
    return _oracle(setup["gsd"], setup["sample"], setup["bg"], setup["render"], True, 1)


def _tuner(setup, total=TOTAL, fix=FIX, **kw):
    from impersonator_amd.models.post_tune import SwapTuner
    return SwapTuner(setup["G"], setup["bg"], setup["render"], total=total, fix=fix, **kw)


NAMES = ("fake_src", "fake_tsf", "cyc_tsf", "src_mask", "tsf_mask")


def _check_images_and_terms(tuner, sample, o, precision):
    out = dict(zip(NAMES, (t.cpu() for t in tuner.forward(sample))))
    first_pass = 1e-4 if precision == "fp32" else 2e-4                       # the project's bounds on a generator pass
    for k in ("fake_src", "fake_tsf", "src_mask", "tsf_mask"):
        err = float((out[k] - o["img32"][k]).abs().max())
        print("%s %s vs the float32 oracle: %.3g" % (precision, k, err))
        assert err < first_pass, k
    for k in ("fake_tsf", "cyc_tsf"):
        own = float((o["img32"][k].double() - o["img64"][k]).abs().max())   # the float32 oracle's own distance from float64
        err = float((out[k].double() - o["img64"][k]).abs().max())
        print("%s %s vs float64: %.3g (float32 oracle: %.3g)" % (precision, k, err, own))
        assert err <= MARGIN * own * (1 if precision == "fp32" else 2), k
    terms = tuner.backward()
    assert "fid" not in terms                                               # no face network: the readout is left out
    for k, v in o["hist64"][0].items():
        print("%s term %s: %.7g (float64 %.7g)" % (precision, k, float(terms[k]), v))
        assert abs(float(terms[k]) - v) < 1e-4 * max(1.0, abs(v)), k
    return terms


def test_images_terms_and_gradient(setup):
    o = setup["plain"]
    # on the oracle alone first: the gradient with the cycle inputs detached can be told apart from the full one at this allowance
    cut = _dist(o["cut64"], o["grad64"])
    print("float32 oracle vs float64: %.3g; float64 gradient with the cycle inputs detached: %.3g from the full one" % (o["d32"], cut))
    assert cut > 3 * MARGIN * o["d32"]
    tuner = _tuner(setup)
    _check_images_and_terms(tuner, setup["sample"], o, "fp32")
    grads = tuner.gradients()
    with_grad = sorted(k for k, v in o["grad64"].items() if v is not None)
    assert len(with_grad) == 136 and all(k.startswith(("src_model.", "tsf_model.")) for k in with_grad)
    assert sorted(grads) == with_grad
    dev = _dist(grads, o["grad64"])
    dev_cut = _dist(grads, o["cut64"], scale=o["grad64"])
    print("whole-gradient relative L2 vs float64: device fp32 %.3g, CPU float32 oracle %.3g; device vs the cut gradient %.3g" % (
        dev, o["d32"], dev_cut))
    assert dev <= MARGIN * o["d32"]
    assert dev_cut >= cut - MARGIN * o["d32"]                               # the cycle path is live
    assert float(tuner.flat_g[:tuner._lo].abs().max()) == 0.0


def test_bf16x3(setup):
    """conv_precision='bf16x3': within 3 x the exact-fp32 device tuner's own distance from float64 (the project's convention)."""
    o = setup["plain"]
    t32, t16 = _tuner(setup), _tuner(setup, conv_precision="bf16x3")
    _check_images_and_terms(t16, setup["sample"], o, "bf16x3")
    t32.forward(setup["sample"])
    t32.backward()
    d16, d32 = _dist(t16.gradients(), o["grad64"]), _dist(t32.gradients(), o["grad64"])
    print("whole-gradient relative L2 vs float64: bf16x3 %.3g, fp32 device %.3g" % (d16, d32))
    assert d16 <= 3.0 * d32


def test_front_warp(setup, setup_front):
    o = setup_front
    cut = _dist(o["cut64"], o["grad64"])
    assert cut > 3 * MARGIN * o["d32"]
    tuner = _tuner(setup, front_warp=True)
    _check_images_and_terms(tuner, setup["sample"], o, "fp32")
    dev = _dist(tuner.gradients(), o["grad64"])
    print("front_warp whole-gradient relative L2 vs float64: device %.3g, CPU float32 oracle %.3g" % (dev, o["d32"]))
    assert dev <= MARGIN * o["d32"]
    assert _dist(tuner.gradients(), o["cut64"], scale=o["grad64"]) >= cut - MARGIN * o["d32"]


# ------------------------------------------------------------------------------------------------ 3. four steps, decaying rate
def test_four_steps_with_a_decaying_rate(setup):
    o = setup["plain"]
    tuner = _tuner(setup)
    assert tuner.lr_table.tolist() == pytest.approx([2e-4, 2e-4, 2e-4, 1e-5], rel=1e-6)
    tuner.load(setup["sample"])
    before = tuner.flat_p.clone()
    moved = []
    for i in range(TOTAL):
        prev = tuner.flat_p.clone()
        tuner.optimize()
        moved.append(float((tuner.flat_p - prev).abs().max()))
    hist = tuner.terms_history()                                             # the one read-back
    for i in range(TOTAL):
        total, v64, v32 = hist[i]["total"], o["hist64"][i]["total"], o["hist32"][i]["total"]
        allow = max(1e-4 * abs(v64), MARGIN * abs(v32 - v64))
        print("step %d total: device %.6f, float64 %.6f, float32 oracle %.6f (allowance %.2e)" % (i, total, v64, v32, allow))
        assert abs(total - v64) <= allow, i
    assert o["hist64"][3]["total"] < o["hist64"][0]["total"] and hist[3]["total"] < hist[0]["total"]     # it is a descent
    assert torch.equal(tuner.flat_p[:tuner._lo], before[:tuner._lo])         # bg_model.*: bit-unchanged
    assert not torch.equal(tuner.flat_p[tuner._lo:], before[tuner._lo:])
    # the last step ran at 1e-5, a twentieth of the rate before: Adam's largest move scales with the rate
    print("largest parameter move per step: %s" % ", ".join("%.3g" % m for m in moved))
    assert moved[3] < 0.25 * moved[2]
    assert int(tuner.step_state[0]) == TOTAL


# ------------------------------------------------------------------------------------------------ 4. graph = eager
@pytest.mark.parametrize("precision,batch_size", [("fp32", 2), ("bf16x3", 2), ("fp32", 1)])
def test_graph_replays_equal_eager_iterations_bit_for_bit(setup, precision, batch_size):
    """Two tuners from one seed, one stepped by optimize(), one by optimize_graphed() in strict mode: identical buffers and
    history rows after every step, one capture across the three rate changes.

    [fp32-2] is also the regression test of the re-laid-out weight matrix's row padding (csrc/train.hip, relayout): zeroed by a
    runtime memset it kept stale workspace bits in a replay, and the first stem's output was NaN at step 5."""
    total, fix = 6, 2                                                        # rates 2e-4 x 4, 1.05e-4, 1e-5: three changes in a row
    sample = {k: v.cuda() for k, v in setup["sample"].items()}
    kept = {k: v.clone() for k, v in sample.items()}
    eager = _tuner(setup, total, fix, conv_precision=precision, batch_size=batch_size)
    graphed = _tuner(setup, total, fix, conv_precision=precision, batch_size=batch_size)
    assert eager.bs == graphed.bs == batch_size
    eager.load(sample)
    graphed.load(sample)
    assert len(graphed.rows) == (1 if batch_size == 2 else 2)
    if batch_size == 1:     # swapper.py:421: sample i's masks are rows i and 2 + i of cat([source masks, transfer masks])
        flat = torch.cat([sample["pseudo_masks"][:, 0], sample["pseudo_masks"][:, 1]], dim=0)
        for i in (0, 1):
            assert torch.equal(graphed.rows[i]["pseudo"], flat[i:4:2].permute(0, 2, 3, 1))
            assert torch.equal(graphed.rows[i]["bg"], setup["bg"][i:i + 1].permute(0, 2, 3, 1).cuda())
    for step in range(total):
        eager.optimize()
        graphed.optimize_graphed(warmup=2, strict=True)
        assert (graphed._graph is not None) == (step >= 2), step
        for name in ("flat_p", "flat_g", "flat_m", "flat_v"):
            assert torch.equal(getattr(eager, name), getattr(graphed, name)), (step, name)
        assert torch.equal(eager.history, graphed.history), step
        assert bool((eager.history[:step + 1, 3] > 0).all()) and not bool(eager.history[step + 1:].any())
        assert torch.equal(eager.step_state, graphed.step_state) and int(graphed.step_state[0]) == step + 1
    assert graphed.captures == 1 and graphed.replays == total - 2           # never re-captured across the three rate changes
    for k, v in kept.items():
        assert torch.equal(sample[k], v), k                                  # the caller's tensors are untouched
    for t in (eager, graphed):
        with pytest.raises(RuntimeError, match="learning-rate table"):
            (t.optimize if t is eager else t.optimize_graphed)()
    assert int(graphed.step_state[0]) == total


# ------------------------------------------------------------------------------------------------ 5. fid
def test_fid_is_a_readout(setup):
    from impersonator_amd.networks.facenet import SphereFaceLoss
    fsd = helpers.sphere20a_state_dict(seed=4)
    plain, faced = _tuner(setup), _tuner(setup, face=SphereFaceLoss(fsd))
    for t in (plain, faced):
        t.forward(setup["sample"])
    a, b = plain.backward(), faced.backward()
    assert torch.equal(plain.flat_g, faced.flat_g)
    with torch.no_grad():
        want = sref.step_loss(setup["gsd"], setup["sample"], setup["bg"], fsd=fsd)[1]
    print("fid: device %.6f, float32 oracle %.6f" % (float(b["fid"]), float(want["fid"])))
    for k in ("fid", "total"):
        assert abs(float(b[k]) - float(want[k])) < 1e-4 * max(1.0, abs(float(want[k]))), k
    assert abs(float(b["total"]) - float(a["total"]) - float(b["fid"])) < 1e-5 * float(b["total"])
    hist = faced.run(graphed=True)                                           # asked for replays -- but not with a face readout
    assert len(hist) == TOTAL and all("fid" in h for h in hist)
    assert faced._graph is None and faced.replays == 0 and faced.captures == 0


# ------------------------------------------------------------------------------------------------ 6. the task model
SIZE = 128     # the smallest image the generator's device handle takes


def _swapper(**over):
    from impersonator_amd import demo
    from impersonator_amd.utils import synthetic
    opt = demo.default_opt(batch_size=2, image_size=SIZE, post_tune=True, **over)
    sw, smpl_a, img_a, bg_a = demo.build_synthetic_imitator(batch_size=1, image_size=SIZE, model="swapper", opt=opt)
    smpl_b = demo.synthetic_smpls(8, seed=3)[5]
    img_b = synthetic.smooth_image(77, (1, 3, SIZE, SIZE))[0]
    bg_b = synthetic.smooth_image(78, (1, 3, SIZE, SIZE))[0]
    return sw, (img_a, img_b, smpl_a, smpl_b, bg_a, bg_b)


def test_post_personalize_needs_swap_setup():
    sw, _ = _swapper()
    with pytest.raises(RuntimeError, match="swap_setup"):
        sw.post_personalize('', None, verbose=False)


@pytest.fixture(scope="module")
def tuned():
    from impersonator_amd.models.post_tune import swap_samples
    sw, (img_a, img_b, smpl_a, smpl_b, bg_a, bg_b) = _swapper()
    sw.swap_setup(img_a, img_b, src_smpl=smpl_a, tgt_smpl=smpl_b, src_bg=bg_a, tgt_bg=bg_b)
    before = {k: v.detach().cpu().clone() for k, v in sw.generator.state_dict().items()}
    run = sw.swap_graph(sw.src_info, sw.tsf_info)
    untuned = run().clone()
    assert torch.equal(untuned, sw.swap(sw.src_info, sw.tsf_info))
    samples = {k: v.cpu().clone() for k, v in swap_samples(sw).items()}
    old_tsf_feat = sw.tsf_info["feats"][0][-1].clone()
    history = sw.post_personalize('', None, verbose=False)                   # on the code before: NotImplementedError
    return dict(sw=sw, before=before, run=run, untuned=untuned, samples=samples, history=history, old_tsf_feat=old_tsf_feat)


def test_post_personalize_returns_the_terms_of_fifty_steps(tuned):
    hist = tuned["history"]
    assert len(hist) == 50 and all(set(h) == {"cycle", "struct", "mask", "total"} for h in hist)
    assert all(np.isfinite(h["total"]) and h["total"] > 0 for h in hist)
    assert hist[-1]["total"] < hist[0]["total"]


def test_swap_samples_equal_the_reference_set_inputs(tuned):
    sw, got, sd = tuned["sw"], tuned["samples"], tuned["before"]

    def cpu_info(info):
        out = {k: info[k].cpu() for k in ("fim", "wim", "cond", "img", "bg", "src_inputs", "j2d")}
        out["p2verts"] = info["p2verts_c"].cpu().reshape(1, -1, 3, 2)
        out["feats"] = torch_ref.encode_src(sd, out["src_inputs"])
        return out

    with torch.no_grad():
        want = sref.set_inputs(sd, cpu_info(sw.src_info), cpu_info(sw.tsf_info), ft_ks=sw._opt.ft_ks)
    assert sorted(got) == sorted(want)
    for k in ("images", "j2d", "src_inputs", "src_fim", "tsf_fim", "bg", "pseudo_masks"):
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k].float()), k
    assert float((got["T"] - want["T"]).abs().max()) <= 1e-6                  # test_gpu_imitator_golden.py's bound on a flow
    assert torch.equal(got["T_cycle"], got["T"].flip(0))
    assert bool((got["T"] == -2).any()) and bool((got["T"] != -2).any())
    assert torch.equal(got["tsf_inputs"][:, 3:], want["tsf_inputs"][:, 3:])
    assert float((got["tsf_inputs"][:, :3] - want["tsf_inputs"][:, :3]).abs().max()) <= 2e-6   # the warped source: test_gpu_raster.py's bound
    assert float((got["preds"] - want["preds"]).abs().max()) <= 1e-3          # the final-image bound (smoke, test_gpu_cli.py)
    assert got["preds"].shape == (2, 3, SIZE, SIZE) and got["pseudo_masks"].shape == (2, 2, 1, SIZE, SIZE)


def test_tuned_weights_reach_both_subjects(tuned):
    sw = tuned["sw"]
    after = {k: v.detach().cpu() for k, v in sw.generator.state_dict().items()}
    for k, v in tuned["before"].items():                                      # only the two streams moved
        if k.startswith("bg_model."):
            assert torch.equal(after[k], v), k
        elif v.dim() == 4:
            assert not torch.equal(after[k], v), k
    for info in (sw.src_info, sw.tsf_info):                                   # both feature sets are the tuned weights'
        enc, res = sw.generator.encode_src(info["src_inputs"])
        for a, b in zip(list(info["feats"][0]) + list(info["feats"][1]), list(enc) + list(res)):
            assert torch.equal(a, b)
    assert not torch.equal(tuned["old_tsf_feat"], sw.tsf_info["feats"][0][-1])   # ... not the ones swap_setup encoded
    preds = sw.swap(sw.src_info, sw.tsf_info)
    assert not torch.equal(preds, tuned["untuned"])
    with pytest.raises(RuntimeError, match="record a new one"):
        tuned["run"]()
    again = sw.swap_graph(sw.src_info, sw.tsf_info)                           # a graph recorded afterwards serves the tuned swap
    assert torch.equal(again(), preds)


# ------------------------------------------------------------------------------------------------ 7. CLI
def test_cli_post_tune(tmp_path):
    """run_swap.py --synthetic --save_res [--post_tune]: both exit 0 and write the swap, and the pictures differ."""
    from PIL import Image
    outs = {}
    for flag in ("", "--post_tune"):
        out = tmp_path / ("tuned" if flag else "plain")
        cmd = [sys.executable, os.path.join(ROOT, "run_swap.py"), "--synthetic", "--save_res", "--image_size", str(SIZE),
               "--output_dir", str(out)] + ([flag] if flag else [])
        proc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        assert proc.returncode == 0, proc.stdout[-2000:]
        files = sorted(f for f in os.listdir(out / "swappers") if f.endswith(".png"))
        assert len(files) == 1, files
        outs[flag] = np.asarray(Image.open(out / "swappers" / files[0]))
    assert outs[""].shape == outs["--post_tune"].shape and not np.array_equal(outs[""], outs["--post_tune"])
