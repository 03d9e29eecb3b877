"""GPU: Animator (impersonator_amd/models/animator.py) -- appearance transfer driven by a motion sequence -- and its one-launch
per-frame geometry, lwg_animate_inputs (csrc/animate.hip).

The reference's own models/animator.py cannot run against its utils/nmr.py, so there is no golden file: the kernel's specification is
bit-identity with the chain of existing entries it replaces, and the model's oracle is composed here from oracle.torch_ref pieces that
tests/test_oracle_vs_reference.py pins to the live reference (swapper_personalize, render_fim_wim, encode_fim, cal_bc_transform,
grid_sample, generator_swap), restarted from the product's posed cameras and vertices.

Inputs throughout: subject A = the rest pose, subject B = frame 200 of the synthetic motion (helpers.task_scene()); the driven poses
are frames 64, 400 and 900 under synthetic.cams(3, seed=5); a fourth frame repeats the first under the camera [1, 5, 0], which puts
the whole body off screen (all background)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from impersonator_amd import _lib, demo
from impersonator_amd.models.animator import Animator, left_face_flags, side_table
from impersonator_amd.utils import synthetic
from tests import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVEN = (64, 400, 900)


@functools.lru_cache(maxsize=None)
def _scene():
    """Shared, read-only: the two subjects and the four driven frames (numpy)."""
    sc = helpers.task_scene()
    verts = np.stack([synthetic.motion_verts(sc["rest"], t) for t in DRIVEN])
    cams = synthetic.cams(3, seed=5)
    sc["drv_verts"] = np.concatenate([verts, verts[:1]])
    sc["drv_cams"] = np.concatenate([cams, np.array([[1.0, 5.0, 0.0]], np.float32)])
    sc["par14"] = synthetic.part_map_fn(sc["rest"], sc["faces"], num_parts=13)[0]      # a 14-column one-hot table as condition map
    return sc


def _ids(target_part):
    selected = Animator.PART_IDS[target_part]
    return selected, [i for i in Animator.PART_IDS['all'] if i not in selected]


def _shares(part, selected, left, frames):
    """Per frame: (covered pixels, the reference's share of them, the source's share) from a part map (n, 11, H, W)."""
    out = []
    for k in frames:
        ref = float((part[k, selected].sum(0) != 0).sum())
        src = float((part[k, left].sum(0) != 0).sum()) if left else 0.0
        out.append((ref + src, ref / max(ref + src, 1.0), src / max(ref + src, 1.0)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the chain of existing entries, through the C entry, no generator
@functools.lru_cache(maxsize=None)
def _kernel_case(size, align):
    """Device inputs at one image size: renderer, the two subjects' p2verts and images, the four driven frames' fim / wim."""
    from impersonator_amd.utils.nmr import SMPLRenderer
    sc = _scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = SMPLRenderer(image_size=size, faces=sc["faces"], map_fn=sc["map_fn"], align_corners=bool(align)).cuda()
    case = dict(render=r, part_fn=t(sc["part_fn"]), par14=t(sc["par14"]))
    for n, seed in (("a", 11), ("b", 77)):
        f2v, _, _ = r.render_fim_wim(t(sc["cam_" + n]), t(sc["verts_" + n]))
        case["p2v_" + n] = r.source_p2verts(f2v)
        case["img_" + n] = t(synthetic.smooth_image(seed, (1, 3, size, size)))
    _, case["fim"], case["wim"] = r.render_fim_wim(t(sc["drv_cams"]), t(sc["drv_verts"]))
    return case


def _masked(p2v, drop):
    out = torch.empty_like(p2v)
    flags = torch.from_numpy(np.ascontiguousarray(drop, np.uint8)).cuda()
    _lib.check(_lib.load().lwg_mask_faces(_lib.ptr(p2v), _lib.ptr(flags), p2v.shape[1], 6, _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out


GUARD, SENTINEL = 64, -77.25


def _guarded(*shape):
    """An output tensor with GUARD sentinel floats on either side (a store outside the tensor shows)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n].view(*shape)


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("nc", [3, 14])
@pytest.mark.parametrize("target_part", ["upper_body", "all", "torso"])
@pytest.mark.parametrize("size", [32, 100])
def test_kernel_equals_the_chain_bit_for_bit(size, target_part, nc, align):
    """lwg_animate_inputs against lwg_mask_faces / lwg_encode_fim / lwg_cal_bc_transform / lwg_clamp / lwg_grid_sample plus the
    mask-and-compose expression in torch: torch.equal on T_src, T_ref, cond, tsf_img and both input layouts.  100 x 100 x 4 pixels
    is no multiple of the 256-lane workgroup; 'all' leaves the source's side empty; nc 14 has no NHWC8 form."""
    sc, case = _scene(), _kernel_case(size, align)
    lib, r = _lib.load(), case["render"]
    nf, bs = r.nf, 4
    selected, left = _ids(target_part)
    keep = left_face_flags(sc["part_faces"], left, nf)
    ref_f2p, src_f2p = _masked(case["p2v_b"], keep), _masked(case["p2v_a"], 1 - keep)
    side = torch.from_numpy(side_table(sc["part_fn"], selected, left)).cuda()
    table = r.map_fn if nc == 3 else case["par14"]
    assert table.shape == (nf + 1, nc)
    fim, wim = case["fim"], case["wim"]

    # the chain
    cond = r._lookup(fim, table, True)
    part = r._lookup(fim, case["part_fn"], True)
    part_mask = (torch.sum(part[:, selected], dim=1, keepdim=True) != 0).float()
    left_mask = (torch.sum(part[:, left], dim=1, keepdim=True) != 0).float() if left else torch.zeros_like(part_mask)
    flows = []
    for f2p in (ref_f2p, src_f2p):
        T = r.cal_bc_transform(f2p, fim, wim)
        _lib.check(lib.lwg_clamp(_lib.ptr(T), T.numel(), -2.0, 2.0, _lib.stream_ptr()))
        flows.append(T)
    T_ref, T_src = flows
    tsf_img = r.grid_sample(case["img_b"], T_ref) * part_mask + r.grid_sample(case["img_a"], T_src) * left_mask
    x = torch.cat([tsf_img, cond], dim=1)

    if target_part == "upper_body":
        for covered, ref_share, src_share in _shares(part, selected, left, range(3)):
            print("size %d: %d covered pixels, reference %.1f %%, source %.1f %%" % (size, covered, 100 * ref_share, 100 * src_share))
            assert covered > 0 and ref_share >= 0.30 and src_share >= 0.30      # a test on an empty side proves nothing
    assert bool((fim[:3] >= 0).any()) and bool((fim[3] == -1).all())

    # the kernel, every output at once
    bufs = dict(T_src=_guarded(bs, size, size, 2), T_ref=_guarded(bs, size, size, 2), cond=_guarded(bs, nc, size, size),
                tsf_img=_guarded(bs, 3, size, size), x=_guarded(bs, 3 + nc, size, size))
    if nc == 3:
        bufs["x8"] = _guarded(bs, size, size, 8)
    o = {k: v[1] for k, v in bufs.items()}
    _lib.check(lib.lwg_animate_inputs(
        _lib.ptr(fim), _lib.ptr(wim), bs, nf, size, _lib.ptr(table), nc, _lib.ptr(side), _lib.ptr(src_f2p), _lib.ptr(ref_f2p),
        _lib.ptr(case["img_a"]), _lib.ptr(case["img_b"]), align, _lib.ptr(o["T_src"]), _lib.ptr(o["T_ref"]), _lib.ptr(o["cond"]),
        _lib.ptr(o["tsf_img"]), _lib.ptr(o["x"]), _lib.ptr(o.get("x8")), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(o["T_src"], T_src) and torch.equal(o["T_ref"], T_ref)
    assert torch.equal(o["cond"], cond) and torch.equal(o["tsf_img"], tsf_img) and torch.equal(o["x"], x)
    if nc == 3:
        assert torch.equal(o["x8"][..., :6].permute(0, 3, 1, 2), x) and not bool(o["x8"][..., 6:].any())
    for name, (buf, _) in bufs.items():
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), name
    # the all-background frame: flows of exactly -2, nothing warped
    assert bool((o["T_src"][3] == -2).all()) and bool((o["T_ref"][3] == -2).all()) and not bool(o["tsf_img"][3].any())
    # only the flows requested: the other outputs may be NULL
    t_src, t_ref = torch.empty_like(T_src), torch.empty_like(T_ref)
    _lib.check(lib.lwg_animate_inputs(
        _lib.ptr(fim), _lib.ptr(wim), bs, nf, size, _lib.ptr(table), nc, _lib.ptr(side), _lib.ptr(src_f2p), _lib.ptr(ref_f2p),
        _lib.ptr(case["img_a"]), _lib.ptr(case["img_b"]), align, _lib.ptr(t_src), _lib.ptr(t_ref), None, None, None, None,
        _lib.stream_ptr()))
    assert torch.equal(t_src, T_src) and torch.equal(t_ref, T_ref)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the model against the CPU oracle
def _fixed_hmr(sc, *pairs):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return helpers.FixedHMR([(t(c), t(v)) for c, v in pairs])


@functools.lru_cache(maxsize=None)
def _oracle(size, target_part):
    """The three on-screen frames through oracle.torch_ref (CPU), computed once: the oracle depends on the posed cameras and
    vertices only, and those are fixed inputs here (helpers.FixedHMR hands them to the product unchanged)."""
    from oracle import torch_ref
    sc = _scene()
    # the weights demo.build_synthetic_imitator(seed=0, affine="random") loads (same seeded generator, same shapes)
    sd = torch_ref.state_dict_from_numpy(helpers.generator_state_dict(seed=0, affine="random"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    faces_t, map_fn, part_fn = t(sc["faces"].astype(np.int32)), t(sc["map_fn"]), t(sc["part_fn"])
    img_a, img_b = t(synthetic.smooth_image(11, (1, 3, size, size))), t(synthetic.smooth_image(77, (1, 3, size, size)))
    bg = t(synthetic.smooth_image(12, (1, 3, size, size)))
    selected, left = _ids(target_part)
    left_faces = sorted(set(f for i in left for f in sc["part_faces"][i]))
    other_faces = sorted(set(range(sc["faces"].shape[0])) - set(left_faces))
    with torch.no_grad():
        A = torch_ref.swapper_personalize(sd, img_a, t(sc["cam_a"]), t(sc["verts_a"]), faces_t, map_fn, part_fn, image_size=size)
        B = torch_ref.swapper_personalize(sd, img_b, t(sc["cam_b"]), t(sc["verts_b"]), faces_t, map_fn, part_fn, image_size=size)
        cam, verts = t(sc["drv_cams"][:3]), t(sc["drv_verts"][:3])
        _, fim, wim = torch_ref.render_fim_wim(cam, verts, faces_t, size)
        cond, part = torch_ref.encode_fim(fim, map_fn), torch_ref.encode_fim(fim, part_fn)
        part_mask = (torch.sum(part[:, selected], dim=1, keepdim=True) != 0).float()
        left_mask = (torch.sum(part[:, left], dim=1, keepdim=True) != 0).float()
        ref_f2p, src_f2p = B["p2verts"].clone(), A["p2verts"].clone()
        ref_f2p[0, left_faces] = -2
        src_f2p[0, other_faces] = -2
        T_ref = torch_ref.cal_bc_transform(ref_f2p, fim, wim).clamp(-2, 2)
        T_src = torch_ref.cal_bc_transform(src_f2p, fim, wim).clamp(-2, 2)
        n = fim.shape[0]
        tsf_img = torch_ref.grid_sample(img_b.expand(n, -1, -1, -1), T_ref) * part_mask \
            + torch_ref.grid_sample(img_a.expand(n, -1, -1, -1), T_src) * left_mask
        x = torch.cat([tsf_img, cond], dim=1)
        color, mask = torch_ref.generator_swap(sd, x, B["enc"], A["enc"], B["res"], A["res"], T_ref, T_src)
        preds = mask * bg + (1 - mask) * color
    return dict(fim=fim, part=part, T_ref=T_ref, T_src=T_src, tsf_inputs=x, preds=preds, bg=bg, img_a=img_a, img_b=img_b,
                shares=_shares(part, selected, left, range(3)))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_animator_matches_the_oracle(precision):
    """Animator.animate_setup + transfer (three driven frames in one call, upper_body, 128 x 128) against the oracle composed from
    torch_ref pieces.  Bounds as test_swapper_matches_the_reference_golden: flows 1e-6, tsf_inputs 1e-5, preds 1e-3 (the project's
    image budget); fim identical on all three frames.
    Observed on the MI355X (printed below, copied into profiles/animate.md): flows 0, tsf_inputs 1.2e-7, preds 1.1e-5 (fp32) /
    4.8e-5 (bf16x3)."""
    size, sc = 128, _scene()
    ref = _oracle(size, "upper_body")
    for covered, ref_share, src_share in ref["shares"]:
        assert covered > 0 and ref_share >= 0.30 and src_share >= 0.30, ref["shares"]
    an, _, _, _ = demo.build_synthetic_imitator(batch_size=3, seed=0, affine="random", image_size=size, model="animator")
    an.generator.precision = precision
    an.hmr = _fixed_hmr(sc, (sc["cam_a"], sc["verts_a"]), (sc["cam_b"], sc["verts_b"]), (sc["drv_cams"][:3], sc["drv_verts"][:3]))
    smpl = np.zeros(85, np.float32)
    an.animate_setup(ref["img_a"][0].numpy(), ref["img_b"][0].numpy(), src_smpl=smpl, ref_smpl=smpl, src_bg=ref["bg"][0].numpy(),
                     ref_bg=ref["bg"][0].numpy())
    an.set_target_part("upper_body")
    seen = {}
    forward = an.forward
    an.forward = lambda x, *a, **k: (seen.setdefault("x", x.clone()), forward(x, *a, **k))[1]
    preds = an.transfer(np.zeros((3, 85), np.float32), cam_strategy="copy", t=0)
    info = an.tsf_info
    assert preds.shape == (3, 3, size, size) and seen["x"].shape == (3, 6, size, size)
    assert torch.equal(info["cam"].cpu(), torch.from_numpy(sc["drv_cams"][:3])) and torch.equal(info["verts"].cpu(),
                                                                                                 torch.from_numpy(sc["drv_verts"][:3]))
    for k in range(3):
        assert torch.equal(info["fim"][k].cpu(), ref["fim"][k]), k
    e_src, e_ref = helpers.maxdiff(info["T"], ref["T_src"])[0], helpers.maxdiff(info["T_ref"], ref["T_ref"])[0]
    e_x, e_p = helpers.maxdiff(seen["x"], ref["tsf_inputs"])[0], helpers.maxdiff(preds, ref["preds"])[0]
    print("animator vs oracle (%s): T_src %.3g  T_ref %.3g  tsf_inputs %.3g  preds %.3g; shares %s"
          % (precision, e_src, e_ref, e_x, e_p, ["%d px, ref %.0f %%" % (c, 100 * r) for c, r, _ in ref["shares"]]))
    assert e_src <= 1e-6 and e_ref <= 1e-6, (e_src, e_ref)
    assert e_x <= 1e-5, e_x
    assert e_p <= 1e-3, e_p
    an.generator.release()


# ---------------------------------------------------------------------------------------------------------------------
# 3. batches, lanes, the chain form and graph replay give the same bits
@functools.lru_cache(maxsize=None)
def _synthetic_pair(batch_size, size):
    """An Animator over the synthetic body model with two personalised subjects (as run_animate.py --synthetic builds it)."""
    an, smpl_a, img_a, bg_a = demo.build_synthetic_imitator(
        batch_size=batch_size, image_size=size, model="animator", opt=demo.default_opt(batch_size=batch_size, image_size=size))
    smpl_b = demo.synthetic_smpls(8, seed=3)[5]
    img_b = synthetic.smooth_image(77, (1, 3, size, size))[0]
    an.animate_setup(img_a, img_b, src_smpl=smpl_a, ref_smpl=smpl_b, src_bg=bg_a, ref_bg=bg_a)
    return an


def test_batches_chain_and_graph_give_the_same_bits():
    """11 frames at batch_size 4 (batches of 4, 4 and 3, two lanes, default fuse) through `animate` == the same frames one at a
    time through `transfer` at batch 1 -- the two-stream generator at bs > 1 over shared batch-1 source features; the same bits
    from Animator(fused=False); and frame_graph(batch=1) replays equal the eager frames."""
    size, n = 128, 11
    an = _synthetic_pair(4, size)
    smpls = demo.synthetic_smpls(n, seed=0)
    dev_smpls = torch.from_numpy(smpls).cuda()
    an.fused = True
    batched = np.stack(an.animate(None, tgt_smpls=smpls, cam_strategy="smooth", target_part="upper_body"))
    assert batched.shape == (n, size, size, 3) and an.tsf_info["T_ref"].shape[0] == 3       # the ragged tail came last
    singles = []
    for i in range(n):
        singles.append(an.transfer(dev_smpls[i:i + 1], "smooth", t=i).clone())
        assert an.tsf_info["T"].shape == an.tsf_info["T_ref"].shape == (1, size, size, 2)
    eager = torch.cat(singles).permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(batched, eager)
    assert batched.std() > 0.05 and np.abs(batched[0] - batched[5]).max() > 0.05              # frames that move
    an.fused = False
    chain = np.stack(an.animate(None, tgt_smpls=smpls, cam_strategy="smooth", target_part="upper_body"))
    assert np.array_equal(chain, batched)
    an.fused = True
    an.first_cam = dev_smpls[0:1, 0:3].clone()
    run = an.frame_graph(batch=1)
    for i in range(n):
        out = run(dev_smpls[i], t=i)
        torch.cuda.synchronize()
        assert torch.equal(out, singles[i]), i


# ---------------------------------------------------------------------------------------------------------------------
# 4. no framework kernel per frame
def test_transfer_launches_no_framework_kernel():
    """One transfer_params_by_smpl + forward after setup under the torch profiler (the check of
    test_swap_launches_no_framework_kernel_and_replays_as_one_graph): every device record is liblwg's."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    an = _synthetic_pair(4, 128)
    an.fused = True
    an.set_target_part("upper_body")
    smpls = torch.from_numpy(demo.synthetic_smpls(8, seed=0)).cuda()
    an.first_cam = smpls[0:1, 0:3].clone()
    eager = an.forward(an.transfer_params_by_smpl(smpls[2:4], "smooth", t=2), an.tsf_info["T"]).clone()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        again = an.forward(an.transfer_params_by_smpl(smpls[2:4], "smooth", t=2), an.tsf_info["T"])
        torch.cuda.synchronize()
    assert torch.equal(again, eager)
    records = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    foreign = sorted({k for k in records if "lwg" not in k})
    print("animate frame: %d device records, others: %s" % (len(records), foreign))
    assert len(records) >= 40 and not foreign, foreign
    assert sum("animate_inputs_kernel" in k for k in records) == 1


def test_front_warp_uses_the_composite_and_the_frames_fim():
    """--front_warp: Imitator.warp_front's expression with the COMPOSITE tsf_img and the driven frame's fim, on top of the
    two-stream generator's blended image; through `animate` (one batch per generator call under front_warp) the same bits."""
    size = 128
    an, smpl_a, img_a, bg_a = demo.build_synthetic_imitator(
        batch_size=2, image_size=size, model="animator", opt=demo.default_opt(batch_size=2, image_size=size, front_warp=True))
    img_b = synthetic.smooth_image(77, (1, 3, size, size))[0]
    an.animate_setup(img_a, img_b, src_smpl=smpl_a, ref_smpl=demo.synthetic_smpls(8, seed=3)[5], src_bg=bg_a, ref_bg=bg_a)
    an.set_target_part("upper_body")
    smpls = demo.synthetic_smpls(5, seed=0)
    dev = torch.from_numpy(smpls).cuda()
    batched = np.stack(an.animate(None, tgt_smpls=smpls, target_part="upper_body"))
    for s in (0, 2, 4):
        x = an.transfer_params_by_smpl(dev[s:s + 2], "smooth", t=s)
        info = an.tsf_info
        preds = an.forward(x, info["T"])
        assert an.tsf_info is info
        (ref_enc, ref_res), (src_enc, src_res) = an.ref_info["feats"], an.src_info["feats"]
        plain, _, mask = an.generator.swap(x, ref_enc, src_enc, ref_res, src_res, info["T_ref"], info["T"], bg_img=an.src_info["bg"])
        front = an.render.encode_front_fim(info["fim"], transpose=True, front_fn=True)
        assert bool(front.any()) and bool((front * info["tsf_img"].abs()).any())         # the warp has something to paste
        want = (1 - front) * plain + info["tsf_img"] * front * (1 - mask)
        assert torch.equal(preds, want) and not torch.equal(preds, plain)
        assert np.array_equal(batched[s:s + 2], preds.permute(0, 2, 3, 1).cpu().numpy())
    an.generator.release()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the command line
def _u8(x):
    """utils/cv_utils.py:31-33: (x + 1) / 2 * 255 then astype(uint8) -- truncation, not rounding."""
    return ((np.asarray(x) + 1) / 2.0 * 255).astype(np.uint8)


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_run_animate_writes_the_frames(tmp_path):
    """`run_animate.py --synthetic --num_frames 5 --batch_size 2 --swap_part upper_body --save_res` writes five JPEG files.  JPEG is
    lossy, so a decoded file is not the frame's uint8 form; it is compared with the decoded JPEG of the frame the same model computes
    in this process, written by the same encoder, under the bound tests/test_gpu_cli.py holds run_imitator.py's files to (at most one
    grey level, on fewer than a quarter of the values)."""
    from impersonator_amd.utils import cv_utils
    out_dir = str(tmp_path / "animate")
    cmd = [sys.executable, "run_animate.py", "--synthetic", "--num_frames", "5", "--batch_size", "2", "--swap_part", "upper_body",
           "--save_res", "--output_dir", out_dir]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=900, text=True)
    assert p.returncode == 0, "%s failed (%d)\n%s\n%s" % (cmd, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    folder = os.path.join(out_dir, "animators")
    files = sorted(os.listdir(folder))
    assert files == ["pred_%.8d.jpg" % t for t in range(5)] and "Saving 5 frames" in p.stdout

    an = _synthetic_pair(2, 256)
    an.fused = True
    mine = an.animate(None, tgt_smpls=demo.synthetic_smpls(5, seed=0), cam_strategy="smooth", target_part="upper_body")
    assert len(mine) == 5
    for t, name in enumerate(files):
        disk = _read(os.path.join(folder, name))
        assert disk.shape == (256, 256, 3) and disk.dtype == np.uint8
        again = str(tmp_path / ("mine_%d.jpg" % t))
        cv_utils.save_cv2_img(mine[t], again, normalize=True)
        d = np.abs(disk.astype(np.int16) - _read(again).astype(np.int16))
        lossy = np.abs(disk.astype(np.int16) - _u8(mine[t]).astype(np.int16))
        print("frame %d: decoded file vs decoded API frame max %d; vs the frame's uint8 form (JPEG loss) max %d" % (t, d.max(), lossy.max()))
        assert d.max() <= 1 and (d > 0).mean() < 0.25
    assert _read(os.path.join(folder, files[4])).std() > 10
