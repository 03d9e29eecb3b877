"""GPU parity: InpaintSANet (background inpaintor, once per source) through the C ABI vs the CPU oracle."""
import numpy as np
import pytest
import torch

from impersonator_amd.utils import synthetic
from oracle import torch_ref
from tests import helpers

pytestmark = pytest.mark.gpu


def _net_and_sd(seed=0):
    from impersonator_amd.networks.inpaintor import InpaintSANet
    net = InpaintSANet(c_dim=4).eval()
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in synthetic.random_inpaintor_state_dict(shapes, seed).items()}
    net.load_state_dict(sd)
    return net.cuda(), sd


def test_inpaintor_matches_oracle():
    net, sd = _net_and_sd(0)
    img = torch.from_numpy(synthetic.smooth_image(5))
    yy, xx = np.mgrid[0:256, 0:256]
    mask = torch.from_numpy((((yy - 120) / 90.0) ** 2 + ((xx - 128) / 50.0) ** 2 < 1).astype(np.float32))[None, None]
    coarse, x, comp = net(img.cuda(), mask.cuda())
    with torch.no_grad():
        oc, ox, ocomp = torch_ref.inpaint_forward(sd, img, mask)
    for name, a, b in (("coarse", coarse, oc), ("x", x, ox), ("comp", comp, ocomp)):
        err = float((a.cpu() - b).abs().max())
        assert err <= 1e-3, (name, err)
    # the three return conventions of the reference (inpaintor.py:198-202)
    assert torch.equal(net(img.cuda(), mask.cuda(), only_x=True), x)
    assert torch.equal(net(img.cuda(), mask.cuda(), only_out=True), comp)
    assert float(x.abs().max()) <= 1.0


def test_inpaintor_precisions():
    """InpaintSANet.precision: 'bf16x3' (default: the gated convs with >= 32 input channels on the split-operand MFMA kernels)
    against 'fp32' (exact fp32 MFMA everywhere) and the CPU oracle.  fp32 sits at float rounding from the oracle; bf16x3 within a
    few 1e-5 of it through the 35 gated layers (bound of the network: 1e-3)."""
    net, sd = _net_and_sd(0)
    img = torch.from_numpy(synthetic.smooth_image(5))
    yy, xx = np.mgrid[0:256, 0:256]
    mask = torch.from_numpy((((yy - 120) / 90.0) ** 2 + ((xx - 128) / 50.0) ** 2 < 1).astype(np.float32))[None, None]
    with torch.no_grad():
        oracle = torch_ref.inpaint_forward(sd, img, mask)
    errs = {}
    outs = {}
    for prec in ("bf16x3", "fp32"):
        net.precision = prec
        outs[prec] = [t.clone() for t in net(img.cuda(), mask.cuda())]
        errs[prec] = [float((a.cpu() - b).abs().max()) for a, b in zip(outs[prec], oracle)]
    print("inpaintor vs oracle (coarse, x, comp): bf16x3 %s, fp32 %s" % (["%.2e" % e for e in errs["bf16x3"]], ["%.2e" % e for e in errs["fp32"]]))
    assert not torch.equal(outs["bf16x3"][1], outs["fp32"][1]), "the bf16x3 route did not run"
    assert max(errs["fp32"]) <= 2e-5 and max(errs["bf16x3"]) <= 3e-4, errs


def test_imitator_personalize_with_inpaintor():
    """models/imitator.py:116-131: bg = bgnet(img, masks=body_mask, only_x=True) when no bg_img is supplied."""
    from impersonator_amd import demo
    net, sd = _net_and_sd(1)
    imitator, src_smpl, src_img, _ = demo.build_synthetic_imitator(batch_size=1, seed=0)
    imitator.bgnet = net
    imitator.personalize(src_img, src_smpl=src_smpl)
    si = imitator.src_info
    with torch.no_grad():
        bg_mask = torch_ref.morph(si["cond"][:, -1:].cpu(), imitator._opt.bg_ks, "erode")
        _, ox, _ = torch_ref.inpaint_forward(sd, torch.from_numpy(src_img)[None], 1 - bg_mask)
    assert float((si["bg"].cpu() - ox).abs().max()) <= 1e-3
    # the inpaintor runs on a side stream underneath the source-stream encoder (both bf16x3 / fp32 MFMA launches of 64-128
    # workgroups): the same call with everything in sequence on one stream must give the same bits, five times over
    import os
    keep = {k: si[k].clone() for k in ("bg",)}
    feats = [f.clone() for f in si["feats"][0] + si["feats"][1]]
    for rep in range(5):
        os.environ["LWG_BG_SIDE_STREAM"] = "0" if rep % 2 == 0 else "1"
        try:
            imitator.personalize(src_img, src_smpl=src_smpl)
        finally:
            os.environ.pop("LWG_BG_SIDE_STREAM", None)
        assert torch.equal(imitator.src_info["bg"], keep["bg"]), rep
        for a, b in zip(imitator.src_info["feats"][0] + imitator.src_info["feats"][1], feats):
            assert torch.equal(a, b), rep


def test_mfma_attention_equals_the_vector_alu_attention(tmp_path):
    """The 4096-token self-attention (networks/inpaintor.py:85-103) on the exact-fp32 matrix cores (attention_mfma_kernel: key
    chunks + combine) against the streaming vector-ALU kernel it replaces (LWG_ATTN=valu, read once per process: two runs): the
    same softmax and the same products, summed in another order -- the refined image agrees to 1e-5, and both sit within 2e-5 of
    the CPU oracle (bound of the whole network: 1e-3)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_inpaintor import _net_and_sd\n"
            "from impersonator_amd.utils import synthetic\n"
            "net, sd = _net_and_sd(0)\n"
            "img = torch.from_numpy(synthetic.smooth_image(5))\n"
            "yy, xx = np.mgrid[0:256, 0:256]\n"
            "mask = torch.from_numpy((((yy - 120) / 90.0) ** 2 + ((xx - 128) / 50.0) ** 2 < 1).astype(np.float32))[None, None]\n"
            "coarse, x, comp = net(img.cuda(), mask.cuda())\n"
            "np.save(sys.argv[1], x.cpu().numpy())\n" % root)
    outs = {}
    for mode in ("mfma", "valu"):
        path = str(tmp_path / (mode + ".npy"))
        env = dict(os.environ, PYTHONPATH=root, LWG_INPAINT_PRECISION="fp32")   # exact-fp32 convs: only the attention differs
        env.pop("LWG_ATTN", None)
        if mode == "valu":
            env["LWG_ATTN"] = "valu"
        p = subprocess.run([sys.executable, "-c", code, path], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[mode] = np.load(path)
    d = float(np.abs(outs["mfma"] - outs["valu"]).max())
    _, sd = _net_and_sd(0)
    img = torch.from_numpy(synthetic.smooth_image(5))
    yy, xx = np.mgrid[0:256, 0:256]
    mask = torch.from_numpy((((yy - 120) / 90.0) ** 2 + ((xx - 128) / 50.0) ** 2 < 1).astype(np.float32))[None, None]
    with torch.no_grad():
        _, ox, _ = torch_ref.inpaint_forward(sd, img, mask)
    e_m, e_v = float(np.abs(outs["mfma"] - ox.numpy()).max()), float(np.abs(outs["valu"] - ox.numpy()).max())
    print("attention: mfma vs valu %.3g; vs oracle: mfma %.3g, valu %.3g" % (d, e_m, e_v))
    assert d <= 1e-5 and e_m <= 2e-5 and e_v <= 2e-5, (d, e_m, e_v)


# ---------------------------------------------------------------------------------------------------------------------
# The self-attention on its own: lwg_inpaint_attention runs the launch code of lwg_inpaint_forward (launch_attention, inpaint.hip)
# on the cases of tests/helpers.py, which tests/test_inpaintor_cases.py proves on the CPU: exact one-hot, peaked, and sensitive --
# a wrong key/V pairing, a wrong tile, a lost chunk or a missing rescale moves the output by >= 5e4 x the bound held here.
# (tokens, kernel 0 vector ALU / 1 matrix cores, key chunks; 0 = the product's choice: 8 x 1 tile at 256 -- the loop never
# prefetches --, 16 x 2 at 1024, 12 x 6 at 2304 -- 9 query blocks --, 16 x 8 at 4096); 1 and 2 chunks at 1024: the longest tile
# loops (32 and 16 tiles), no merge and a trivial one
ATTN_CONFIGS = [(n, kern, 0) for n in sorted(helpers.ATTN_PRODUCT_CHUNKS) for kern in (0, 1)] + [(1024, 1, 1), (1024, 1, 2)]
_attn_id = lambda c: "N%d-%s-chunks%d" % (c[0], "mfma" if c[1] else "valu", c[2])


def _run_attention(case, kernel, key_chunks=0, split_out=0):
    """lwg_inpaint_attention on a case of tests/helpers.py -> out (N,128) on the CPU.  The output and the workspace start as NaN: a
    partial or an output nobody wrote shows."""
    import ctypes
    from impersonator_amd import _lib
    lib = _lib.load()
    N = case["N"]
    qkv, bias, x = case["qkv"].cuda(), case["bias"].cuda(), case["x"].cuda()
    out = torch.full((N, helpers.ATTN_C), float("nan"), device="cuda")
    nbytes = lib.lwg_inpaint_attention_workspace_bytes(N, kernel, key_chunks)
    assert (nbytes > 0) == (kernel == 1)
    ws = torch.full((nbytes // 4,), float("nan"), device="cuda") if nbytes else None
    _lib.check(lib.lwg_inpaint_attention(_lib.ptr(qkv), _lib.ptr(bias), _lib.ptr(x), ctypes.c_float(case["gamma"]), N, kernel,
                                         key_chunks, split_out, _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr()))
    return out.cpu()


@pytest.mark.parametrize("config", ATTN_CONFIGS, ids=_attn_id)
def test_attention_onehot_is_bit_exact(config):
    """The exact one-hot case (helpers.attention_onehot_case): every product and sum is exact in fp32 -- scores of +-64 x +-1, p in
    {0, 1}, l = 1, V / x / biases on a 2^-8 grid, gamma 0.5 -- so fused multiply-adds and the summation order cannot change a bit,
    and the output must EQUAL 0.5 (v + b_v)[perm[i]] + x[i].  A wrong key/V pairing, tile, chunk, buffer or bias slot, a missing max
    subtraction (exp(768) overflows) or a missing rescale ('last': everything accumulated before the last tile must be multiplied
    by exactly 0; 'first': nothing after the first tile may change it) is a gross mismatch."""
    N, kernel, chunks = config
    for winners in ("perm", "first", "last"):
        case = helpers.attention_onehot_case(N, winners)
        out = _run_attention(case, kernel, chunks)
        wrong = int((out != case["expected"]).sum())
        assert torch.equal(out, case["expected"]), (winners, wrong, float((out - case["expected"]).abs().max()))


@pytest.mark.parametrize("config", ATTN_CONFIGS, ids=_attn_id)
def test_attention_matches_fp64_within_4x_the_fp32_yardstick(config):
    """Flat (logit std 0.05) and peaked (2 and 8: a median of 21-157 and 1.7-2.0 effective keys) random cases against the fp64
    reference.  The yardstick is the error of the plain torch fp32 evaluation of the same formula on the same inputs against the same
    reference (computed here per case); the kernels are fp32 too -- another summation order, another expf -- and may be at most
    ATTN_TOL_FACTOR = 4 x as far.  Measured on MI355X, kernel error / yardstick at logit std (0.05, 2, 8):
        N256   valu 1.00 1.06 0.98   mfma 8 chunks  1.00 1.04 0.98
        N1024  valu 1.00 0.93 0.97   mfma 16 chunks 1.00 0.79 0.97   1 chunk 1.00 1.39 1.12   2 chunks 1.00 1.34 1.03
        N2304  valu 1.00 1.35 0.87   mfma 12 chunks 1.00 1.06 1.01
        N4096  valu 1.03 1.32 0.99   mfma 16 chunks 1.03 1.22 0.98
    (yardsticks 2.0e-7 to 2.3e-7 flat, 1.0e-6 to 1.4e-6 at std 2, 3.8e-6 to 7.6e-6 at std 8).  This test found attention_kernel
    summing all N keys in one chain: valu 4.35 / 6.30 at N4096 std 0.05 / 2 (1.98 at N1024, 2.53 at N2304 std 2) before it got
    per-tile partial sums."""
    N, kernel, chunks = config
    for std in (0.05, 2.0, 8.0):
        case = helpers.attention_checked_case(N, std)
        err = float((_run_attention(case, kernel, chunks).double() - case["ref"]).abs().max())
        print("attention %s logit std %.2f: kernel vs fp64 %.3g, torch fp32 vs fp64 %.3g, ratio %.2f" %
              (_attn_id(config), std, err, case["yardstick"], err / case["yardstick"]))
        assert err <= helpers.ATTN_TOL_FACTOR * case["yardstick"], (std, err, case["yardstick"])


@pytest.mark.parametrize("N", sorted(helpers.ATTN_PRODUCT_CHUNKS))
def test_attention_mfma_and_valu_agree_on_peaked_cases(N):
    """Both kernels in one process (the `kernel` argument; the product switches by LWG_ATTN, read once per process) on the peaked
    cases: each within 4 x the fp32 yardstick of the fp64 reference; their mutual difference is printed.  Measured on MI355X at
    N = 256 / 1024 / 2304 / 4096: mfma vs valu 1.0e-6 / 1.2e-6 / 1.3e-6 / 1.9e-6 at std 2, 2.5e-6 / 3.3e-6 / 3.8e-6 / 5.0e-6 at
    std 8; kernel error / yardstick between 0.79 and 1.35."""
    for std in (2.0, 8.0):
        case = helpers.attention_checked_case(N, std)
        mfma, valu = _run_attention(case, 1), _run_attention(case, 0)
        e_m, e_v = (float((o.double() - case["ref"]).abs().max()) for o in (mfma, valu))
        print("attention N=%d logit std %.0f: mfma vs valu %.3g; vs fp64: mfma %.3g, valu %.3g, torch fp32 %.3g" %
              (N, std, float((mfma - valu).abs().max()), e_m, e_v, case["yardstick"]))
        assert max(e_m, e_v) <= helpers.ATTN_TOL_FACTOR * case["yardstick"], (std, e_m, e_v, case["yardstick"])


@pytest.mark.parametrize("config", [c for c in ATTN_CONFIGS if c[1] == 1], ids=_attn_id)
def test_attention_split_bf16_output(config):
    """attention_combine_kernel's split-bf16 output (what refine_upsample_net's first bf16x3 conv reads): the same call with
    split_out 0 and 1; per 32 channels the buffer holds 32 bf16 hi then 32 bf16 lo (csrc/conv.h), hi = bf16(r), lo = bf16(r - hi)
    of the fp32 result r, exactly."""
    N, kernel, chunks = config
    case = helpers.attention_checked_case(N, 2.0)
    r = _run_attention(case, kernel, chunks, split_out=0)
    assert float((r.double() - case["ref"]).abs().max()) <= helpers.ATTN_TOL_FACTOR * case["yardstick"]
    hi, lo = helpers.split_bf16_decode(_run_attention(case, kernel, chunks, split_out=1))
    want_hi, want_lo = helpers.split_bf16_encode(r)
    assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo), (int((hi != want_hi).sum()), int((lo != want_lo).sum()))


# query and key conv weights x QK_SCALE: with the seeded weights alone the softmax is flat (logit std 0.05) and the attention term is
# the mean of V whatever the kernel pairs.  Chosen on the CPU oracle: x 16 on the query alone leaves 681 of 1024 effective keys, x 16
# on both 57 of 256 at 64 x 64 pixels; x 32 on both gives a median of 11.9 / 10.6 / 10.6 effective keys of 256 / 1024 / 2304.
QK_SCALE = 32.0


@pytest.mark.parametrize("size", (64, 128, 192))
def test_inpaintor_other_sizes_with_a_peaked_attention(size):
    """InpaintSANet(image_size=64 / 128 / 192): gated convs down to 16 x 16, 32 x 32 and 48 x 48 maps, attention over 256, 1024 and
    2304 tokens (8 x 1, 16 x 2 and 12 x 6 key tiles), with an attention that matters -- condition, checked on the oracle's own logits:
    median effective key count <= N / 8.  Against the fp64 oracle on the same weights: fp32 mode at most 4 x as far as the fp32
    oracle is, bf16x3 within the network bound 1e-3.  Measured on MI355X, worst of (coarse, x, comp) against the fp64 oracle:
        64 x 64    fp32 oracle 1.46e-7   fp32 mode 1.72e-7 (ratio 1.18)   bf16x3 1.80e-6   11.9 effective keys of 256
        128 x 128  fp32 oracle 1.36e-7   fp32 mode 2.42e-7 (ratio 1.78)   bf16x3 1.77e-6   10.6 of 1024
        192 x 192  fp32 oracle 1.52e-7   fp32 mode 2.03e-7 (ratio 1.34)   bf16x3 1.69e-6   10.6 of 2304"""
    from impersonator_amd.networks.inpaintor import InpaintSANet
    net = InpaintSANet(c_dim=4, image_size=size).eval()
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in synthetic.random_inpaintor_state_dict(shapes, 0).items()}
    for k in ("refine_attn.query_conv.weight", "refine_attn.key_conv.weight"):
        sd[k] = sd[k] * QK_SCALE
    net.load_state_dict(sd)
    net = net.cuda()
    img = torch.from_numpy(synthetic.smooth_image(5, (1, 3, size, size)))
    yy, xx = np.mgrid[0:size, 0:size]
    r = size / 256.0
    mask = torch.from_numpy((((yy - 120 * r) / (90.0 * r)) ** 2 + ((xx - 128 * r) / (50.0 * r)) ** 2 < 1).astype(np.float32))[None, None]
    probe = {}
    with torch.no_grad():
        o32 = torch_ref.inpaint_forward(sd, img, mask, probe=probe)
        o64 = torch_ref.inpaint_forward({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, img.double(),
                                        mask.double())
    N = (size // 4) ** 2
    eff = float(helpers.effective_keys(probe["attn_logits"]).median())
    yard = max(float((a.double() - b).abs().max()) for a, b in zip(o32, o64))
    print("inpaintor %d x %d: %d tokens, median effective keys %.1f, fp32 oracle vs fp64 %.3g" % (size, size, N, eff, yard))
    assert probe["attn_logits"].shape == (N, N) and eff <= N / 8
    outs, errs = {}, {}
    for prec in ("bf16x3", "fp32"):
        net.precision = prec
        outs[prec] = [t.cpu() for t in net(img.cuda(), mask.cuda())]
        errs[prec] = [float((a.double() - b).abs().max()) for a, b in zip(outs[prec], o64)]
        print("    %s vs fp64 oracle (coarse, x, comp): %s" % (prec, ["%.3g" % e for e in errs[prec]]))
    net.release()
    assert not torch.equal(outs["bf16x3"][1], outs["fp32"][1]), "the bf16x3 route did not run"
    assert max(errs["bf16x3"]) <= 1e-3, errs
    assert max(errs["fp32"]) <= 4 * yard, (errs["fp32"], yard)
