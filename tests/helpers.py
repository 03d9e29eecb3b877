"""Shared fixtures for the parity tests: the seeded synthetic scene of tests/golden/make_golden.py,
rebuilt WITHOUT the reference (it does not exist on the GPU box)."""
import functools
import os

import numpy as np
import torch

from impersonator_amd.utils import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def has_gpu():
    return torch.cuda.is_available()


def scene():
    """Numpy/torch CPU inputs identical to make_golden.make_frame()."""
    rest, faces = synthetic.body_mesh()
    s = dict(rest=rest, faces=faces, map_fn=synthetic.uv_seg_map_fn(rest, faces))
    s["src_cam"] = synthetic.cams(1, seed=100)
    s["src_verts"] = rest[None].copy()
    s["src_img"] = synthetic.smooth_image(11)
    s["bg_img"] = synthetic.smooth_image(12)
    s["tgt_verts"] = np.stack([synthetic.motion_verts(rest, t) for t in (3, 200)])
    s["tgt_cam"] = synthetic.cams(2, seed=5)
    return s


def generator_state_dict(seed=0, affine="random"):
    """Seeded weights keyed like ImpersonatorGenerator.state_dict() (numpy)."""
    from impersonator_amd.networks.generator import ImpersonatorGenerator
    G = ImpersonatorGenerator(bg_dim=4, src_dim=6, tsf_dim=6, repeat_num=6)
    shapes = [(k, tuple(v.shape)) for k, v in G.state_dict().items()]
    return synthetic.random_state_dict(shapes, seed=seed, affine=affine)


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def t(x, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def maxdiff(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.from_numpy(np.asarray(b)).double()
    d = (a - b).abs()
    idx = int(d.argmax())
    return float(d.max()), np.unravel_index(idx, tuple(d.shape))


def discriminator_state_dict(seed=0, input_nc=6, ndf=64, n_layers=4):
    """Seeded PatchDiscriminator parameters (conv weights ~ N(0, 0.02) as networks.py:57-58, biases ~ U(-0.1, 0.1))."""
    import torch
    g = torch.Generator().manual_seed(seed)
    sd, idx, cin, mult = {}, 0, input_nc, 1
    chans = [ndf] + [ndf * min(2 ** n, 8) for n in range(1, n_layers)] + [ndf * min(2 ** n_layers, 8), 1]
    for l, cout in enumerate(chans):
        sd["model.%d.weight" % idx] = torch.randn(cout, cin, 4, 4, generator=g) * 0.02
        sd["model.%d.bias" % idx] = torch.rand(cout, generator=g) * 0.2 - 0.1
        idx += 2 if l == 0 else 3
        cin = cout
    return sd


def vgg19_state_dict(seed=0):
    """Random VGG19 conv stack in torchvision's naming (features.N.weight / .bias) up to relu5_1 -- the real weights are a
    download; He-scaled so that activations keep their magnitude through the 13 layers."""
    import torch
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for idx, cout in [(0, 64), (2, 64), (5, 128), (7, 128), (10, 256), (12, 256), (14, 256), (16, 256), (19, 512), (21, 512),
                      (23, 512), (25, 512), (28, 512)]:
        sd["features.%d.weight" % idx] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd["features.%d.bias" % idx] = torch.randn(cout, generator=g) * 0.05
        cin = cout
    return sd


def sphere20a_state_dict(seed=0):
    """Random Sphere20a (networks/facenet.py:200-262) in its own state_dict naming -- the real file
    (sphere20a_20171020.pth) is a download; He-scaled convs, PReLU slopes around 0.25."""
    import torch
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for st, c, units in (("1", 64, 1), ("2", 128, 2), ("3", 256, 4), ("4", 512, 1)):
        for j in range(1, 2 + 2 * units):
            name = "%s_%d" % (st, j)
            ci = cin if j == 1 else c
            sd["conv%s.weight" % name] = torch.randn(c, ci, 3, 3, generator=g) * (1.0 / (9 * ci)) ** 0.5
            sd["conv%s.bias" % name] = torch.randn(c, generator=g) * 0.05
            sd["relu%s.weight" % name] = 0.25 + 0.1 * torch.rand(c, generator=g)
        cin = c
    sd["fc5.weight"] = torch.randn(512, 512 * 7 * 6, generator=g) * (1.0 / (512 * 42)) ** 0.5
    sd["fc5.bias"] = torch.randn(512, generator=g) * 0.05
    return sd


def train_batch(seed=0, n=2, size=64, bg_both=False):
    """Seeded stand-in for what the reference's BodyRecoveryFlow hands the trainer (impersonator_trainer.py:300-319);
    bg_both: the background input carries the source's and the target's (2n images, :333-337)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    T = torch.rand(n, size, size, 2, generator=g) * 2.4 - 1.2
    T[0, size // 4:size // 2, size // 8:size // 3] = -2
    if bg_both:
        return dict(input_G_src=r(n, 6, size, size), input_G_tsf=r(n, 6, size, size), T=T, real_src=r(n, 3, size, size),
                    real_tsf=r(n, 3, size, size), bg_mask=(torch.rand(2 * n, 1, size, size, generator=g) > 0.5).float(),
                    input_G_bg=r(2 * n, 4, size, size))
    return dict(input_G_bg=r(n, 4, size, size), input_G_src=r(n, 6, size, size), input_G_tsf=r(n, 6, size, size), T=T,
                real_src=r(n, 3, size, size), real_tsf=r(n, 3, size, size),
                bg_mask=(torch.rand(2 * n, 1, size, size, generator=g) > 0.5).float())


class FixedHMR(object):
    """`hmr` stand-in: get_details() hands out prepared (cam, verts) in call order (the SMPL regressor / LBS are not
    what these fixtures pin)."""

    def __init__(self, infos):
        self.infos = list(infos)

    def get_details(self, smpl):
        cam, verts = self.infos.pop(0)
        return dict(theta=smpl, cam=cam, pose=smpl[:, 3:75], shape=smpl[:, 75:], verts=verts)

    def cuda(self):
        return self


def task_scene():
    """Inputs of tests/golden/tasks_golden.npz (numpy): two subjects (rest pose / frame 200 of the synthetic motion, own
    cameras and images), the synthetic 10-part partition, two views."""
    rest, faces = synthetic.body_mesh()
    part_fn, part_faces = synthetic.part_map_fn(rest, faces)
    return dict(rest=rest, faces=faces, map_fn=synthetic.uv_seg_map_fn(rest, faces), part_fn=part_fn, part_faces=part_faces,
                cam_a=synthetic.cams(1, seed=100), verts_a=rest[None].copy(), img_a=synthetic.smooth_image(11),
                cam_b=synthetic.cams(1, seed=101), verts_b=synthetic.motion_verts(rest, 200)[None].copy(),
                img_b=synthetic.smooth_image(77),
                views=[((0.0, 0.6, 0.0), (0.0, 0.0, 0.0), False), ((0.2, -1.1, 0.1), (0.02, 0.0, 0.0), True)])


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/imitator_golden.npz: the reference's own Imitator methods run unbound (make_golden.py::make_imitator)
IMITATOR_VARIANTS = {
    # name: image size, --only_vis, --bg_model (ORIGINAL = the generator's BGNet, else InpaintSANet), --front_warp, --cam_strategy
    "main": dict(size=256, only_vis=False, bg_model="ORIGINAL", front_warp=False, cam_strategy="smooth"),
    "vis_inpaint_front_source": dict(size=128, only_vis=True, bg_model="deepfillv2", front_warp=True, cam_strategy="source"),
    "vis_bgnet_front_copy": dict(size=128, only_vis=True, bg_model="ORIGINAL", front_warp=True, cam_strategy="copy"),
    "inpaint_smooth": dict(size=128, only_vis=False, bg_model="deepfillv2", front_warp=False, cam_strategy="smooth"),
}


def imitator_scene(size):
    """Inputs of imitator_golden.npz (numpy) at one image size: synthetic SMPL model + mesh tables, one source (rest pose,
    own camera and betas), four target SMPL vectors far apart in the synthetic motion, seeded images."""
    from impersonator_amd import demo
    from impersonator_amd.networks.batch_smpl import synthetic_smpl_params
    rest, faces = synthetic.body_mesh()
    src_smpl = demo.synthetic_smpls(1, seed=1)[0]
    src_smpl[3:75] = 0.0
    return dict(rest=rest, faces=faces, map_fn=synthetic.uv_seg_map_fn(rest, faces), front_map_fn=synthetic.front_map_fn(rest, faces),
                smpl_params=synthetic_smpl_params(0), src_smpl=src_smpl, tgt_smpls=demo.synthetic_smpls(64, seed=0)[::16].copy(),
                src_img=synthetic.smooth_image(11, (1, 3, size, size)), size=size)


def inpaintor_state_dict(seed=1):
    """Seeded InpaintSANet(c_dim=4) weights (numpy), keyed like the reference's state_dict."""
    from impersonator_amd.networks.inpaintor import InpaintSANet
    shapes = [(k, tuple(v.shape)) for k, v in InpaintSANet(c_dim=4).state_dict().items()]
    return synthetic.random_inpaintor_state_dict(shapes, seed)


def tensor_stat(x):
    x = torch.as_tensor(x).double()
    return np.array([x.mean().item(), x.abs().mean().item(), (x * x).mean().item()])


# ---------------------------------------------------------------------------------------------------------------------
# The inpaintor's self-attention on its own (lwg_inpaint_attention): case builders and the fp64 reference.
#   out = gamma * softmax((q + b_q)(k + b_k)^T)(v + b_v) + x,  qkv (N,192) raw [q 16 | k 16 | v 128 | 32 unused], bias (192) alike
ATTN_D, ATTN_C, ATTN_LD, ATTN_TILE = 16, 128, 192, 32
# token count -> key chunks lwg_inpaint_create picks for the matrix-core kernel (tests/test_abi.py reads the same numbers back
# from lwg_inpaint_attention_workspace_bytes): 1, 2, 6 and 8 tiles of 32 keys per chunk
ATTN_PRODUCT_CHUNKS = {256: 8, 1024: 16, 2304: 12, 4096: 16}


def _attn_pack(q, k, v, bq, bk, bv, x, gamma):
    """Targets (q, k, v: what the kernel must see AFTER the bias add) -> the raw buffers: raw = target - bias."""
    N = q.shape[0]
    qkv = torch.zeros(N, ATTN_LD, dtype=torch.float32)
    qkv[:, :ATTN_D], qkv[:, ATTN_D:2 * ATTN_D], qkv[:, 2 * ATTN_D:2 * ATTN_D + ATTN_C] = q - bq, k - bk, v - bv
    bias = torch.zeros(ATTN_LD, dtype=torch.float32)
    bias[:ATTN_D], bias[ATTN_D:2 * ATTN_D], bias[2 * ATTN_D:2 * ATTN_D + ATTN_C] = bq, bk, bv
    return dict(qkv=qkv, bias=bias, x=x.float().contiguous(), gamma=float(gamma), N=N)


def attention_onehot_case(N, winners="perm", seed=0):
    """A softmax that is EXACTLY one-hot in fp32.  Key j is the 12-bit +-1 code of j (dimensions 12-15 zero), query i is 64 x the
    code of perm[i]: the winning logit is 64 * 12 = 768, any other key differs in >= 1 bit, <= 640, and exp(-128) is 0 in fp32
    (smallest denormal 1.4e-45): every other probability is exactly 0, l exactly 1.  V, x and the biases lie on a 2^-8 grid with
    |.| <= 4, gamma = 0.5, raw = target - bias (exact, so is the kernel's bias add): every product and sum of the computation is
    exact and the output is 0.5 * (v + b_v)[perm[i]] + x[i] bit for bit, whatever the summation order or contraction.
    winners: 'perm' a seeded permutation; 'first' / 'last': every winner inside the first / last 32-key tile (nothing / everything
    accumulated before it has to be rescaled by exactly 0).  -> case dict with 'expected' (N,128) and 'perm'."""
    assert N <= 4096
    g = torch.Generator().manual_seed(1000 + seed)
    grid = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float() / 256.0
    code = torch.zeros(N, ATTN_D)
    idx = torch.arange(N)
    for b in range(12):
        code[:, b] = ((idx >> b) & 1).float() * 2 - 1
    if winners == "perm":
        perm = torch.randperm(N, generator=g)
    else:
        perm = torch.randint(0, ATTN_TILE, (N,), generator=g) + (0 if winners == "first" else N - ATTN_TILE)
    v, x = grid(-1024, 1024, N, ATTN_C), grid(-1024, 1024, N, ATTN_C)
    bq, bk, bv = grid(-64, 64, ATTN_D), grid(-64, 64, ATTN_D), grid(-64, 64, ATTN_C)
    case = _attn_pack(64.0 * code[perm], code, v, bq, bk, bv, x, 0.5)
    case["perm"] = perm
    case["expected"] = 0.5 * v[perm] + x
    return case


def attention_random_case(N, logit_std, seed=0):
    """Raw q, k ~ N(0, s^2) with 4 s^2 = logit_std (16 products of two N(0, s^2) values), V, x ~ N(0,1), biases ~ N(0, 0.1^2),
    gamma = 0.7.  logit_std 2 and 8 give a peaked softmax (a few to a few hundred effective keys), 0.05 the flat one of the seeded
    network."""
    g = torch.Generator().manual_seed(2000 + seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    s = (logit_std / 4.0) ** 0.5
    qkv = torch.zeros(N, ATTN_LD)
    qkv[:, :2 * ATTN_D] = r(N, 2 * ATTN_D) * s
    qkv[:, 2 * ATTN_D:2 * ATTN_D + ATTN_C] = r(N, ATTN_C)
    bias = torch.zeros(ATTN_LD)
    bias[:2 * ATTN_D + ATTN_C] = r(2 * ATTN_D + ATTN_C) * 0.1
    return dict(qkv=qkv, bias=bias, x=r(N, ATTN_C), gamma=0.7, N=N)


def attention_parts(case, dtype=torch.float64):
    """(logits (N,N), v + b_v (N,128)) of a case, the float32 inputs converted to `dtype` before the first operation."""
    qkv, bias = case["qkv"].to(dtype), case["bias"].to(dtype)
    t = qkv + bias
    return t[:, :ATTN_D] @ t[:, ATTN_D:2 * ATTN_D].T, t[:, 2 * ATTN_D:2 * ATTN_D + ATTN_C]


def attention_reference(case, dtype=torch.float64):
    """out = gamma * softmax((q + b_q)(k + b_k)^T)(v + b_v) + x, plainly, in `dtype` (float64: the reference; float32: the yardstick
    of what fp32 arithmetic costs on these inputs)."""
    logits, v = attention_parts(case, dtype)
    return case["gamma"] * (torch.softmax(logits, dim=-1) @ v) + case["x"].to(dtype)


@functools.lru_cache(maxsize=None)
def _attention_ref_and_yardstick(N, logit_std):
    case = attention_random_case(N, logit_std)
    ref = attention_reference(case)
    return ref, float((attention_reference(case, torch.float32).double() - ref).abs().max())


def attention_checked_case(N, logit_std):
    """attention_random_case (a fresh dict per call) plus 'ref' (the fp64 reference) and 'yardstick' (max |fp32 evaluation - ref| of
    the same formula on the same inputs), those two computed once per process.  The GPU kernels are fp32 with another summation
    order and another expf: ATTN_TOL_FACTOR x the yardstick is their bound."""
    case = attention_random_case(N, logit_std)
    ref, case["yardstick"] = _attention_ref_and_yardstick(N, logit_std)
    case["ref"] = ref.clone()
    return case


ATTN_TOL_FACTOR = 4.0


def effective_keys(logits):
    """1 / sum p^2 per query: how many keys share the softmax."""
    p = torch.softmax(logits.double(), dim=-1)
    return 1.0 / (p * p).sum(-1)


def attention_mutant(case, which, key_chunks):
    """The fp64 reference with one indexing bug of the kind the kernels could have:
    'pair'    V rows of keys k and k ^ 4 swapped (the half-wave pairing of p[r] with V rows);
    'tiles'   V tiles 0 and 1 (keys 0-31 / 32-63) swapped (a stale double buffer);
    'chunk'   the last of key_chunks key chunks dropped, the rest renormalised (a lost partial);
    'rescale' online softmax over 32-key tiles whose accumulator is never rescaled when the running max moves (l is)."""
    logits, v = attention_parts(case)
    N = case["N"]
    idx = torch.arange(N)
    if which == "pair":
        attn = torch.softmax(logits, -1) @ v[idx ^ 4]
    elif which == "tiles":
        j = idx.clone()
        j[:ATTN_TILE], j[ATTN_TILE:2 * ATTN_TILE] = idx[ATTN_TILE:2 * ATTN_TILE], idx[:ATTN_TILE]
        attn = torch.softmax(logits, -1) @ v[j]
    elif which == "chunk":
        keep = N - N // key_chunks
        attn = torch.softmax(logits[:, :keep], -1) @ v[:keep]
    elif which == "rescale":
        tmax = logits.view(N, N // ATTN_TILE, ATTN_TILE).max(-1).values
        run = torch.cummax(tmax, dim=1).values                              # the running max when a tile is accumulated
        m = run[:, -1:]
        p_stale = torch.exp(logits - run.repeat_interleave(ATTN_TILE, dim=1))   # never brought down to the final max
        attn = (p_stale @ v) / torch.exp(logits - m).sum(-1, keepdim=True)
    else:
        raise ValueError(which)
    return case["gamma"] * attn + case["x"].double()


def split_bf16_encode(r):
    """fp32 (N, C), C % 32 == 0 -> the split-bf16 format (csrc/conv.h, split.h) as (hi, lo) bf16 tensors of r's shape."""
    hi = r.to(torch.bfloat16)
    return hi, (r - hi.float()).to(torch.bfloat16)


def split_bf16_decode(buf):
    """A split-bf16 buffer viewed as fp32 (N, C) -> (hi, lo) bf16 (N, C): per 32 channels, 128 bytes = [32 bf16 hi | 32 bf16 lo]."""
    N, C = buf.shape
    h = buf.contiguous().view(torch.bfloat16).view(N, C // 32, 2, 32)
    return h[:, :, 0].reshape(N, C), h[:, :, 1].reshape(N, C)


# ---------------------------------------------------------------------------------------------------------------------
# The two direct kernels of the bf16x3 inference path on their own (lwg_stem_forward, lwg_heads_inference): seeded inputs, the
# float64 references and a float64 restatement of the split arithmetic.  tests/test_direct_cases.py proves on the CPU that the
# restatement sits inside a third of every bound tests/test_gpu_direct_kernels.py holds the kernels to.
BF16X3_REL = 3e-5        # bf16x3 against float64, relative to max |reference| (the bound of tests/test_gpu_ops.py)
FP32_REL = 1e-5          # exact-fp32 kernels, same convention (tests/test_gpu_ops.py)
ACT_ABS = 1e-5           # tanh / sigmoid allowance of test_heads_ops; also the whole fp32 heads bound
# (mean, M2) partials of the stem: relative error of the restatement's M2 per 128-pixel tile against float64, relative to
# max |M2|, measured over STEM_CASES (test_direct_cases.py prints it per case and asserts that none exceeds this figure):
STEM_M2_MEASURED = 2.2e-6   # 1.74e-6 to 2.17e-6 over the five cases, the worst on (2,8,384)
STEM_M2_REL = 10 * STEM_M2_MEASURED

# (N, H, W, cin, grids): grids = the max_workgroups values to run (0: the launcher's own grid)
STEM_CASES = [
    (1, 2, 128, 6, (0,)),        # one tile, every pixel at a border, the workgroup's second four-wave group idle
    (1, 6, 128, 6, (1,)),        # three tiles on one workgroup: group 0 walks two, group 1 one
    (1, 6, 128, 3, (1,)),        # cin 3: the filter bank's entries of the missing channels stay zero
    (3, 4, 256, 6, (1, 2, 0)),   # six / three tiles per group, tiles cross image boundaries, a real left halo
    (2, 8, 384, 6, (0,)),        # three tiles per row
]
# (N, H, W, w_rows, bands tuple)
HEADS_CASES = [(2, H, 27, 4, (0,)) for H in range(1, 9)] + [   # one band of H rows: every residue of the accumulator ring's last slot;
                                                               # the second strip owns a single column
    (2, 8, 26, 8, (0,)),          # exactly one strip; weight rows 4-7 hold garbage
    (2, 8, 5, 4, (0,)),           # narrower than the kernel
    (3, 45, 104, 8, (4, 1, 0)),   # bands of 12, 12, 12, 9 rows / one band of 51 steps (six ring laps) / the launcher's choice
    (2, 24, 64, 4, (3, 0)),       # band edges on multiples of 8
]


def bf16_split(v):
    """fp32 tensor -> (hi, lo) as float64: hi = bf16(v), lo = bf16(v - hi), round to nearest even like the hardware conversion."""
    v = v.float()
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def conv7_bf16x3(x, w, drop=None):
    """The split arithmetic restated in float64: 7x7 / pad 3 convolution of x (N,C,H,W) with w (O,C,7,7), both fp32, as
    lo*hi + hi*lo + hi*hi of their bf16 halves (every product exact, sums in float64).  drop: 'lo_hi' / 'hi_lo' leaves that cross
    product out (a mutant for the sensitivity checks)."""
    import torch.nn.functional as F
    xh, xl = bf16_split(x)
    wh, wl = bf16_split(w)
    y = F.conv2d(xh, wh, None, 1, 3)
    if drop != "lo_hi":
        y = y + F.conv2d(xl, wh, None, 1, 3)
    if drop != "hi_lo":
        y = y + F.conv2d(xh, wl, None, 1, 3)
    return y


@functools.lru_cache(maxsize=None)
def stem_case(N, H, W, cin):
    """Seeded inputs and the float64 reference of one stem case (shared: treat as read-only).  x8 (N,H,W,8): uniform [-1,1] in
    channels 0..cin-1, non-zero finite garbage in every other channel (6-7 are never read, cin..5 meet zero weights); w 0.05 randn.
    ref (N,H,W,64) float64 = F.conv2d; mean / m2 (N*H*W/128, 64): float64 statistics of ref over each run of 128 pixels."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4000 + 97 * N + 13 * H + W + cin)
    x8 = (torch.rand(N, H, W, 8, generator=g) + 0.5) * 1000.0 * (torch.randint(0, 2, (N, H, W, 8), generator=g) * 2 - 1).float()
    x8[..., :cin] = torch.rand(N, H, W, cin, generator=g) * 2 - 1
    w = torch.randn(64, cin, 7, 7, generator=g) * 0.05
    xc = x8[..., :cin].permute(0, 3, 1, 2).contiguous()
    ref = F.conv2d(xc.double(), w.double(), None, 1, 3).permute(0, 2, 3, 1).contiguous()
    tiles = ref.reshape(-1, 128, 64)
    mean = tiles.mean(1)
    m2 = ((tiles - mean[:, None]) ** 2).sum(1)
    return dict(x8=x8, x=xc, w=w, ref=ref, mean=mean, m2=m2, N=N, H=H, W=W, cin=cin)


def tile_stats(y):
    """(N,H,W,64) -> float64 (mean, M2) per run of 128 consecutive pixels: the mtile = pixel / 128 order of launch_in_finalize."""
    tiles = y.double().reshape(-1, 128, 64)
    mean = tiles.mean(1)
    return mean, ((tiles - mean[:, None]) ** 2).sum(1)


def heads_activation(x, ss, dtype):
    """relu(x * scale + shift) as (N,64,H,W).  float64: exactly; float32: one rounding of the exact product-sum, i.e. fmaf."""
    v = x.double() * ss[:, None, None, :, 0].double() + ss[:, None, None, :, 1].double()
    return v.to(dtype).clamp(min=0).permute(0, 3, 1, 2).contiguous()


def heads_outputs(pre, bg):
    """pre (N,4,H,W) float64 -> dict(pre, color, mask, pred): tanh, sigmoid and the blend mask*bg + (1-mask)*color."""
    color, mask = torch.tanh(pre[:, 0:3]), torch.sigmoid(pre[:, 3:4])
    return dict(pre=pre, color=color, mask=mask, pred=mask * bg.double() + (1 - mask) * color)


@functools.lru_cache(maxsize=None)
def heads_case(N, H, W, w_rows):
    """Seeded inputs and the float64 reference of one heads case (shared: treat as read-only).  x (N,H,W,64) randn; ss (N,64,2) =
    (scale randn -- negative ones included, shift 0.5 randn -- positive ones included, so padding with relu(shift) instead of 0
    shows); w (w_rows,64,7,7): rows 0-3 0.03 randn, further rows garbage; bg (N,3,H,W) uniform [-1,1].  ref: heads_outputs of the
    float64 F.conv2d on the float64 activation."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5000 + 977 * N + 131 * H + 7 * W + w_rows)
    x = torch.randn(N, H, W, 64, generator=g)
    ss = torch.stack([torch.randn(N, 64, generator=g), 0.5 * torch.randn(N, 64, generator=g)], dim=-1).contiguous()
    w = torch.randn(w_rows, 64, 7, 7, generator=g) * 7.0
    w[:4] = torch.randn(4, 64, 7, 7, generator=g) * 0.03
    bg = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    pre = F.conv2d(heads_activation(x, ss, torch.float64), w[:4].double(), None, 1, 3)
    return dict(x=x, ss=ss, w=w, bg=bg, ref=heads_outputs(pre, bg), N=N, H=H, W=W)


def heads_restatement(case, drop=None, pad_relu_shift=False):
    """heads_outputs of the bf16x3 restatement: conv7_bf16x3 on relu(fmaf(x, scale, shift)) in fp32.  pad_relu_shift: the mutant
    that normalises the zero padding too (a padded tap contributes relu(shift) instead of 0), in exact float64."""
    import torch.nn.functional as F
    if pad_relu_shift:
        a = heads_activation(case["x"], case["ss"], torch.float64)
        N, C, H, W = a.shape
        padded = case["ss"][:, :, 1].double().clamp(min=0)[:, :, None, None].expand(N, C, H + 6, W + 6).clone()
        padded[:, :, 3:-3, 3:-3] = a
        return heads_outputs(F.conv2d(padded, case["w"][:4].double()), case["bg"])
    return heads_outputs(conv7_bf16x3(heads_activation(case["x"], case["ss"], torch.float32), case["w"][:4], drop), case["bg"])


def heads_bounds(case, precision):
    """(colour bound, mask bound) absolute: |tanh'| <= 1, |sigmoid'| <= 1/4 on the pre-activation bound, plus the activation
    allowance; the exact-fp32 kernel keeps the 1e-5 of test_heads_ops."""
    if precision == "fp32":
        return ACT_ABS, ACT_ABS
    pre_max = float(case["ref"]["pre"].abs().max())
    return BF16X3_REL * pre_max + ACT_ABS, BF16X3_REL * pre_max / 4 + ACT_ABS


# ---------------------------------------------------------------------------------------------------------------------
# Order-independent exactness of the bf16x3 (and fp32) convolutions and their gradients: operands on a coarse binary grid.
# One operand is n / 256 with |n| <= 511 (ten significant bits: it needs its lo term), the other m / 16 with |m| <= 8 (bf16
# carries it: no lo term, so no lo * lo product is missing from hi*hi + hi*lo + lo*hi).  Every product is a multiple of 2^-12;
# where the sum of |products| of an output stays below 2^24 quanta, every partial sum in ANY order is an fp32 number and the
# float64 result rounded to fp32 is the specification, bit for bit.  tests/test_gpu_halo_mfma_shape.py and
# tests/test_gpu_conv_exact.py hold the kernels to it; tests/test_conv_exact_cases.py proves the conditions and that a wrong
# hi/lo pairing or tile placement cannot meet it.
EXACT_FAMILIES = ("a_lo", "b_lo")   # which operand carries the lo term: (activation, weight) forward and data gradient, (x, dy) wgrad
EXACT_NCU = 256                     # the CU count the CPU statement of the CU-sized batches uses (an MI355X)


def grid(shape, g, limit, denom):
    """integers in [-limit, limit] over denom"""
    return torch.randint(-limit, limit + 1, shape, generator=g).float() / denom


def exact_operands(family, shape_a, shape_b, g):
    """family 'a_lo': A = n / 256, |n| <= 511, B = m / 16, |m| <= 8; 'b_lo': the converse (A is drawn first in both)"""
    if family == "a_lo":
        return grid(shape_a, g, 511, 256.0), grid(shape_b, g, 8, 16.0)
    assert family == "b_lo"
    return grid(shape_a, g, 8, 16.0), grid(shape_b, g, 511, 256.0)


def bf16_split_f32(t):
    """fp32 tensor -> (hi, lo) as fp32: hi = bf16(t), lo = bf16(t - hi)"""
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi, lo


class ConvCase(object):
    """One op-level call.  kind 'fwd': operands (x, w) -> y; 'dgrad': (dy, w) -> dx; 'wgrad': (x, dy) -> dW.  H x W is the layer's
    INPUT map, N a number or a function of the CU count.  axes: per operand, the axis of the channels that the split format
    groups by 32 (the reduction channels of the forward pass and the data gradient).  pixels: per operand, whether its last axis
    walks the pixels of a row.  midrow: a 128-pixel tile of the kernel's output starts inside a row and the conv has padding."""

    def __init__(self, kind, cin, cout, k, stride, pad, H, W, N, transposed=False, midrow=False, expect=None, precision="bf16x3"):
        self.kind, self.cin, self.cout, self.k, self.stride, self.pad = kind, cin, cout, k, stride, pad
        self.H, self.W, self.N, self.transposed, self.midrow, self.expect, self.precision = H, W, N, transposed, midrow, expect, precision

    def batch(self, ncu):
        return self.N(ncu) if callable(self.N) else self.N

    def out_hw(self):
        if self.transposed:
            return 2 * self.H, 2 * self.W
        return (self.H + 2 * self.pad - self.k) // self.stride + 1, (self.W + 2 * self.pad - self.k) // self.stride + 1

    def w_shape(self):
        return (self.cin, self.cout, self.k, self.k) if self.transposed else (self.cout, self.cin, self.k, self.k)

    def shapes(self, ncu):
        """the two operands' shapes (NCHW / the weight's own layout)"""
        n, (ho, wo) = self.batch(ncu), self.out_hw()
        x, dy = (n, self.cin, self.H, self.W), (n, self.cout, ho, wo)
        return {"fwd": (x, self.w_shape()), "dgrad": (dy, self.w_shape()), "wgrad": (x, dy)}[self.kind]

    @property
    def axes(self):
        return {"fwd": (1, 0 if self.transposed else 1), "dgrad": (1, 1 if self.transposed else 0), "wgrad": (1, 1)}[self.kind]

    @property
    def pixels(self):
        return (True, self.kind == "wgrad")

    def reduction(self, ncu):
        """products per output: K of the forward pass / data gradient, pixels of the weight gradient"""
        ho, wo = self.out_hw()
        return {"fwd": self.k * self.k * self.cin, "dgrad": self.k * self.k * self.cout, "wgrad": self.batch(ncu) * ho * wo}[self.kind]

    def _conv(self, x, w, wrap_left=False):
        import torch.nn.functional as F
        if self.transposed:
            assert not wrap_left
            return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
        return conv_wrap_left(x, w, self.stride, self.pad) if wrap_left else F.conv2d(x, w, None, self.stride, self.pad)

    def op(self, a, b, wrap_left=False):
        """The case's bilinear map in float64: F.conv2d / F.conv_transpose2d, or their float64 autograd gradient.  wrap_left
        (plain convs with padding): the mutant of conv_wrap_left on the conv the kernel runs -- the layer's own forward, or for
        the stride-1 data gradient the conv of dy with the flipped, transposed filter."""
        a, b = a.double(), b.double()
        if self.kind == "fwd":
            return self._conv(a, b, wrap_left)
        if self.kind == "dgrad" and wrap_left:
            assert not self.transposed and self.stride == 1
            return conv_wrap_left(a, b.flip(2, 3).transpose(0, 1), 1, self.k - 1 - self.pad)
        assert not wrap_left
        if self.kind == "dgrad":
            x = torch.zeros(a.shape[0], self.cin, self.H, self.W, dtype=torch.float64, requires_grad=True)
            return torch.autograd.grad(self._conv(x, b), x, a)[0]
        w = torch.zeros(self.w_shape(), dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(self._conv(a, w), w, b)[0]


def conv_wrap_left(x, w, stride, pad):
    """F.conv2d whose left padding tap next to column 0 reads the last pixel of the previous row instead of zero (rows 1 and up):
    what a kernel computes that walks a flat run of pixels and misses a row wrap.  A mutant for the sensitivity checks."""
    import torch.nn.functional as F
    assert pad >= 1
    H, W = x.shape[2:]
    xp = F.pad(x, (pad, pad, pad, pad))
    xp[:, :, pad + 1:pad + H, pad - 1] = x[:, :, :H - 1, W - 1]
    return F.conv2d(xp, w, None, stride, 0)


def _every32(t, axis):
    idx = (torch.arange(t.shape[axis]) % 32 == 0)
    return idx.view([-1 if d == axis else 1 for d in range(t.dim())])


CONV_MUTANTS = ("drop_a_lo", "drop_b_lo", "lo32", "pair32", "wrap_left")


def conv_bf16x3(op, a, b, axes=(1, 1), pixels=(True, False), mutant=None):
    """The split arithmetic of a bilinear map op(A, B) (float64 in, float64 out) restated in float64: hi*hi + lo*hi + hi*lo of
    the bf16 halves of the fp32 operands a and b (every product exact, sums in float64); a cross product whose lo is zero
    everywhere is not evaluated.  mutant, each a wrong hi/lo pairing or tile placement:
      'drop_a_lo' / 'drop_b_lo'  the cross product with that operand's lo left out;
      'lo32'       lo dropped on every 32nd channel along `axes` (one lane of a 32-channel group of the split format);
      'pair32'     in each cross product, on every 32nd channel, lo meets the hi of the neighbouring pixel of the row: the
                   pixel-walking factor (`pixels`; lo where both walk pixels) is shifted by one along its last axis;
      'wrap_left'  op(..., wrap_left=True) for all three products (conv_wrap_left)."""
    assert mutant is None or mutant in CONV_MUTANTS
    (ah, al), (bh, bl) = bf16_split(a), bf16_split(b)
    kw = dict(wrap_left=True) if mutant == "wrap_left" else {}
    if mutant == "lo32":
        al, bl = al.masked_fill(_every32(al, axes[0]), 0.0), bl.masked_fill(_every32(bl, axes[1]), 0.0)

    def pair(lo, hi, lo_axis, hi_axis, lo_pixels, hi_pixels):
        if mutant != "pair32":
            return lo, hi
        assert lo_pixels or hi_pixels
        if lo_pixels:
            return torch.where(_every32(lo, lo_axis), lo.roll(1, -1), lo), hi
        return lo, torch.where(_every32(hi, hi_axis), hi.roll(1, -1), hi)

    y = op(ah, bh, **kw)
    if mutant != "drop_a_lo" and bool(al.any()):
        lo, hi = pair(al, bh, axes[0], axes[1], pixels[0], pixels[1])
        y = y + op(lo, hi, **kw)
    if mutant != "drop_b_lo" and bool(bl.any()):
        lo, hi = pair(bl, ah, axes[1], axes[0], pixels[1], pixels[0])
        y = y + op(hi, lo, **kw)
    return y


def exact_conditions(a, b, op, family):
    """The conditions under which bit equality is the specification, as a dict of booleans, with the float64 reference: hi + lo
    carries each operand, the operand without a lo term has none and the other has some, the sum of |products| of every output
    stays below 2^24 quanta of 2^-12, and the reference is its own fp32 rounding.  Conditions on the inputs, not measurements."""
    (ah, al), (bh, bl) = bf16_split_f32(a), bf16_split_f32(b)
    none, some = (bl, al) if family == "a_lo" else (al, bl)
    ref = op(a, b)
    return dict(carried=torch.equal(ah + al, a) and torch.equal(bh + bl, b),
                one_lo=float(none.abs().max()) == 0 and float(some.abs().max()) > 0,
                quanta=float(op(a.abs(), b.abs()).max()) * 4096 < 2 ** 24,
                ref_is_fp32=torch.equal(ref.float().double(), ref)), ref


def exact_forward_cases():
    """name -> ConvCase of the forward cases of tests/test_gpu_conv_exact.py: the ring and in-kernel-split rows of
    tests/test_gpu_conv_dispatch.CASES (one per instantiation, batches sized from the CU count as there) and the shapes whose
    128-pixel tiles start inside a row."""
    from tests.test_gpu_conv_dispatch import CASES, _RING, _F32
    cases = {}
    for name in ("ring64", "ring128", "ring_tall", "gen64_x3", "gen128_x3", "gen_small_cin_x3"):
        cin, cout, k, stride, pad, transposed, H, W, n_of, precision = CASES[name]
        assert precision == "bf16x3" and not transposed
        cases[name] = ConvCase("fwd", cin, cout, k, stride, pad, H, W, n_of, expect=_RING if name.startswith("ring") else _F32)
    # 16 x 24 map, 384 pixels: tiles start at row 5 column 8 and at row 10 column 16
    cases["ring_midrow"] = ConvCase("fwd", 64, 64, 1, 1, 0, 16, 24, 1, expect=_RING)
    # 16 x 24 output: both horizontal padding taps fall inside tiles, tiles 3 to 5 belong to image 1
    cases["ring_s2_midrow"] = ConvCase("fwd", 32, 64, 3, 2, 1, 32, 48, 2, midrow=True, expect=_RING)
    # one 128-pixel tile, K = 2304, 72 stages: many turns of the ring
    cases["ring_long_k"] = ConvCase("fwd", 256, 64, 3, 2, 1, 16, 32, 1, expect=_RING)
    return cases


def exact_dgrad_cases():
    """name -> ConvCase of the data-gradient cases, rectangular maps throughout.  lwg_conv2d_backward_data writes dx through
    64-channel tiles, so the layer's Cin is a multiple of 64: the gradient conv reduces the layer's Cout channels of dy to them."""
    from tests.test_gpu_conv_dispatch import _HALO, _RING
    return {
        # flipped-filter relayout mode 1; a 4 x 32 map is one halo tile
        "3x3_s1": ConvCase("dgrad", 64, 32, 3, 1, 1, 4, 32, 1, expect=_HALO),
        # the same at a width that is no multiple of 32: the ring, three tiles per image, padding taps inside tiles
        "3x3_s1_n3": ConvCase("dgrad", 64, 32, 3, 1, 1, 8, 48, 3, midrow=True, expect=_RING),
        "1x1": ConvCase("dgrad", 64, 128, 1, 1, 0, 16, 24, 1, expect=_RING),
        # four-phase transposed conv of dy (4 x 32) behind relayout mode 2
        "3x3_s2": ConvCase("dgrad", 64, 32, 3, 2, 1, 8, 64, 2, expect=_HALO),
        # stride-2 ring conv of dy (16 x 32) behind relayout mode 0
        "conv_transpose": ConvCase("dgrad", 64, 32, 3, 2, 1, 8, 16, 2, transposed=True, expect=_RING),
    }


def exact_wgrad_cases():
    """name -> ConvCase of the weight-gradient cases: every row of tests/test_gpu_wgrad_dispatch.CASES (expect = its table row),
    a transposed layer (the roles of x and dy swap), a batch larger than one, and the call whose bias gradient is checked."""
    from tests.test_gpu_wgrad_dispatch import CASES
    cases = {}
    for name, (cin, cout, k, stride, pad, N, H, W, precision, row) in CASES.items():
        cases[name] = ConvCase("wgrad", cin, cout, k, stride, pad, H, W, N, expect=row, precision=precision)
    cases["transposed"] = ConvCase("wgrad", 128, 64, 3, 2, 1, 16, 16, 1, transposed=True, expect=2)
    cases["row3 <64,64> batch 3"] = ConvCase("wgrad", 64, 64, 3, 1, 1, 8, 32, 3, expect=4)
    cases["bias fp32"] = ConvCase("wgrad", 64, 128, 3, 2, 1, 32, 32, 1, expect=0, precision="fp32")
    return cases


EXACT_KINDS = {"fwd": exact_forward_cases, "dgrad": exact_dgrad_cases, "wgrad": exact_wgrad_cases}


@functools.lru_cache(maxsize=None)
def exact_case_operands(kind, name, family, ncu=EXACT_NCU):
    """(A, B) of one exact case, seeded by (kind, name, family); family 'random': Gaussian activations, 0.05 x Gaussian second
    operand.  The 8-channel stem's weight gradient keeps channels 6 and 7 of x at zero.  Shared: treat as read-only."""
    case = EXACT_KINDS[kind]()[name]
    families = EXACT_FAMILIES + ("random",)
    seed = 100000 * sorted(EXACT_KINDS).index(kind) + 10 * sorted(EXACT_KINDS[kind]()).index(name) + families.index(family)
    g = torch.Generator().manual_seed(seed)
    sa, sb = case.shapes(ncu)
    if family == "random":
        a, b = torch.randn(sa, generator=g), torch.randn(sb, generator=g) * 0.05
    else:
        a, b = exact_operands(family, sa, sb, g)
    if case.cin == 8 and case.kind == "wgrad":
        a[:, 6:] = 0
    return a, b


# Order-independent exactness of bilinear sampling (csrc/sample.h and its consumers in warp.hip, train.hip, scatter.hip): pixel
# coordinates on a 1/8-texel lattice make every bilinear weight a multiple of 1/64 in [0, 1]; integer data in [-8, 8] then make every
# product w * v a multiple of 1/64 of magnitude <= 8, and where 8 * 64 * (longest contribution list) stays below 2^24 every partial
# sum in ANY order is an fp32 number: the float64 result rounded to fp32 is the specification, bit for bit, for the two forward
# kernels, the atomic scatter and the planned gather alike.  The grid itself is exact: align_corners=False with power-of-two H, W
# (g = (2 ix + 1) / W - 1), align_corners=True with power-of-two H - 1, W - 1 (g = 2 ix / (W - 1) - 1), so g and every intermediate
# of sample.h::unnormalize are fp32 numbers.  tests/test_gpu_sampling_exact.py holds the kernels to it; tests/test_sampling_cases.py
# proves the conditions and that a wrong unnormalise, floor, validity rule or pitch cannot meet it.
class SampleCase(object):
    """One sampling problem: source (xn, C, H, W) with xn in {1, n}, grid (n, Ho, Wo, 2).  kind: 'lattice' (uniform on the lattice
    over [-2, W + 1] x [-2, H + 1]), 'named' (hand-set border coordinates, then wild values), 'thresholds_exact' /
    'thresholds_ordered' (list lengths on the plan's thresholds), 'crowded' (every texel queued)."""

    def __init__(self, kind, align, H, W, xn, n, Ho, Wo, seed):
        self.kind, self.align, self.H, self.W, self.xn, self.n, self.Ho, self.Wo, self.seed = kind, align, H, W, xn, n, Ho, Wo, seed


SAMPLE_SIZES = {False: [(8, 16), (16, 4), (1, 2)], True: [(5, 9), (17, 3), (2, 2)]}
SAMPLE_THRESHOLDS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)   # 13 347 pixels: kHeavy, bitonic sizes, kSortMax
SAMPLE_BLOCKS = [(3 * by, 3 * bx) for by in range(3) for bx in range(5)]              # north-west texels of fifteen 2 x 2 blocks
SAMPLE_WILD = (float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 3e38, -3e38)
SAMPLE_POINT = (20.375, 11.625)       # (ix, iy) that the crowded case aims an 80 x 80 patch of image 1 at
SAMPLE_MUTANTS = ("swap_hw", "other_align", "trunc", "drop_partial", "border_clamp", "last_col", "out_pitch", "first_image_only")


def _sample_cases():
    cases, seed = {}, 0
    for align in (False, True):
        for H, W in SAMPLE_SIZES[align]:
            for xn in (1, 3):
                seed += 1
                cases["lattice align %d %dx%d %s" % (align, H, W, "shared" if xn == 1 else "per image")] = \
                    SampleCase("lattice", align, H, W, xn, 3, 24, 40, seed)
    # one image on the thresholds cases' dimensions: a second grid for the same plan buffer, and more than one block of pixels
    cases["lattice align 0 8x16 one image 96x160"] = SampleCase("lattice", False, 8, 16, 1, 1, 96, 160, 40)
    cases["named align 0"] = SampleCase("named", False, 4, 8, 2, 2, 9, 16, 50)
    cases["named align 1"] = SampleCase("named", True, 5, 9, 2, 2, 9, 16, 51)
    cases["thresholds exact"] = SampleCase("thresholds_exact", False, 8, 16, 1, 1, 96, 160, 60)
    cases["thresholds ordered"] = SampleCase("thresholds_ordered", False, 8, 16, 1, 1, 96, 160, 61)
    cases["thresholds ordered n3"] = SampleCase("thresholds_ordered", False, 8, 16, 1, 3, 96, 160, 62)
    cases["crowded"] = SampleCase("crowded", True, 33, 65, 1, 2, 192, 192, 7)
    return cases


SAMPLE_CASES = _sample_cases()


def named_coordinates(size):
    """the border coordinates of the 'named' cases along an axis of `size` texels"""
    return [-1.5, -1.0, -0.5, -0.125, 0.0, size - 1.0, size - 0.875, size - 0.5, float(size)]


def _lattice(g, shape, lo, hi):
    """float64 multiples of 1/8, uniform on [lo, hi]"""
    return torch.randint(int(8 * lo), int(8 * hi) + 1, shape, generator=g).double() / 8


def sample_pixel_coordinates(case):
    """(ix, iy, sentinel) of a case: float64 pixel coordinates (n, Ho, Wo) on the 1/8 lattice and the mask of the pixels that carry
    the -2 sentinel (or, in a 'named' case, a wild value) instead."""
    g = torch.Generator().manual_seed(case.seed)
    n, Ho, Wo, H, W = case.n, case.Ho, case.Wo, case.H, case.W
    shape, P = (n, Ho, Wo), n * Ho * Wo
    sentinel = torch.zeros(P, dtype=torch.bool)
    if case.kind == "lattice":
        ix, iy = _lattice(g, shape, -2, W + 1), _lattice(g, shape, -2, H + 1)
    elif case.kind == "crowded":
        ix, iy = _lattice(g, shape, 0, W - 1), _lattice(g, shape, 0, H - 1)
        ix[1, 50:130, 60:140], iy[1, 50:130, 60:140] = SAMPLE_POINT
    elif case.kind == "named":
        xs, ys = named_coordinates(W), named_coordinates(H)
        ix, iy = torch.full((n, Ho * Wo), 2.5, dtype=torch.float64), torch.full((n, Ho * Wo), 1.5, dtype=torch.float64)
        ix[:, :81], iy[:, :81] = torch.tensor(xs * 9, dtype=torch.float64), torch.tensor(ys, dtype=torch.float64).repeat_interleave(9)
        sentinel = sentinel.view(n, -1)
        sentinel[:, 81:] = True
        ix[1], iy[1], sentinel[1] = ix[0].flip(0), iy[0].flip(0), sentinel[0].flip(0)   # image 1: image 0's pixels in reverse order
    else:
        assert case.kind in ("thresholds_exact", "thresholds_ordered") and not case.align
        perm = torch.randperm(P, generator=g)
        ix, iy = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
        sentinel[:] = True
        pos = 0
        for (ty, tx), K in zip(SAMPLE_BLOCKS, SAMPLE_THRESHOLDS):   # the fifteenth block stays empty
            pix = perm[pos:pos + K]
            pos += K
            inside = _lattice(g, (2, K), 0.125, 0.875) if case.kind == "thresholds_exact" else torch.zeros(2, K, dtype=torch.float64)
            ix[pix], iy[pix], sentinel[pix] = tx + inside[0], ty + inside[1], False
    return ix.view(shape), iy.view(shape), sentinel.view(shape)


@functools.lru_cache(maxsize=None)
def sample_grid(case):
    """The fp32 grid (n, Ho, Wo, 2) of a case, from its pixel coordinates: exact in fp32, as is every intermediate of
    sample.h::unnormalize.  Sentinel pixels hold -2; in a 'named' case the pixels after the 81 hand-set ones hold SAMPLE_WILD in x
    only (y inside the image), in y only and in both; image 1 holds image 0's pixels in reverse order.  Shared: read-only."""
    ix, iy, sentinel = sample_pixel_coordinates(case)
    norm = (lambda v, s: 2 * v / (s - 1) - 1) if case.align else (lambda v, s: (2 * v + 1) / s - 1)
    g64 = torch.stack([norm(ix, case.W), norm(iy, case.H)], dim=-1)
    grid = g64.float()
    assert torch.equal(grid.double(), g64)
    if case.kind == "named":
        wild = torch.tensor(SAMPLE_WILD)
        tail = grid[0].view(-1, 2)[81:]
        tail[0:7, 0] = wild
        tail[7:14, 1] = wild
        tail[14:63, 0], tail[14:63, 1] = wild.repeat(7), wild.repeat_interleave(7)
        grid[1] = grid[0].flip(0, 1)
    else:
        grid[sentinel] = -2.0
    return grid


def sample_tame(grid):
    """(grid with every wild entry -- NaN, infinite or of magnitude >= 1e30 -- replaced by -3, mask (n, Ho, Wo) of the pixels that
    had one): the reference of the 'named' cases is computed from this grid."""
    wild = ~torch.isfinite(grid) | (grid.abs() >= 1e30)
    return torch.where(wild, torch.full_like(grid, -3.0), grid), wild.any(-1)


@functools.lru_cache(maxsize=None)
def sample_data(case, C):
    """(x (xn, C, H, W), dy (n, C, Ho, Wo)): fp32 integers in [-8, 8], seeded by the case and C.  Shared: read-only."""
    g = torch.Generator().manual_seed(1000 * case.seed + C)
    draw = lambda *shape: torch.randint(-8, 9, shape, generator=g).float()
    return draw(case.xn, C, case.H, case.W), draw(case.n, C, case.Ho, case.Wo)


@functools.lru_cache(maxsize=None)
def sample_ordered_dy(case, C=4):
    """dy (n, C, Ho, Wo) of the 'ordered' family: normal * 2^k, k uniform in [-12, 12] -- an fp32 sum of these depends on its order"""
    g = torch.Generator().manual_seed(1000 * case.seed + 500 + C)
    shape = (case.n, C, case.Ho, case.Wo)
    return torch.randn(shape, generator=g) * torch.pow(2.0, torch.randint(-12, 13, shape, generator=g).float())


class SampleTaps(object):
    """tex (n, Ho, Wo, 4): flat texel index into (xn, H, W) of the taps nw, ne, sw, se, or -1 outside the image; w: their float64
    weights; valid: tex >= 0; counts (xn * H * W): contributions per texel, zero-weight valid taps included."""

    def __init__(self, tex, w, valid, counts):
        self.tex, self.w, self.valid, self.counts = tex, w, valid, counts


def _sample_taps(grid, H, W, align, xn, mutant=None):
    assert mutant is None or mutant in SAMPLE_MUTANTS
    g = grid.double()
    n, Ho, Wo = g.shape[:3]
    al = bool(align) != (mutant == "other_align")
    sx, sy = (H, W) if mutant == "swap_hw" else (W, H)
    unn = (lambda v, s: (v + 1) / 2 * (s - 1)) if al else (lambda v, s: ((v + 1) * s - 1) / 2)
    ix, iy = unn(g[..., 0], sx), unn(g[..., 1], sy)
    # sample.h's clamps: wild coordinates become -4 or size + 4 and sample nothing
    lo = torch.full_like(ix, -4.0)
    ix, iy = torch.where(ix > -4, ix, lo).clamp(max=W + 4.0), torch.where(iy > -4, iy, lo).clamp(max=H + 4.0)
    rnd = torch.trunc if mutant == "trunc" else torch.floor
    fx, fy = rnd(ix), rnd(iy)
    ex, ey = fx + 1, fy + 1
    w = torch.stack([(ex - ix) * (ey - iy), (ix - fx) * (ey - iy), (ex - ix) * (iy - fy), (ix - fx) * (iy - fy)], dim=-1)
    x0, y0 = fx.long(), fy.long()
    xs, ys = torch.stack([x0, x0 + 1, x0, x0 + 1], dim=-1), torch.stack([y0, y0, y0 + 1, y0 + 1], dim=-1)
    valid = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    if mutant == "last_col":
        valid[..., 1::2] &= xs[..., 1::2] < W - 1
    if mutant == "border_clamp":
        xs, ys, valid = xs.clamp(0, W - 1), ys.clamp(0, H - 1), torch.ones_like(valid)
    if mutant == "drop_partial":
        valid = valid & valid.all(-1, keepdim=True)
    flat = (ys * Wo + xs) % (H * W) if mutant == "out_pitch" else ys * W + xs
    base = (torch.arange(n) * (H * W) if xn > 1 else torch.zeros(n, dtype=torch.long)).view(n, 1, 1, 1)
    tex = torch.where(valid, base + flat, torch.full_like(flat, -1))
    return SampleTaps(tex, w, valid, torch.bincount(tex[valid], minlength=xn * H * W))


def sample_taps(grid, H, W, align, xn):
    """The four tap texels, weights and validity of every pixel of `grid` on an (xn, H, W) source, in float64 by sample.h's
    formulas, and the per-texel contribution counts (a valid tap of weight 0 counts, as in gs_plan_count_kernel)."""
    return _sample_taps(grid, H, W, align, xn)


def grid_sample_restated(x, grid, align, mutant=None):
    """F.grid_sample(x, grid, bilinear, zeros) restated in float64 from sample_taps: x (xn, C, H, W), xn in {1, n} -> (n, C, Ho, Wo).
    mutant, each a way a kernel goes wrong:
      'swap_hw'       x unnormalised with H, y with W;
      'other_align'   the other mode's unnormalise;
      'trunc'         (int) truncation instead of floor;
      'drop_partial'  a pixel with any tap outside samples nothing;
      'border_clamp'  outside taps read the edge texel;
      'last_col'      east taps valid only for x0 + 1 < W - 1;
      'out_pitch'     source rows addressed with Wo (wrapped into the image);
      'first_image_only'  (adjoint, shared source) only image 0's gradient arrives."""
    assert mutant != "first_image_only"
    xn, C, H, W = x.shape
    t = _sample_taps(grid, H, W, align, xn, mutant)
    xf = x.double().permute(0, 2, 3, 1).reshape(xn * H * W, C)
    y = torch.zeros(t.tex[..., 0].numel(), C, dtype=torch.float64)
    for k in range(4):
        v, idx = t.valid[..., k].reshape(-1, 1), t.tex[..., k].reshape(-1).clamp(min=0)
        y = y + torch.where(v, t.w[..., k].reshape(-1, 1) * xf[idx], torch.zeros_like(y))
    return y.view(tuple(grid.shape[:3]) + (C,)).permute(0, 3, 1, 2)


def grid_sample_adjoint_restated(dy, grid, x_shape, align, mutant=None):
    """The input gradient of grid_sample_restated: dy (n, C, Ho, Wo) -> dx of x_shape (xn, C, H, W), float64."""
    xn, C, H, W = x_shape
    t = _sample_taps(grid, H, W, align, xn, None if mutant == "first_image_only" else mutant)
    dyf = dy.double().permute(0, 2, 3, 1).reshape(-1, C).clone()
    if mutant == "first_image_only":
        assert xn == 1
        dyf[dy.shape[2] * dy.shape[3]:] = 0
    dx = torch.zeros(xn * H * W, C, dtype=torch.float64)
    for k in range(4):
        v = t.valid[..., k].reshape(-1)
        dx.index_add_(0, t.tex[..., k].reshape(-1)[v], (t.w[..., k].reshape(-1, 1) * dyf)[v])
    return dx.view(xn, H, W, C).permute(0, 3, 1, 2)


def grid_sample_float64(x, grid, align, dy):
    """(y, dx): F.grid_sample and its input gradient for the cotangent dy, float64 on the CPU -- the reference"""
    import torch.nn.functional as F
    xr = x.double().clone().requires_grad_(True)
    n = grid.shape[0]
    y = F.grid_sample(xr.expand(n, -1, -1, -1) if x.shape[0] == 1 and n > 1 else xr, grid.double(), mode="bilinear",
                      padding_mode="zeros", align_corners=bool(align))
    y.backward(dy.double())
    return y.detach(), xr.grad


def sample_case_mutants(case):
    """The mutants that must change a case's result, from its geometry: a square source hides swap_hw; a one-row source or
    Wo == W hides out_pitch; coordinates inside the image hide trunc; the threshold blocks have every tap inside and never reach
    the last column, nor does an east tap of the named coordinates; in the crowded case an outside tap has weight 0 (ix = W - 1 exactly), which border_clamp keeps at nothing."""
    inside = case.kind in ("thresholds_exact", "thresholds_ordered", "crowded")
    m = ["other_align"]
    if case.H != case.W:
        m.append("swap_hw")
    if not inside:
        m.append("trunc")
    if not case.kind.startswith("thresholds"):
        m.append("drop_partial")
    if case.kind in ("lattice", "crowded"):   # no named coordinate has x0 = W - 2
        m.append("last_col")
    if case.kind != "crowded":
        m.append("border_clamp")
    if case.H > 1 and case.Wo != case.W:
        m.append("out_pitch")
    if case.xn == 1 and case.n > 1:
        m.append("first_image_only")
    return m


def sample_threshold_lists(case, taps):
    """[(K, texel, pixels)] of a thresholds case: the aimed (north-west) texel of every used block and the flat indices of the
    pixels aiming at it, ascending -- the key order of its contribution list."""
    nw = taps.tex[..., 0].reshape(-1)
    return [(K, ty * case.W + tx, torch.nonzero(nw == ty * case.W + tx).reshape(-1))
            for (ty, tx), K in zip(SAMPLE_BLOCKS, SAMPLE_THRESHOLDS)]


def ordered_running_sums(dy, lists, T, reverse=False):
    """dx (T, C) fp32 of the 'ordered' family: the aimed texel of each list gets the numpy float32 running sum of its pixels' dy
    (n, C, Ho, Wo) in ascending pixel index -- what acc = fma(1, dy, acc) in key order computes; every other texel 0."""
    rows = dy.permute(0, 2, 3, 1).reshape(-1, dy.shape[1]).numpy()
    dx = np.zeros((T, rows.shape[1]), dtype=np.float32)
    for _, tex, pixels in lists:
        acc = np.zeros(rows.shape[1], dtype=np.float32)
        for p in (reversed(pixels.tolist()) if reverse else pixels.tolist()):
            acc = acc + rows[p]
        dx[tex] = acc
    return torch.from_numpy(dx)


SAMPLE_FLOW_SIZES = [(17, 9), (9, 5), (65, 33), (33, 17), (3, 2), (1, 1)]


@functools.lru_cache(maxsize=None)
def sample_flow():
    """A dyadic flow (2, 33, 17, 2): multiples of 1/64 in [-2, 1] with a patch of the -2 sentinel.  Every scale 32 / (h - 1),
    16 / (w - 1) of SAMPLE_FLOW_SIZES is a power of two, so the interpolation weights are dyadic and fp32 is exact."""
    g = torch.Generator().manual_seed(33)
    T = torch.randint(-128, 65, (2, 33, 17, 2), generator=g).float() / 64
    T[0, 5:12, 3:9] = -2.0
    return T


def resize_flow_float64(T, h, w):
    """F.interpolate(bilinear, align_corners=True) of a flow (bs, H, W, 2) to (bs, h, w, 2), float64"""
    import torch.nn.functional as F
    return F.interpolate(T.double().permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# The inference path's norm chain link by link (lwg_norm_conv_forward, lwg_norm_finalize, lwg_norm_apply; include/lwg.h states
# which 128 pixels a partial covers and the conditioning contract of finalize).  tests/test_norm_chain_cases.py proves on the
# CPU the conditions the exact expectations rest on and that the listed mutants miss them; tests/test_gpu_norm_chain.py holds
# the kernels to them.
IN_EPS = float(np.float32(1e-5))   # kInEps widened to double, as in_finalize_kernel widens it

# name -> (Cin, Cout, k, stride, pad, transposed, H, W, N(ncu), precision, bn, partition, kernel name the profiler must show)
_HALO_K, _RING_K, _DMA_K, _F32_K = "conv3x3_halo_bf16x3", "conv_igemm_bf16x3", "conv_igemm_dma_f32", "conv_igemm_f32"
NORM_STAT_CASES = {
    "halo64": (32, 64, 3, 1, 1, False, 4, 32, lambda ncu: 1, "bf16x3", 64, "blocks", _HALO_K + "<64,1,2,3,32,128,0,false>"),
    # two block columns, six blocks per image, blocks that are no runs of consecutive pixels
    "halo64_8x64": (32, 64, 3, 1, 1, False, 8, 64, lambda ncu: 3, "bf16x3", 64, "blocks", _HALO_K + "<64,1,2,3,32,128,0,false>"),
    "halo128": (32, 128, 3, 1, 1, False, 12, 32, lambda ncu: -(-ncu // 3), "bf16x3", 128, "blocks", _HALO_K + "<128,2,2,4,32,128,0,false>"),
    "halo_tall": (32, 128, 3, 1, 1, False, 8, 32, lambda ncu: ncu, "bf16x3", 128, "blocks", _HALO_K + "<128,2,2,4,32,256,0,false>"),
    "ct_narrow": (32, 64, 3, 2, 1, True, 4, 32, lambda ncu: 1, "bf16x3", 0, "blocks", _HALO_K + "<64,1,2,3,32,128,1,false>"),
    "ct_wide": (32, 128, 3, 2, 1, True, 16, 32, lambda ncu: -(-ncu // 4), "bf16x3", 0, "blocks", _HALO_K + "<128,2,2,4,32,128,1,false>"),
    "ring64": (32, 64, 1, 1, 0, False, 4, 32, lambda ncu: 1, "bf16x3", 64, "runs", _RING_K + "<64,1,2,3,0,128>"),
    "ring128": (32, 512, 3, 2, 1, False, 24, 64, lambda ncu: 44, "bf16x3", 128, "runs", _RING_K + "<128,2,2,4,0,128>"),
    "ring_tall": (32, 128, 1, 1, 0, False, 8, 32, lambda ncu: ncu, "bf16x3", 128, "runs", _RING_K + "<128,2,2,3,0,256>"),
    # a map wider than 128 on the ring: a run is part of one row (the TC2 > 0 epilogue of igemm_epilogue is instantiated by no kernel)
    "ring_wide_map": (32, 64, 1, 1, 0, False, 4, 192, lambda ncu: 2, "bf16x3", 64, "runs", _RING_K + "<64,1,2,3,0,128>"),
    # exact fp32, non-general kernels
    "dma32": (32, 64, 3, 1, 1, False, 8, 16, lambda ncu: 1, "fp32", 32, "runs", _DMA_K + "<32,1,1,0,3>"),
    "dma64": (32, 64, 3, 1, 1, False, 8, 16, lambda ncu: 1, "fp32", 64, "runs", _DMA_K + "<64,1,2,0,3>"),
    "dma128": (32, 128, 3, 1, 1, False, 8, 16, lambda ncu: 1, "fp32", 128, "runs", _DMA_K + "<128,2,2,0,3>"),
    "reg128": (32, 128, 1, 1, 0, False, 4, 32, lambda ncu: ncu + 1, "fp32", 128, "runs", _F32_K + "<128,2,2,false,0,false,false>"),
    "small_cin": (8, 64, 7, 1, 3, False, 16, 16, lambda ncu: 1, "fp32", 64, "runs", _F32_K + "<64,1,2,true,0,false,false>"),
    "ct_fused_f32": (32, 64, 3, 2, 1, True, 4, 32, lambda ncu: 1, "fp32", 0, "runs", _DMA_K + "<64,1,2,0,3>"),
}
NORM_F32_CASES = ("dma32", "dma64", "dma128", "reg128", "small_cin", "ct_fused_f32")


def norm_case(name, ncu=EXACT_NCU):
    """ConvCase of a NORM_STAT_CASES row with its batch fixed, plus .bn, .partition, .kernel, .name"""
    cin, cout, k, stride, pad, transposed, H, W, n_of, precision, bn, partition, kernel = NORM_STAT_CASES[name]
    c = ConvCase("fwd", cin, cout, k, stride, pad, H, W, n_of(ncu), transposed=transposed, precision=precision)
    c.bn, c.partition, c.kernel, c.name = bn, partition, kernel, name
    return c


def norm_grid(case):
    """(nphase, Hm, Wm): the phase grid per image whose pixels the partials tile"""
    return (4, case.H, case.W) if case.transposed else (1,) + case.out_hw()


def _ct_taps(co):
    """transposed conv: the (ky, kx) of output channel co's tap per output parity class p = 2 py + px.  Row 2i + py is fed by
    ky = 1 (py 0: input row i) or by ky in {2 (input row i), 0 (input row i + 1)} (py 1); columns alike."""
    odd_y, odd_x = ((2, 0)[co & 1], (2, 0)[(co >> 1) & 1]) if co >= 2 else (2, 2)   # channels 0, 1 never read past the border
    return [(1, 1), (1, odd_x), (odd_y, 1), (odd_y, odd_x)]


def onehot_stat_operands(case, seed=0):
    """The exact statistics family.  x (N,H,W,Cin) NHWC: integers in [-2, 2], every input channel with its own distribution --
    channel 0 all zero, 1 constant per image, 2 only +-2, 3 rows alternating {1, 2} / {-2, -1} (group means far apart), the others
    uniform on a subset of {-2..2} that depends on the channel; images differ.  w (PyTorch layout) one-hot: output channel co takes
    input channel co % Cin at a tap that varies with co (the centre for channels 0 and 1, which thus stay all-zero / constant --
    per phase for a transposed conv),
    value 2^e(co), e in [-6, 6]; a transposed conv gets one tap per output parity class (_ct_taps), the sign alternating with the
    class.  -> (x, w, ci (Cout), e (Cout))."""
    g = torch.Generator().manual_seed(7000 + seed)
    N, H, W, cin, cout, k = case.N, case.H, case.W, case.cin, case.cout, case.k
    x = torch.zeros(N, H, W, cin)
    for c in range(cin):
        if c == 0:
            continue
        if c == 1:
            x[..., c] = torch.tensor([2.0, -1.0, 1.0, -2.0])[torch.arange(N) % 4].view(N, 1, 1)
        elif c == 2:
            x[..., c] = torch.randint(0, 2, (N, H, W), generator=g).float() * 4 - 2
        elif c == 3:
            v = torch.randint(1, 3, (N, H, W), generator=g).float()
            x[..., c] = torch.where((torch.arange(H) % 2 == 0).view(1, H, 1), v, -v)
        else:
            lo, hi = -2 + (c % 3), 2 - ((c // 3) % 2)
            x[..., c] = torch.randint(lo, hi + 1, (N, H, W), generator=g).float()
    co = torch.arange(cout)
    ci = co % cin
    e = (co * 7) % 13 - 6
    w = torch.zeros(case.w_shape())
    for o in range(cout):
        s = 2.0 ** int(e[o])
        if case.transposed:
            for p, (ky, kx) in enumerate(_ct_taps(o)):
                w[ci[o], o, ky, kx] = s if p in (0, 3) else -s
        else:
            tap = (k * k) // 2 if o < 2 else (o // cin + o) % (k * k)
            w[o, ci[o], tap // k, tap % k] = s
    return x, w, ci, e


def onehot_conv_reference(case, x, w):
    """The raw output (N,Ho,Wo,Cout) float64 of a one-hot weight tensor as shifted, scaled copies of x's channels: no conv."""
    N, H, W, cin, cout, k = case.N, case.H, case.W, case.cin, case.cout, case.k
    Ho, Wo = case.out_hw()
    y = torch.zeros(N, Ho, Wo, cout, dtype=torch.float64)
    xd = x.double()
    if case.transposed:
        xp = torch.nn.functional.pad(xd, (0, 0, 0, 1, 0, 1))   # one zero row / column behind the image
        wt = w.permute(1, 0, 2, 3)                              # (Cout, Cin, 3, 3)
        for ky in range(3):
            for kx in range(3):
                nz = wt[:, :, ky, kx].abs().sum(1).nonzero().flatten()
                if not len(nz):
                    continue
                ci = wt[nz, :, ky, kx].abs().argmax(1)
                val = wt[nz, ci, ky, kx].double()
                py, dy = (0, 0) if ky == 1 else (1, 1 if ky == 0 else 0)
                px, dx = (0, 0) if kx == 1 else (1, 1 if kx == 0 else 0)
                y[:, py::2, px::2, nz] = xp[:, dy:dy + H, dx:dx + W][..., ci] * val
        return y
    p, s = case.pad, case.stride
    xp = torch.nn.functional.pad(xd, (0, 0, p, p, p, p))
    for kh in range(k):
        for kw in range(k):
            nz = w[:, :, kh, kw].abs().sum(1).nonzero().flatten()
            if not len(nz):
                continue
            ci = w[nz, :, kh, kw].abs().argmax(1)
            y[..., nz] = xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s][..., ci] * w[nz, ci, kh, kw].double()
    return y


def conv_reference_nhwc(case, x, w):
    """float64 F.conv2d / F.conv_transpose2d of NHWC x -> NHWC y"""
    return case.op(x.permute(0, 3, 1, 2), w).permute(0, 2, 3, 1).contiguous()


def phase_views(case, y):
    """raw output (N,Ho,Wo,C) -> (nphase, N, Hm, Wm, C): the phase grids (phase p = 2 py + px of a transposed conv holds the
    output pixels (2i + py, 2j + px))"""
    if not case.transposed:
        return y.unsqueeze(0)
    return torch.stack([y[:, py::2, px::2] for py in (0, 1) for px in (0, 1)])


STAT_MUTANTS = ("other_partition", "swap_phases", "image0_tiles", "channel32", "channel64", "tall_stride")


def stat_partition(partition, N, Hm, Wm):
    """(mtiles, 128) flat pixel indices into (N, Hm, Wm) of every partial, as include/lwg.h documents them: 'runs' = 128 consecutive
    pixels, images in order; 'blocks' = 4 x 32 blocks numbered row-major within the image."""
    idx = torch.arange(N * Hm * Wm)
    if partition == "runs":
        return idx.view(-1, 128)
    assert partition == "blocks" and Hm % 4 == 0 and Wm % 32 == 0
    return idx.view(N, Hm // 4, 4, Wm // 32, 32).permute(0, 1, 3, 2, 4).reshape(-1, 128)


def stat_expected(case, y, mutant=None):
    """float64 (mean, M2), each (nphase, mtiles, C), of the raw output y (N,Ho,Wo,C) under the documented partition.  mutant:
      'other_partition'  runs where blocks are documented and the reverse;
      'swap_phases'      phases 1 and 2 exchanged;
      'image0_tiles'     image n reads image 0's pixels;
      'channel32' / 'channel64'  channel c holds channel (c + 32 / 64) % C;
      'tall_stride'      an 8 x 32 tile writes its lower block one block row too far (NaN where nothing lands)."""
    assert mutant is None or mutant in STAT_MUTANTS
    nphase, Hm, Wm = norm_grid(case)
    N, C = y.shape[0], y.shape[-1]
    part = case.partition
    if mutant == "other_partition":
        part = "runs" if part == "blocks" else "blocks"
    idx = stat_partition(part, N, Hm, Wm)
    if mutant == "image0_tiles":
        idx = idx % (Hm * Wm)
    v = phase_views(case, y.double()).reshape(nphase, N * Hm * Wm, C)[:, idx]   # (nphase, mtiles, 128, C)
    mean = v.mean(2)
    m2 = ((v - mean[:, :, None]) ** 2).sum(2)
    if mutant == "swap_phases":
        assert nphase == 4
        mean, m2 = mean[[0, 2, 1, 3]], m2[[0, 2, 1, 3]]
    if mutant in ("channel32", "channel64"):
        sh = (torch.arange(C) + int(mutant[7:])) % C
        mean, m2 = mean[..., sh], m2[..., sh]
    if mutant == "tall_stride":
        bx, by = Wm // 32, Hm // 4
        assert part == "blocks" and by % 2 == 0
        out = []
        for t in (mean, m2):
            t = t.view(nphase, N, by, bx, C)
            moved = torch.full_like(t, float("nan"))
            moved[:, :, 0::2] = t[:, :, 0::2]
            moved[:, :, 2::2] = t[:, :, 1:-1:2]          # lower blocks land on the next tile's upper block
            out.append(moved.view(nphase, -1, C))
        mean, m2 = out
    return mean, m2


def two_level_stats_f32(v, rng=None):
    """The epilogues' reduction restated in numpy float32, v (..., 128) float32 -> (mean, M2) float32: four groups of 32 -- sum,
    division by 32, squared deviations from the group mean -- combined by Chan's formula with the factor 32, every operation a
    separately rounded fp32 one, each sum SEQUENTIAL (the worst order a kernel could choose).  rng: shuffle the 128 values first."""
    v = np.asarray(v, dtype=np.float32)
    if rng is not None:
        v = np.take_along_axis(v, np.argsort(rng.random(v.shape), axis=-1), axis=-1)
    gsh = v.reshape(v.shape[:-1] + (4, 32))
    s = np.zeros(gsh.shape[:-1], dtype=np.float32)
    for i in range(32):
        s = s + gsh[..., i]
    mu = s * np.float32(1.0 / 32.0)
    q = np.zeros_like(s)
    for i in range(32):
        d = gsh[..., i] - mu
        q = q + d * d
    mean = np.zeros(s.shape[:-1], dtype=np.float32)
    for w in range(4):
        mean = mean + mu[..., w]
    mean = mean * np.float32(0.25)
    m2 = np.zeros_like(mean)
    for w in range(4):
        d = mu[..., w] - mean
        m2 = m2 + (q[..., w] + np.float32(32.0) * d * d)
    return mean, m2


# Random statistics: the restatement above against float64 on the same fp32 values, over norm_random_tiles() -- per family the
# worst |mean - ref| / max |y| and |M2 - ref| / max ref M2 (the convention of STEM_M2_REL), measured by tests/test_norm_chain_cases.py,
# which prints them and asserts that none exceeds the figures below.  The GPU assertions use 4 x them (NORM_STAT_REL); the raw
# output of Gaussian operands is held to the 'offset' figures (its tile means wander by a few sigma / sqrt(128) at most).
# family -> (mean figure, M2 figure) as measured (8.29e-9 / 1.74e-7, 4.49e-8 / 1.43e-7, 1.31e-7 / 4.67e-5).  At |mean| / std = 2^10 the
# fp32 group means carry an error of ~2^-14 std, which the between-group term of Chan's formula turns into ~5e-5 of M2.
NORM_STAT_MEASURED = {"gauss": (9e-9, 1.8e-7), "offset": (4.6e-8, 1.8e-7), "ratio1024": (1.4e-7, 4.8e-5)}
NORM_STAT_REL = {k: (4 * v[0], 4 * v[1]) for k, v in NORM_STAT_MEASURED.items()}
NORM_RANDOM_FAMILIES = ("gauss", "offset", "ratio1024")


def norm_random_tiles(family, tiles=256, C=16, seed=0):
    """(tiles, C, 128) float32 samples of a raw output: 'gauss' N(0, s_c^2); 'offset' mean of a few sigma per channel;
    'ratio1024' |mean| / std = 2^10 in every channel."""
    g = torch.Generator().manual_seed(8000 + seed + NORM_RANDOM_FAMILIES.index(family))
    z = torch.randn(tiles, C, 128, generator=g, dtype=torch.float64)
    s = torch.pow(2.0, torch.randint(-4, 5, (1, C, 1), generator=g).double())
    m = {"gauss": 0.0, "offset": torch.randn(1, C, 1, generator=g, dtype=torch.float64) * 3, "ratio1024": 1024.0}[family]
    return ((z + m) * s).float()


def stat_errors(mean, m2, ref_mean, ref_m2, ymax):
    """(mean error / max |y|, M2 error / max ref M2): the two figures NORM_STAT_REL bounds"""
    return (float((torch.as_tensor(mean).double() - ref_mean).abs().max()) / ymax,
            float((torch.as_tensor(m2).double() - ref_m2).abs().max()) / float(ref_m2.max()))


# ---- finalize
def finalize_reference(mean, m2, N, gamma, beta, exact=False):
    """scale_shift (N, C, 2) float64 BEFORE the final rounding, from partials (nphase, mtiles, C) given as float64 (the fp32
    partials widened): Chan's combination, biased variance over the image's nphase * tiles * 128 samples, eps = IN_EPS.
    exact: the combination in exact rationals (fractions) -- for ill-conditioned synthetic partials; otherwise float64 in the
    cancellation-free form sum M2 + 128 sum (mean_t - mean)^2."""
    nphase, mtiles, C = mean.shape
    tiles = mtiles // N
    mu = mean.view(nphase, N, tiles, C).permute(1, 3, 0, 2).reshape(N, C, -1).double()
    q = m2.view(nphase, N, tiles, C).permute(1, 3, 0, 2).reshape(N, C, -1).double()
    cnt = mu.shape[-1]
    if exact:
        from fractions import Fraction
        gm = torch.zeros(N, C, dtype=torch.float64)
        var = torch.zeros(N, C, dtype=torch.float64)
        for n in range(N):
            for c in range(C):
                ms = [Fraction(v) for v in mu[n, c].tolist()]
                qs = [Fraction(v) for v in q[n, c].tolist()]
                m = sum(ms) / cnt
                gm[n, c] = float(m)
                var[n, c] = float((sum(qs) + 128 * sum((a - m) ** 2 for a in ms)) / (cnt * 128))
    else:
        gm = mu.mean(-1)
        var = (q.sum(-1) + 128 * ((mu - gm[..., None]) ** 2).sum(-1)) / (cnt * 128)
    inv = 1.0 / torch.sqrt(var + IN_EPS)
    ga, be = gamma.double().view(1, C), beta.double().view(1, C)
    return torch.stack([ga * inv, be - gm * ga * inv], dim=-1)


def finalize_emulated(mean, m2, N, gamma, beta):
    """in_finalize_kernel's double arithmetic restated in numpy: 16 slices walk the tiles t = slice, slice + 16, ... of each phase
    in turn, the slices are added in order, between = sum mean^2 - cnt mean^2 (clamped at 0) -> (N, C, 2) float32."""
    nphase, mtiles, C = mean.shape
    tiles = mtiles // N
    mu = mean.view(nphase, N, tiles, C).double().numpy()
    q = m2.view(nphase, N, tiles, C).double().numpy()
    sm, sq, s2 = (np.zeros((16, N, C)) for _ in range(3))
    for p in range(nphase):
        for t in range(tiles):
            sm[t % 16] += mu[p, :, t]
            sq[t % 16] += mu[p, :, t] * mu[p, :, t]
            s2[t % 16] += q[p, :, t]
    tot = [np.zeros((N, C)) for _ in range(3)]
    for k in range(16):
        tot[0] = tot[0] + sm[k]
        tot[1] = tot[1] + sq[k]
        tot[2] = tot[2] + s2[k]
    cnt = float(nphase * tiles)
    m = tot[0] / cnt
    between = np.maximum(tot[1] - cnt * m * m, 0.0)
    var = (tot[2] + 128.0 * between) / (cnt * 128.0)
    inv = 1.0 / np.sqrt(var + IN_EPS)
    ga, be = gamma.double().numpy()[None], beta.double().numpy()[None]
    return torch.from_numpy(np.stack([(ga * inv).astype(np.float32), (be - m * ga * inv).astype(np.float32)], axis=-1))


def ulp_error(got, ref64):
    """|got - ref| in units of the fp32 spacing at the reference, elementwise (float64 tensor)"""
    ref32 = ref64.float()
    ulp = torch.from_numpy(np.spacing(np.abs(ref32.numpy()).astype(np.float32))).double()
    return (got.double() - ref64).abs() / ulp


def synthetic_partials(nphase, tiles, N, C, ratio=None, seed=0):
    """fp32 partials (nphase, N * tiles, C) each of mean and M2, as tiles of N(m_c, s_c^2) samples would give them: the tile means
    scatter by s / sqrt(128) around m, M2 ~ s^2 chi^2_127.  Channel 0 is constant (mean 3, M2 0), channel 1 all zero.  ratio:
    |m_c| / s_c for every other channel (None: a few sigma either way).  gamma, beta seeded alike."""
    g = torch.Generator().manual_seed(9000 + 131 * nphase + 17 * tiles + C + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    s = torch.pow(2.0, torch.randint(-3, 4, (C,), generator=g).double())
    m = (r(C) * 3 * s) if ratio is None else s * ratio * (torch.randint(0, 2, (C,), generator=g).double() * 2 - 1)
    if ratio is None:
        m = m + r(N, 1, C).expand(nphase, N, tiles, C).reshape(nphase, N * tiles, C) * s   # images differ
    mean = m + r(nphase, N * tiles, C) * s / 128 ** 0.5
    m2 = s * s * (127 + (2 * 127) ** 0.5 * r(nphase, N * tiles, C)).clamp(min=1.0)
    mean[..., 0], m2[..., 0] = 3.0, 0.0
    mean[..., 1], m2[..., 1] = 0.0, 0.0
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    beta = torch.randn(C, generator=g) * 0.5
    return mean.float(), m2.float(), gamma, beta


# ---- apply
APPLY_MUTANTS = ("no_relu", "res_lo_dropped", "ld_dst_is_c", "ld_res_is_c", "shared_per_sample", "per_sample_shared",
                 "swap_hw", "other_align", "second_warp_ignored")
# Random flows: the kernel computes the tap weights in fp32 (sample.h), the reference in float64.  The weights' fp32 error moves an
# output by at most this fraction of S = |v s| + |t| + |res| + sum |w src| (float64 weights); measured over the random cases by
# tests/test_norm_chain_cases.py from an fp32 restatement of sample.h (it prints the figure and asserts it stays below), never tuned
# on the device.  The assertion allows 2^-19 S (21 fp32 operations of relative rounding 2^-24 each) plus 4 x this.
APPLY_TAP_MEASURED = 3.6e-6   # 0 (no warp) to 3.55e-6 over the sixteen random cases: a coordinate near 2^5 carries 2^-19 of absolute error
APPLY_REL = 2.0 ** -19 + 4 * APPLY_TAP_MEASURED


class ApplyCase(object):
    """One lwg_norm_apply call.  warps: tuple of 'shared' / 'per_sample' (0 to 2 entries); res: None, 'fp32' or 'split' (the
    latter with a split destination only); every buffer is built by apply_operands."""

    def __init__(self, family, N, H, W, C, relu, warps, align, res, seed):
        self.family, self.N, self.H, self.W, self.C, self.relu, self.warps, self.align, self.res, self.seed = \
            family, N, H, W, C, relu, tuple(warps), align, res, seed


def apply_flow(N, H, W, g, random=False):
    """(N,H,W,2) fp32 flow.  Exact family: multiples of 1/16 in [-2.5, 2.5] -- g + 1, its product with any size below 2^10, the
    - 1 and the halving of sample.h::unnormalize are then exact in fp32 for EITHER align_corners and any H, W (the lattice cases of
    sample_grid need power-of-two sizes), every weight a multiple of 2^-10 -- with the border coordinates -1, +1, the value -2 the
    generator's flows carry (a patch and single pixels) and coordinates outside the image.  random: uniform on [-1.2, 1.2] with a
    -2 patch, as helpers.train_batch."""
    if random:
        T = torch.rand(N, H, W, 2, generator=g) * 2.4 - 1.2
    else:
        T = torch.randint(-40, 41, (N, H, W, 2), generator=g).float() / 16
        T[0, 0, :6, 0] = torch.tensor([-1.0, 1.0, -1.0, 1.0, -2.0, 2.5])
        T[0, 0, :6, 1] = torch.tensor([-1.0, 1.0, 1.0, -1.0, 0.5, -2.5])
    T[N - 1, H // 2:, W // 4:W // 2] = -2.0
    return T


@functools.lru_cache(maxsize=None)
def apply_operands(case):
    """dict of fp32 CPU tensors: raw (N,H,W,C), ss (N,C,2), res (N,H,W,C) or None, warps [(src (1 or N,H,W,C), flow (N,H,W,2))].
    Exact family: raw = integers in [-8, 8] / 4; scale in {+-2^e, +-1.5 * 2^e}, e in [-2, 2]; shift = m / 16, |m| <= 64, both
    signs; res = n / 256, |n| <= 511 (it needs its lo term); warp sources integers in [-8, 8]; flows from apply_flow.  Every
    product and partial sum is a multiple of 2^-10 below 2^7: exact in fp32 in any order, contracted or not.  Shared: read-only."""
    g = torch.Generator().manual_seed(11000 + case.seed)
    N, H, W, C = case.N, case.H, case.W, case.C
    rnd = case.family == "random"
    if rnd:
        raw = torch.randn(N, H, W, C, generator=g)
        ss = torch.stack([torch.randn(N, C, generator=g), 0.5 * torch.randn(N, C, generator=g)], dim=-1).contiguous()
        res = torch.randn(N, H, W, C, generator=g) if case.res else None
        if case.res == "split":   # the operand IS the split buffer: what hi + lo carries
            hi, lo = bf16_split_f32(res)
            res = hi + lo
    else:
        raw = torch.randint(-8, 9, (N, H, W, C), generator=g).float() / 4
        e = torch.randint(-2, 3, (N, C), generator=g).float()
        mant = torch.where(torch.randint(0, 2, (N, C), generator=g) == 0, torch.tensor(1.0), torch.tensor(1.5))
        sign = torch.randint(0, 2, (N, C), generator=g).float() * 2 - 1
        ss = torch.stack([sign * mant * torch.pow(2.0, e), grid((N, C), g, 64, 16.0)], dim=-1).contiguous()
        res = grid((N, H, W, C), g, 511, 256.0) if case.res else None
    warps = []
    for kind in case.warps:
        xn = 1 if kind == "shared" else N
        src = torch.randn(xn, H, W, C, generator=g) if rnd else torch.randint(-8, 9, (xn, H, W, C), generator=g).float()
        warps.append((src, apply_flow(N, H, W, g, rnd)))
    return dict(raw=raw, ss=ss, res=res, warps=warps)


def apply_reference(case, ops=None, mutant=None, with_S=False):
    """The apply pass in float64: [relu](raw * scale + shift) [+ res] [+ sum_k grid_sample(src_k, flow_k)] -> (N,H,W,C), the warps
    from helpers.grid_sample_restated.  with_S: also S = |v s| + |t| + |res| + sum_k sum_taps |w src|.  mutant (APPLY_MUTANTS; the
    ld_* ones are layout mutants, see apply_layout_mutant; swap_hw / other_align are grid_sample_restated's): the way a kernel goes wrong."""
    o = ops or apply_operands(case)
    N, H, W, C = case.N, case.H, case.W, case.C
    v, s, t = o["raw"].double(), o["ss"][:, None, None, :, 0].double(), o["ss"][:, None, None, :, 1].double()
    y = v * s + t
    S = (v * s).abs() + t.abs()
    if case.relu and mutant != "no_relu":
        y = y.clamp(min=0)
    if o["res"] is not None:
        r = o["res"].double()
        if mutant == "res_lo_dropped":
            r = o["res"].bfloat16().double()
        y = y + r
        S = S + r.abs()
    for k, (src, flow) in enumerate(o["warps"]):
        if mutant == "second_warp_ignored" and k == 1:
            continue
        x = src
        if mutant == "shared_per_sample" and src.shape[0] == 1 and N > 1:
            x = torch.cat([src, torch.zeros(N - 1, H, W, C)])   # images 1.. read whatever lies behind the one source: not it
        if mutant == "per_sample_shared" and src.shape[0] > 1:
            x = src[:1]
        xc = x.permute(0, 3, 1, 2)
        align = bool(case.align) != (mutant == "other_align")
        smut = "swap_hw" if mutant == "swap_hw" else None
        y = y + grid_sample_restated(xc, flow, align, smut).permute(0, 2, 3, 1)
        S = S + grid_sample_restated(src.permute(0, 3, 1, 2).abs(), flow, case.align).permute(0, 2, 3, 1)
    return (y, S) if with_S else y


def grid_taps_f32(flow, H, W, align):
    """sample.h::grid_taps restated in numpy float32, operation by operation -> (x0, y0 int64, weights (…,4) float32 nw ne sw se)"""
    f = np.float32
    gx, gy = flow[..., 0].numpy().astype(f), flow[..., 1].numpy().astype(f)

    def unn(gv, size):
        if align:
            return ((gv + f(1)) / f(2)) * f(size - 1)
        return ((gv + f(1)) * f(size) - f(1)) / f(2)
    ix, iy = unn(gx, W), unn(gy, H)
    ix, iy = np.where(ix > f(-4), ix, f(-4)), np.where(iy > f(-4), iy, f(-4))
    ix, iy = np.minimum(ix, f(W + 4)), np.minimum(iy, f(H + 4))
    fx, fy = np.floor(ix), np.floor(iy)
    ex, ey = fx + f(1), fy + f(1)
    w = np.stack([(ex - ix) * (ey - iy), (ix - fx) * (ey - iy), (ex - ix) * (iy - fy), (ix - fx) * (iy - fy)], axis=-1)
    assert w.dtype == np.float32
    return fx.astype(np.int64), fy.astype(np.int64), w


def apply_f32(case, ops=None, fma=False):
    """The kernels' arithmetic restated in numpy float32 in their order: y = v * s + t (fma: one rounding), relu, + residual, then per warp wsum = 0; wsum += src * w over the valid taps nw, ne, sw, se (fma alike); y += wsum."""
    o = ops or apply_operands(case)
    N, H, W, C = case.N, case.H, case.W, case.C
    f = np.float32
    mul_add = (lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)) if fma \
        else (lambda a, b, c: (a * b).astype(f) + c)
    v = o["raw"].numpy()
    s, t = o["ss"][:, None, None, :, 0].numpy(), o["ss"][:, None, None, :, 1].numpy()
    y = mul_add(v, np.broadcast_to(s, v.shape), np.broadcast_to(t, v.shape))
    if case.relu:
        y = np.maximum(y, f(0))
    if o["res"] is not None:
        y = y + o["res"].numpy()
    for src, flow in o["warps"]:
        x0, y0, w = grid_taps_f32(flow, H, W, case.align)
        sn = src.numpy()
        wsum = np.zeros_like(y)
        nidx = np.arange(N)[:, None, None] if src.shape[0] > 1 else np.zeros((N, 1, 1), dtype=np.int64)
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            yy, xx = y0 + dy, x0 + dx
            valid = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            tap = sn[nidx, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            wk = np.broadcast_to(w[..., k][..., None], tap.shape)
            wsum = np.where(valid[..., None], mul_add(tap, wk, wsum), wsum)
        y = y + wsum
    assert y.dtype == np.float32
    return torch.from_numpy(y)


def apply_layout_mutant(expected, ld, offset, which):
    """What a (N,H,W,ld) NaN-filled buffer holds after a kernel wrote `expected` (N,H,W,C) at channel `offset` with the right pixel
    stride (which None) or with C taken for it ('ld_is_c'): the flat pixel p then starts at p * C + offset."""
    N, H, W, C = expected.shape
    buf = torch.full((N * H * W * ld,), float("nan"), dtype=expected.dtype)
    stride = C if which == "ld_is_c" else ld
    pos = (torch.arange(N * H * W) * stride + offset).view(-1, 1) + torch.arange(C).view(1, -1)
    buf[pos.reshape(-1)] = expected.reshape(-1)
    return buf.view(N, H, W, ld)


def _apply_cases():
    cases, seed = {}, 0
    for family in ("exact", "random"):
        for (H, W) in ((4, 32), (6, 20)):
            for C, warps, align, res, relu in (
                    (8, (), 0, None, 1), (36, ("shared",), 0, "fp32", 1), (64, ("per_sample", "shared"), 1, "fp32", 0),
                    (32, ("shared", "per_sample"), 1, "split", 1), (96, ("per_sample",), 0, "split", 1), (32, (), 0, None, 0),
                    (64, ("shared", "shared"), 0, None, 1), (36, ("per_sample", "per_sample"), 1, None, 1)):
                seed += 1
                name = "%s %dx%d C%d warps[%s] align %d res %s relu %d" % (family, H, W, C, ",".join(warps), align, res, relu)
                cases[name] = ApplyCase(family, 3, H, W, C, relu, warps, align, res, seed)
    return cases


APPLY_CASES = _apply_cases()


# ---- raw-input consumers (ConvArgs::raw_in): the halo kernels normalise channels >= raw_from of their input themselves
RAW_INPUT_CASES = [(name, cin, raw_from) for name in ("halo64", "halo128", "halo_tall", "ct_narrow", "ct_wide")
                   for cin, raw_from in ((64, 0), (64, 32))] + [("halo64", 32, 0)]


def raw_input_case(name, cin, ncu=EXACT_NCU):
    c = norm_case(name, ncu)
    c.cin = cin
    return c


def raw_input_operands(case, raw_from, seed=0):
    """x (N,H,W,Cin): channels < raw_from an activation n / 256, |n| <= 511; channels >= raw_from RAW: integers in [-8, 8] / 4.
    ss (N, Cin - raw_from, 2): scale +-2^e, e in [-3, -1], shift m / 256, |m| <= 255, both signs -- relu(raw * scale + shift) is a
    multiple of 1/256 below 2 (it needs its lo term).  w = m / 16, |m| <= 8 (PyTorch layout).  Every product of the conv is a
    multiple of 2^-12 and the sums stay far below 2^24 quanta: the float64 conv rounded to fp32 is the specification."""
    g = torch.Generator().manual_seed(12000 + seed + raw_from)
    N, H, W, cin = case.N, case.H, case.W, case.cin
    x = grid((N, H, W, cin), g, 511, 256.0)
    x[..., raw_from:] = torch.randint(-8, 9, (N, H, W, cin - raw_from), generator=g).float() / 4
    nr = cin - raw_from
    scale = (torch.randint(0, 2, (N, nr), generator=g).float() * 2 - 1) * torch.pow(2.0, torch.randint(-3, 0, (N, nr), generator=g).float())
    ss = torch.stack([scale, grid((N, nr), g, 255, 256.0)], dim=-1).contiguous()
    w = grid(case.w_shape(), g, 8, 16.0)
    return x, ss, w


def raw_input_activation(x, ss, raw_from):
    """the tensor the kernel must multiply, float64 (N,H,W,Cin): relu(x * scale + shift) on the raw channels"""
    a = x.double().clone()
    a[..., raw_from:] = (a[..., raw_from:] * ss[:, None, None, :, 0].double() + ss[:, None, None, :, 1].double()).clamp(min=0)
    return a


def raw_input_reference(case, x, ss, w, raw_from, pad_normalised=False):
    """float64 conv (N,Ho,Wo,Cout) of the activation with ZERO padding.  pad_normalised: the mutant whose out-of-image taps were
    normalised with the rest -- a padded raw channel contributes relu(shift) instead of 0."""
    import torch.nn.functional as F
    a = raw_input_activation(x, ss, raw_from).permute(0, 3, 1, 2)
    if not pad_normalised:
        return case.op(a, w).permute(0, 2, 3, 1).contiguous()
    N, C, H, W = a.shape
    fill = torch.zeros(N, C, dtype=torch.float64)
    fill[:, raw_from:] = ss[..., 1].double().clamp(min=0)
    if case.transposed:
        ap = fill[:, :, None, None].expand(N, C, H + 1, W + 1).clone()
        ap[:, :, :H, :W] = a
        y = F.conv_transpose2d(ap, w.double(), stride=2, padding=1, output_padding=1)[:, :, :2 * H, :2 * W]
    else:
        p = case.pad
        ap = fill[:, :, None, None].expand(N, C, H + 2 * p, W + 2 * p).clone()
        ap[:, :, p:p + H, p:p + W] = a
        y = F.conv2d(ap, w.double(), None, case.stride, 0)
    return y.permute(0, 2, 3, 1).contiguous()
