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
