"""torch restatement of LPIPS v0.1 with the AlexNet backbone, as csrc/lpips.hip computes it (not a test module; imported by the
tests and by tests/golden/make_lpips_golden.py).

What is restated is the reference's PNetLin('alex', version '0.1').forward in eval mode (thirdparty/his_evaluators/.../metrics/
lpips/models/networks_basic.py): the scaling layer, torchvision's alexnet().features[0:12] tapped after each ReLU, the unit
normalisation with eps = 1e-10 added to the norm, the squared difference, the 1x1 `lin` convolution (dropout is identity) and the
spatial mean; the distance is the sum of the five terms in layer order.  Run in fp64 it is the yardstick; in fp32 it is what torch
itself gives.  shift and scale are the float32 constants of the reference promoted to the working precision, as there.

Also here: the seeded inputs of the golden cases and the error bound of the fused layer-distance kernel.
"""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# index in torchvision's alexnet().features, stride, padding; a MaxPool(3, 2) follows the first two taps
CONVS = ((0, 4, 2), (3, 1, 2), (6, 1, 1), (8, 1, 1), (10, 1, 1))
CHANNELS = (64, 192, 384, 256, 256)
EPS = 1e-10
U64 = 2.0 ** -53

# the golden cases: (name, n, height, width); each is scored as (noise, noise) and as (image, image + 0.1 * noise clamped)
CASES = (("31x31", 2, 31, 31), ("35x47", 1, 35, 47), ("64x64", 1, 64, 64), ("256x256", 1, 256, 256))
GOLDEN_SEED = 0          # utils.synthetic.lpips_state_dicts(GOLDEN_SEED): the AlexNet weights of the golden values


def tensors(state_dict, dtype=torch.float64):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state_dict.items()}


def scale_input(x):
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def features(x, alex):
    """x (N,3,H,W), already scaled -> the five ReLU outputs"""
    taps = []
    for j, (i, stride, pad) in enumerate(CONVS):
        if j in (1, 2):
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, alex["features.%d.weight" % i], alex["features.%d.bias" % i], stride=stride, padding=pad))
        taps.append(x)
    return taps


def layer_distance(f0, f1, w):
    """f0, f1 (N,C,H,W), w (C) -> (N,): mean over pixels of sum_c w_c (f0/(|f0|+eps) - f1/(|f1|+eps))^2"""
    n0 = torch.sqrt((f0 ** 2).sum(dim=1, keepdim=True)) + EPS
    n1 = torch.sqrt((f1 ** 2).sum(dim=1, keepdim=True)) + EPS
    d = ((f0 / n0 - f1 / n1) ** 2 * w.view(1, -1, 1, 1)).sum(dim=1)
    return d.mean(dim=(1, 2))


@torch.no_grad()
def lpips(pred, ref, alex, lin, dtype=torch.float64):
    """pred, ref (N,3,H,W) arrays in [-1,1]; alex, lin: state dicts (arrays or tensors) -> (dist (N,), taps (N,5)) numpy, in
    `dtype` arithmetic from the float32 operands"""
    a, l = tensors(alex, dtype), tensors(lin, dtype)
    f0 = features(scale_input(torch.as_tensor(np.asarray(pred)).to(dtype)), a)
    f1 = features(scale_input(torch.as_tensor(np.asarray(ref)).to(dtype)), a)
    taps = torch.stack([layer_distance(f0[j], f1[j], l["lin%d.model.1.weight" % j].reshape(-1)) for j in range(5)], dim=1)
    dist = taps[:, 0]
    for j in range(1, 5):
        dist = dist + taps[:, j]
    return dist.numpy(), taps.numpy()


def case_inputs(index, kind):
    """the seeded frames of golden case `index`: kind 'noise' -> two independent uniform [-1,1] images; 'near' -> a smooth image
    and that image + 0.1 * noise, clamped to [-1,1].  float32 (n,3,h,w) arrays."""
    from impersonator_amd.utils import synthetic
    _, n, h, w = CASES[index]
    rs = np.random.RandomState(1000 + 10 * index + (0 if kind == "noise" else 1))
    if kind == "noise":
        return (rs.uniform(-1, 1, (n, 3, h, w)).astype(np.float32), rs.uniform(-1, 1, (n, 3, h, w)).astype(np.float32))
    img = synthetic.smooth_image(2000 + index, (n, 3, h, w))
    noisy = np.clip(img + np.float32(0.1) * rs.uniform(-1, 1, (n, 3, h, w)).astype(np.float32), -1, 1).astype(np.float32)
    return noisy, img


def layer_distance_bound(f0, f1, w):
    """Worst-case error of the fused fp64 layer distance against the exact value, per frame: f0, f1 (n,P,C) float32 arrays, w (C)
    non-negative -> (value (n,) in extended precision, bound (n,) in fp64).  With u = 2^-53, a = x0/n0, b = x1/n1:
        delta_c   = (C/2 + 3) u (|a_c| + |b_c|) + u |a_c - b_c|
            -- the norm's relative error: C-1 additions of non-negative exact products under a correctly rounded square root
               ((C-1)/2 u + u), the addition of eps (u) and the correctly rounded division (u), on each of a_c and b_c; then the
               rounding of the subtraction
        per term  <= 2 |a_c - b_c| delta_c + delta_c^2                       -- the square of a perturbed difference
        bound     = mean over pixels of sum_c w_c (per term)  +  (C + P + 4) u value
            -- the square's and the product's roundings, the C additions of non-negative terms per pixel, the P additions over
               the pixels and the final division, all relative to the (non-negative) value itself."""
    # the "exact" value in extended precision (x86 long double, u = 2^-64: 2048 times finer than what is being judged); eps is the
    # fp64 constant 1e-10, as in the kernel
    ld = np.longdouble
    x0, x1, w = np.asarray(f0, ld), np.asarray(f1, ld), np.asarray(w, ld)
    _, P, C = x0.shape
    n0 = np.sqrt((x0 * x0).sum(-1, keepdims=True)) + ld(EPS)
    n1 = np.sqrt((x1 * x1).sum(-1, keepdims=True)) + ld(EPS)
    a, b = x0 / n0, x1 / n1
    value = (w * (a - b) ** 2).sum(-1).mean(-1)
    delta = (C / 2.0 + 3.0) * U64 * (np.abs(a) + np.abs(b)) + U64 * np.abs(a - b)
    term = 2.0 * np.abs(a - b) * delta + delta * delta
    bound = (w * term).sum(-1).mean(-1) + (C + P + 4.0) * U64 * value
    return value, bound.astype(np.float64)
