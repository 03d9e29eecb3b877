"""numpy fp64 restatement of the paired metrics that csrc/eval.hip computes (not a test module; imported by the tests).

What is restated is scikit-image 0.16.2 -- the version the reference's requirements.txt pins -- as the reference's
SSIMMetric / PSNRMetric call it (structural_similarity(pred, ref, multichannel=True) and peak_signal_noise_ratio(ref, pred) on
float32 images in [-1,1], no data_range given), and ScaleShapePoseError.ssp_abs_err_score_func.  scikit-image itself is not a
dependency of this project.
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7
DATA_RANGE = 2.0                       # scikit-image's dtype range of a float image: (-1, 1)
K1, K2 = 0.01, 0.03
C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)   # sample covariance


# ------------------------------------------------------------------------------------------------ the three pixel modes
def map_pixels(x, mode):
    """float32 array -> the float32 values that are scored.  Every step is a separately rounded float32 operation."""
    x = np.asarray(x, np.float32)
    one, two, f255 = np.float32(1), np.float32(2), np.float32(255)
    if mode == 0:
        return x
    if mode == 1:                      # the reference's preprocess: out *= 2; out -= 1
        return (x * two) - one
    if mode == 2:                      # save_cv2_img(normalize=True): ((img + 1) / 2.0 * 255).astype(uint8), then the loader's /255*2-1
        u = np.clip(np.trunc(((x + one) / two) * f255), 0, 255).astype(np.float32)
        return ((u / f255) * two) - one
    raise ValueError(mode)


def quantize_u8(x):
    """the integer the writer stores for a [-1,1] value (truncating, clamped)"""
    x = np.asarray(x, np.float32)
    return np.clip(np.trunc(((x + np.float32(1)) / np.float32(2)) * np.float32(255)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ SSIM
def _s_map(ux, uy, uxx, uyy, uxy):
    vx = COV_NORM * (uxx - ux * ux)
    vy = COV_NORM * (uyy - uy * uy)
    vxy = COV_NORM * (uxy - ux * uy)
    a1, a2 = 2 * ux * uy + C1, 2 * vxy + C2
    b1, b2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (a1 * a2) / (b1 * b2)


def ssim_channel(x, y):
    """one (H,W) channel pair -> mean S over the window positions inside the image (uniform-filter moments, fp64)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if min(x.shape) < WIN:
        raise ValueError("win_size exceeds image extent")
    f = lambda a: uniform_filter(a, size=WIN)
    s = _s_map(f(x), f(y), f(x * x), f(y * y), f(x * y))
    pad = (WIN - 1) // 2
    return float(s[pad:x.shape[0] - pad, pad:x.shape[1] - pad].mean())


def ssim_channel_centred(x, y):
    """the same number by a direct sliding window with centred two-pass sums (another fp64 formulation, no cancellation)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    wx = np.lib.stride_tricks.sliding_window_view(x, (WIN, WIN)).reshape(x.shape[0] - WIN + 1, x.shape[1] - WIN + 1, -1)
    wy = np.lib.stride_tricks.sliding_window_view(y, (WIN, WIN)).reshape(wx.shape)
    ux, uy = wx.mean(-1), wy.mean(-1)
    dx, dy = wx - ux[..., None], wy - uy[..., None]
    n1 = WIN * WIN - 1.0
    vx, vy, vxy = (dx * dx).sum(-1) / n1, (dy * dy).sum(-1) / n1, (dx * dy).sum(-1) / n1
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return float(s.mean())


def ssim(pred, ref, channel=ssim_channel):
    """(3,H,W) float32 in [-1,1] -> the mean of the three channels' mean S"""
    return float(np.mean([channel(pred[c], ref[c]) for c in range(pred.shape[0])]))


# ------------------------------------------------------------------------------------------------ PSNR
def mse(pred, ref):
    d = np.asarray(pred, np.float64) - np.asarray(ref, np.float64)
    return float(np.mean(d * d))


def psnr_data_range(ref):
    lo, hi = float(np.min(ref)), float(np.max(ref))
    if lo < -1 or hi > 1:
        raise ValueError("im_true has intensity values outside the range expected for its data type")
    return 1.0 if lo >= 0 else 2.0


def psnr(pred, ref):
    r = psnr_data_range(ref)
    e = mse(pred, ref)
    return float("inf") if e == 0 else float(10 * np.log10(r * r / e))


def pair_stats(pred, ref, mode=0):
    """(N,3,H,W) float32 pairs -> (N,4) fp64 [mssim, mse, ref_min, ref_max], what lwg_eval_pair_stats writes"""
    p, r = map_pixels(pred, mode), map_pixels(ref, mode)
    return np.array([[ssim(p[i], r[i]), mse(p[i], r[i]), float(r[i].min()), float(r[i].max())] for i in range(len(p))], np.float64)


# ------------------------------------------------------------------------------------------------ SSPE
def sspe_terms(a, b):
    """(N,85) -> (N,3) fp64: |d[0]|, sum |d[-10:]|, sum |d[:-10]| -- the "pose" slice starts at 0, so it holds the camera again"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.stack([d[:, 0], d[:, -10:].sum(1), d[:, 0:-10].sum(1)], 1)


def sspe(a, b):
    """ssp_abs_err_score_func: mean scale error + mean shape error + mean pose error"""
    t = sspe_terms(a, b)
    return float(t[:, 0].mean() + t[:, 1].mean() + t[:, 2].mean())


# ------------------------------------------------------------------------------------------------ resize
def resize_bilinear_ref(x, size):
    import torch
    import torch.nn.functional as F
    return F.interpolate(torch.as_tensor(np.asarray(x)), size=tuple(size), mode="bilinear", align_corners=False).numpy()


def resize_bilinear_restated(x, size):
    """the index arithmetic of lwg_resize_bilinear in numpy float32 (a check of the statement itself): one rounding per step
    except the source index, which is one fused multiply-add"""
    x = np.asarray(x, np.float32)
    f = np.float32

    def taps(n_in, n_out):
        scale = f(n_in) / f(n_out)
        dst = np.arange(n_out, dtype=np.float32)
        # scale*(dst+0.5)-0.5 as ONE fused multiply-add, as torch's binaries evaluate it: the product of two float32 values is
        # exact in fp64 and the sum is then rounded once more to float32 (a double rounding can differ in the last bit only)
        src = np.maximum((np.float64(scale) * (dst + f(0.5)).astype(np.float64) - 0.5).astype(np.float32), f(0))
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        w1 = np.clip(src - i0.astype(np.float32), f(0), f(1)).astype(np.float32)
        return i0, i1, (f(1) - w1).astype(np.float32), w1

    y0, y1, wy0, wy1 = taps(x.shape[2], size[0])
    x0, x1, wx0, wx1 = taps(x.shape[3], size[1])
    top = x[:, :, y0][:, :, :, x0] * wx0 + x[:, :, y0][:, :, :, x1] * wx1
    bot = x[:, :, y1][:, :, :, x0] * wx0 + x[:, :, y1][:, :, :, x1] * wx1
    return (top * wy0[:, None] + bot * wy1[:, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ inputs shared by the tests
def near_flat_pair(h, w, seed=5):
    """a bright, almost flat pair (0.9 +- 1e-4): float32 window moments lose the variance here"""
    rs = np.random.RandomState(seed)
    a = (0.9 + 1e-4 * rs.uniform(-1, 1, (1, 3, h, w))).astype(np.float32)
    b = (0.9 + 1e-4 * rs.uniform(-1, 1, (1, 3, h, w))).astype(np.float32)
    return a, b


def ssim_channel_float32(x, y):
    """the float32 shortcut the kernel must NOT take (kept to show what the 1e-10 bound separates)"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    f = lambda a: uniform_filter(a, size=WIN).astype(np.float32)
    n = np.float32(COV_NORM)
    ux, uy = f(x), f(y)
    vx, vy, vxy = n * (f(x * x) - ux * ux), n * (f(y * y) - uy * uy), n * (f(x * y) - ux * uy)
    c1, c2 = np.float32(C1), np.float32(C2)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    pad = (WIN - 1) // 2
    return float(s[pad:x.shape[0] - pad, pad:x.shape[1] - pad].astype(np.float64).mean())
