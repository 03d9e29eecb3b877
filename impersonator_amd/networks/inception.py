"""torchvision's inception_v3 cut at the final average pool, on the device: the 2048 features per frame that the reference's
FIDMetric and InceptionScoreMetric read (thirdparty/his_evaluators/.../metrics/metrics.py:16-158, 634-781;
InceptionV3(output_blocks=[3], resize_input=False, normalize_input=False) in eval mode).

    net = InceptionV3(inception_v3_state_dict)             # torchvision's keys; AuxLogits.*, fc.* are ignored
    f = net(frames, mode=1)                                # (n,3,H,W) float32 CUDA frames in [0,1] -> (n,2048) float32 CUDA

Everything runs in liblwg (csrc/inception.hip: exact fp32 MFMA convolutions with the BatchNorm folded in); a call only launches
kernels, so it can sit inside the imitation loop and inside a HIP graph.  There is no CPU path: CPU tensors raise.  Out of scope:
the classifier (fc), AuxLogits, `transform_input` (the reference never runs them), gradients.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _chk

BN_EPS = 1e-3
FEATURES = 2048
NET_SIZE = 299           # what the reference resizes every frame to
MIN_SIZE = 75            # 75 -> 37 -> 35 -> 17 -> 15 -> 7 -> 3 -> 1: the smallest input at which Mixed_7c still has a pixel
STAGES = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2",
          "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
          "Mixed_7c")


def _convs():
    """(name, cin, cout, (kh, kw), stride, (ph, pw)) of the 94 BasicConv2d modules, in torchvision's definition order -- the
    order of the weight blob"""
    out = []

    def c(name, cin, cout, k, stride=1, pad=0):
        k = (k, k) if isinstance(k, int) else k
        pad = (pad, pad) if isinstance(pad, int) else pad
        out.append((name, cin, cout, k, stride, pad))

    c("Conv2d_1a_3x3", 3, 32, 3, 2)
    c("Conv2d_2a_3x3", 32, 32, 3)
    c("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    c("Conv2d_3b_1x1", 64, 80, 1)
    c("Conv2d_4a_3x3", 80, 192, 3)
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):          # InceptionA
        c(name + ".branch1x1", cin, 64, 1)
        c(name + ".branch5x5_1", cin, 48, 1)
        c(name + ".branch5x5_2", 48, 64, 5, 1, 2)
        c(name + ".branch3x3dbl_1", cin, 64, 1)
        c(name + ".branch3x3dbl_2", 64, 96, 3, 1, 1)
        c(name + ".branch3x3dbl_3", 96, 96, 3, 1, 1)
        c(name + ".branch_pool", cin, pf, 1)
    c("Mixed_6a.branch3x3", 288, 384, 3, 2)                                                              # InceptionB
    c("Mixed_6a.branch3x3dbl_1", 288, 64, 1)
    c("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    c("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):        # InceptionC
        c(name + ".branch1x1", 768, 192, 1)
        c(name + ".branch7x7_1", 768, c7, 1)
        c(name + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        c(name + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        c(name + ".branch7x7dbl_1", 768, c7, 1)
        c(name + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        c(name + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        c(name + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        c(name + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        c(name + ".branch_pool", 768, 192, 1)
    c("Mixed_7a.branch3x3_1", 768, 192, 1)                                                               # InceptionD
    c("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    c("Mixed_7a.branch7x7x3_1", 768, 192, 1)
    c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    c("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):                                           # InceptionE
        c(name + ".branch1x1", cin, 320, 1)
        c(name + ".branch3x3_1", cin, 384, 1)
        c(name + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        c(name + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        c(name + ".branch3x3dbl_1", cin, 448, 1)
        c(name + ".branch3x3dbl_2", 448, 384, 3, 1, 1)
        c(name + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        c(name + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        c(name + ".branch_pool", cin, 192, 1)
    return tuple(out)


CONVS = _convs()
WHAT = "InceptionV3 (torchvision inception_v3 naming expected)"


def _take(sd, key, shape, what=WHAT):
    try:
        t = sd[key]
    except KeyError:
        raise KeyError("%s state_dict lacks %s" % (what, key))
    t = torch.as_tensor(t).detach()
    if not t.dtype.is_floating_point:
        raise TypeError("%s: %s has dtype %s, expected a floating-point tensor" % (what, key, t.dtype))
    t = t.cpu()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s has shape %s, expected %s" % (what, key, tuple(t.shape), tuple(shape)))
    return t


def fold_bn(gamma, beta, mean, var, eps=BN_EPS):
    """BatchNorm2d in eval mode as y = x * scale + shift, computed in fp64 and rounded once: -> (scale, shift) float32 tensors"""
    g, b, m, v = (torch.as_tensor(t).detach().cpu().double() for t in (gamma, beta, mean, var))
    scale = g / torch.sqrt(v + eps)
    shift = b - m * scale
    return scale.float(), shift.float()


def pack_weights(state_dict):
    """Everything `lwg_inception_set_weights` takes, as one flat fp32 CPU tensor in the order include/lwg.h documents: per conv
    w as [kh][kw][ci][co], then the folded BatchNorm's scale and shift.  AuxLogits.*, fc.* and num_batches_tracked are ignored;
    a missing key raises KeyError, a misshapen one ValueError, a non-float one TypeError, each naming the key."""
    parts = []
    for name, cin, cout, k, _, _ in CONVS:
        w = _take(state_dict, name + ".conv.weight", (cout, cin, k[0], k[1])).float()
        bn = [_take(state_dict, "%s.bn.%s" % (name, s), (cout,)) for s in ("weight", "bias", "running_mean", "running_var")]
        scale, shift = fold_bn(*bn)
        parts += [w.permute(2, 3, 1, 0).contiguous().reshape(-1), scale, shift]
    return torch.cat(parts).contiguous()


class InceptionV3(object):
    """state_dict: torchvision's inception_v3 state_dict (<name>.conv.weight, <name>.bn.{weight,bias,running_mean,running_var};
    other keys are ignored).  max_batch: frames per launch sequence (larger batches are chunked); image_size: the largest height
    and width a call may bring (int or (h, w))."""

    def __init__(self, state_dict, max_batch=8, image_size=256):
        self.max_batch = max(1, int(max_batch))
        hw = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        self.max_h, self.max_w = max(1, int(hw[0])), max(1, int(hw[1]))
        self._blob = pack_weights(state_dict)
        self._handle = None
        self._uploaded = False

    # ------------------------------------------------------------------ handle / weights
    def load_state_dicts(self, state_dict):
        """replaces the weights; the handle and its scratch stay"""
        self._blob = pack_weights(state_dict)
        self._uploaded = False

    def _ensure_handle(self):
        lib = _lib.load()
        if self._handle is None:
            h = ctypes.c_void_p()
            _lib.check(lib.lwg_inception_create(ctypes.byref(h), self.max_batch, self.max_h, self.max_w))
            self._handle = h
            self._uploaded = False
        if not self._uploaded:
            if lib.lwg_inception_weight_floats() != self._blob.numel():
                raise _lib.LwgError(-5, "pack_weights wrote %d floats, the library takes %d"
                                    % (self._blob.numel(), lib.lwg_inception_weight_floats()))
            _lib.check(lib.lwg_inception_set_weights(self._handle, ctypes.c_void_p(self._blob.data_ptr()), self._blob.numel()))
            self._uploaded = True
        return self._handle

    def release(self):
        if self._handle is not None:
            _lib.load().lwg_inception_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def __call__(self, frames, mode=0, out=None, resize=NET_SIZE, tap=None):
        """frames (n,3,H,W) contiguous float32 CUDA tensor -> (n,2048) float32 CUDA tensor.  mode: 0, 1 or 2 as in
        utils.metrics.pair_stats (1 is the reference's `out *= 2; out -= 1` on [0,1] frames).  resize: 299 (the reference's
        F.interpolate to 299 x 299) or 0 (the frames as they are).  out: an (n,2048) float32 tensor to write into.
        tap: (stage, tensor) -- the NHWC output of stage 0..17 (STAGES) is copied into the contiguous float32 tensor; one launch
        sequence only (n <= max_batch).  Only launches kernels."""
        _chk(frames)
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError("InceptionV3 takes an (N,3,H,W) tensor, got %s" % (tuple(frames.shape),))
        if mode not in (0, 1, 2):
            raise ValueError("mode must be 0 ([-1,1] as it is), 1 ([0,1] input) or 2 ([-1,1] through 8 bits), got %r" % (mode,))
        if resize not in (0, NET_SIZE):
            raise ValueError("resize must be %d or 0 (no resize), got %r" % (NET_SIZE, resize))
        n, _, h, w = frames.shape
        feats = out if out is not None else torch.empty((n, FEATURES), device=frames.device, dtype=torch.float32)
        if tuple(feats.shape) != (n, FEATURES) or feats.dtype != torch.float32 or not feats.is_contiguous() or not feats.is_cuda:
            raise ValueError("out must be a contiguous (%d, %d) float32 CUDA tensor" % (n, FEATURES))
        stage, tap_out = (-1, None) if tap is None else (int(tap[0]), tap[1])
        if tap is not None:
            _chk(tap_out)
            if n > self.max_batch or not 0 <= stage < len(STAGES):
                raise ValueError("a tap takes one launch sequence (n <= %d) and a stage in 0..%d" % (self.max_batch, len(STAGES) - 1))
        handle = self._ensure_handle()
        lib = _lib.load()
        st = _lib.stream_ptr()
        for s in range(0, n, self.max_batch):
            e = min(n, s + self.max_batch)
            _lib.check(lib.lwg_inception_forward(handle, _lib.ptr(frames[s:e]), e - s, h, w, int(mode), int(resize), int(resize),
                                                 _lib.ptr(feats[s:e]), stage, _lib.ptr(tap_out), st))
        return feats


def stage_shapes(h, w):
    """[(Hs, Ws, Cs)] of the 18 stages for an h x w network input (what a tap tensor must hold per frame)"""
    co = lambda v, k, s, p: (v + 2 * p - k) // s + 1
    out = []
    h, w = co(h, 3, 2, 0), co(w, 3, 2, 0)
    out.append((h, w, 32))
    h, w = h - 2, w - 2
    out.append((h, w, 32))
    out.append((h, w, 64))
    h, w = co(h, 3, 2, 0), co(w, 3, 2, 0)
    out.append((h, w, 64))
    out.append((h, w, 80))
    h, w = h - 2, w - 2
    out.append((h, w, 192))
    h, w = co(h, 3, 2, 0), co(w, 3, 2, 0)
    out.append((h, w, 192))
    out += [(h, w, 256), (h, w, 288), (h, w, 288)]
    h, w = co(h, 3, 2, 0), co(w, 3, 2, 0)
    out += [(h, w, 768)] * 5
    h, w = co(h, 3, 2, 0), co(w, 3, 2, 0)
    out += [(h, w, 1280), (h, w, 2048), (h, w, 2048)]
    return out

