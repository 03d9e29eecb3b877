"""LPIPS v0.1 with the AlexNet backbone on the device: the distance the reference's PerceptualMetric reports
(thirdparty/his_evaluators/.../metrics/lpips: PerceptualLoss(model='net-lin', net='alex') -> PNetLin.forward, eval mode).

    m = LPIPS(alexnet_state_dict, lin_state_dict)          # torchvision alexnet + the LPIPS v0.1 alex.pth
    d = m(pred, ref)                                       # (n,3,H,W) float32 CUDA frames in [-1,1] -> (n,) float64 CUDA

Everything runs in liblwg (csrc/lpips.hip: exact fp32 MFMA convolutions, fp64 distance); a call only launches kernels, so it can
sit inside the imitation loop and inside a HIP graph.  There is no CPU path: CPU tensors raise.  Out of scope: the vgg and
squeeze backbones, version 0.0, spatial=True, gradients.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _chk

# torchvision's alexnet().features: the index of each convolution and its (Cout, Cin, k)
CONVS = ((0, 64, 3, 11), (3, 192, 64, 5), (6, 384, 192, 3), (8, 256, 384, 3), (10, 256, 256, 3))
CHANNELS = tuple(c[1] for c in CONVS)
MIN_SIZE = 31            # 31 -> 7 -> 3 -> 1: the smallest size at which relu5 still has a pixel
TAPS = len(CONVS)


def _take(sd, key, shape, what):
    try:
        t = sd[key]
    except KeyError:
        raise KeyError("%s state_dict lacks %s" % (what, key))
    t = torch.as_tensor(t).detach().float().cpu()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s has shape %s, expected %s" % (what, key, tuple(t.shape), tuple(shape)))
    return t


def pack_weights(alex_state_dict, lin_state_dict):
    """Everything `lwg_lpips_set_weights` takes, as one flat fp32 CPU tensor in the order include/lwg.h documents:
    per conv w as [kh][kw][ci][co], then its bias; then the five lin vectors.  A missing key raises KeyError naming it."""
    parts = []
    for i, cout, cin, k in CONVS:
        w = _take(alex_state_dict, "features.%d.weight" % i, (cout, cin, k, k), "AlexNet (torchvision alexnet naming expected)")
        b = _take(alex_state_dict, "features.%d.bias" % i, (cout,), "AlexNet (torchvision alexnet naming expected)")
        parts += [w.permute(2, 3, 1, 0).contiguous().reshape(-1), b.reshape(-1)]
    for j, c in enumerate(CHANNELS):
        parts.append(_take(lin_state_dict, "lin%d.model.1.weight" % j, (1, c, 1, 1), "LPIPS v0.1 alex.pth").reshape(-1))
    return torch.cat(parts).contiguous()


class LPIPS(object):
    """alex_state_dict: torchvision's alexnet state_dict (features.{0,3,6,8,10}.{weight,bias}; other keys are ignored);
    lin_state_dict: the LPIPS v0.1 alex.pth (lin{0..4}.model.1.weight, shape (1,C,1,1)).  max_batch: pairs per launch sequence
    (larger batches are chunked); image_size: the largest height and width a call may bring (int or (h, w))."""

    def __init__(self, alex_state_dict, lin_state_dict, max_batch=8, image_size=256):
        self.max_batch = max(1, int(max_batch))
        hw = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        self.max_h, self.max_w = max(MIN_SIZE, int(hw[0])), max(MIN_SIZE, int(hw[1]))
        self._blob = pack_weights(alex_state_dict, lin_state_dict)
        self._handle = None
        self._uploaded = False

    # ------------------------------------------------------------------ handle / weights
    def load_state_dicts(self, alex_state_dict, lin_state_dict):
        """replaces the weights; the handle and its scratch stay"""
        self._blob = pack_weights(alex_state_dict, lin_state_dict)
        self._uploaded = False

    def _ensure_handle(self):
        lib = _lib.load()
        if self._handle is None:
            h = ctypes.c_void_p()
            _lib.check(lib.lwg_lpips_create(ctypes.byref(h), self.max_batch, self.max_h, self.max_w))
            self._handle = h
            self._uploaded = False
        if not self._uploaded:
            if lib.lwg_lpips_weight_floats(self._handle) != self._blob.numel():
                raise _lib.LwgError(-5, "pack_weights wrote %d floats, the library takes %d"
                                    % (self._blob.numel(), lib.lwg_lpips_weight_floats(self._handle)))
            _lib.check(lib.lwg_lpips_set_weights(self._handle, ctypes.c_void_p(self._blob.data_ptr()), self._blob.numel()))
            self._uploaded = True
        return self._handle

    def release(self):
        if self._handle is not None:
            _lib.load().lwg_lpips_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def __call__(self, pred, ref, mode=0, out=None, taps=None):
        """pred, ref (n,3,H,W) contiguous float32 CUDA tensors -> (n,) float64 CUDA tensor, the LPIPS distance per frame.
        mode: 0, 1 or 2 as in utils.metrics.pair_stats, applied to both images.  out: an (n,) float64 tensor to write into;
        taps: an (n,5) float64 tensor that receives the five per-layer terms.  Only launches kernels."""
        _chk(pred, ref)
        if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != ref.shape:
            raise ValueError("LPIPS takes two (N,3,H,W) tensors of one shape, got %s and %s" % (tuple(pred.shape), tuple(ref.shape)))
        if mode not in (0, 1, 2):
            raise ValueError("mode must be 0 ([-1,1] as it is), 1 ([0,1] input) or 2 ([-1,1] through 8 bits), got %r" % (mode,))
        n, _, h, w = pred.shape
        dist = out if out is not None else torch.empty((n,), device=pred.device, dtype=torch.float64)
        for t, shape, name in ((dist, (n,), "out"), (taps, (n, TAPS), "taps")):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("%s must be a contiguous %s float64 CUDA tensor" % (name, shape))
        handle = self._ensure_handle()
        lib = _lib.load()
        st = _lib.stream_ptr()
        for s in range(0, n, self.max_batch):
            e = min(n, s + self.max_batch)
            _lib.check(lib.lwg_lpips_forward(handle, _lib.ptr(pred[s:e]), _lib.ptr(ref[s:e]), e - s, h, w, int(mode),
                                             _lib.ptr(dist[s:e]), None if taps is None else _lib.ptr(taps[s:e]), st))
        return dist
