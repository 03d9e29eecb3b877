"""Small host-side utilities with the reference's names (utils/util.py)."""
import pickle

import torch
import torch.nn.functional as F


def morph(src_bg_mask, ks, mode='erode', kernel=None, complement=False):
    """utils/util.py:73-89: erode / dilate a {0,1} mask with a ks x ks box (border padded with 1 / 0).

    CUDA tensors: liblwg's box-count kernel (lwg_morph, personalize.hip) -- `complement` (extension) returns 1 - result from the
    same launch.  CPU tensors (the host-side tests): the same counts from an integral image (two cumulative sums).  Counts
    are small integers, exact in fp32, so the result equals the reference's ones-kernel conv2d.  Runs once per source image
    (models/imitator.py:116,132)."""
    if kernel is not None:
        raise NotImplementedError("custom structuring elements are not used on the Imitator path")
    if mode not in ('erode', 'dilate'):
        mode = 'dilate'   # the reference's `else` branch
    if src_bg_mask.is_cuda:
        from .. import _lib
        m = src_bg_mask.float()
        n, c, h, w = m.shape
        if c != 1 or m.stride(3) != 1 or m.stride(2) != w:
            raise ValueError("morph: (n,1,H,W) mask with dense image planes expected, got %s strides %s" % (tuple(m.shape), m.stride()))
        out = torch.empty((n, 1, h, w), device=m.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_morph(_lib.ptr(m), n, h, w, m.stride(0) if n > 1 else h * w, ks, 0 if mode == 'erode' else 1,
                                         int(bool(complement)), _lib.ptr(out), _lib.stream_ptr()))
        return out
    n_ks = ks ** 2
    pad = ks // 2
    x = F.pad(src_bg_mask, [pad, pad, pad, pad], value=1.0 if mode == 'erode' else 0.0)
    ii = F.pad(x.cumsum(-1).cumsum(-2), [1, 0, 1, 0])
    box = ii[..., ks:, ks:] - ii[..., :-ks, ks:] - ii[..., ks:, :-ks] + ii[..., :-ks, :-ks]
    out = (box == n_ks).float() if mode == 'erode' else (box >= 1).float()
    return 1 - out if complement else out


def image_grid_shape(n, H, W, nrow=8, padding=2):
    """(grid_h, grid_w) of torchvision's make_grid for n images of H x W (lwg_image_grid_shape; needs no device)."""
    import ctypes
    from .. import _lib
    gh, gw = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().lwg_image_grid_shape(int(n), int(H), int(W), int(nrow), int(padding), ctypes.byref(gh), ctypes.byref(gw)))
    return gh.value, gw.value


def image_grid_u8(x, nrow=8, padding=2, pad_value=0.0, normalize=False):
    """torchvision.utils.make_grid + the uint8 conversion of save_image in one liblwg launch (lwg_image_grid_u8): x (n,3,H,W)
    CUDA float tensor -> (grid_h, grid_w, 3) uint8 CUDA tensor, `uint8(clamp(v * 255 + 0.5, 0, 255))` with v = (x + 1) / 2 when
    `normalize` (the reference's run_view.py:77) else x."""
    from .. import _lib
    if not x.is_cuda:
        raise RuntimeError("image_grid_u8: the images must be a CUDA tensor (no CPU path)")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("image_grid_u8: (n, 3, H, W) expected, got %s" % (tuple(x.shape),))
    x = x.float().contiguous()
    n, _, h, w = x.shape
    gh, gw = image_grid_shape(n, h, w, nrow, padding)
    out = torch.empty((gh, gw, 3), device=x.device, dtype=torch.uint8)
    _lib.check(_lib.load().lwg_image_grid_u8(_lib.ptr(x), n, h, w, int(nrow), int(padding), float(pad_value), int(bool(normalize)),
                                             _lib.ptr(out), _lib.stream_ptr()))
    return out


def save_image_grid(x, path, nrow=8, padding=2, pad_value=0.0, normalize=False):
    """torchvision.utils.save_image(x, path): the grid is laid out and converted on the device (image_grid_u8), its bytes come
    back in ONE device->host copy and PIL writes them."""
    from PIL import Image
    grid = image_grid_u8(x, nrow=nrow, padding=padding, pad_value=pad_value, normalize=normalize)
    Image.fromarray(grid.cpu().numpy()).save(path)
    return grid


_JPEG_SUBSAMPLING = {'4:2:0': 420, '420': 420, 420: 420, '4:4:4': 444, '444': 444, 444: 444}


def _jpeg_subsampling(subsampling):
    try:
        return _JPEG_SUBSAMPLING[subsampling]
    except (KeyError, TypeError):
        raise ValueError("jpeg subsampling %r: '4:2:0' (420) or '4:4:4' (444) expected" % (subsampling,))


def jpeg_stream_bytes(H, W, subsampling='4:2:0'):
    """The most one frame's .jpg stream can take (lwg_jpeg_stream_bytes; needs no device): the row stride of jpeg_encode."""
    from .. import _lib
    n = _lib.load().lwg_jpeg_stream_bytes(int(H), int(W), _jpeg_subsampling(subsampling))
    if n == 0:
        raise ValueError("jpeg: %d x %d: sides must be positive multiples of 16" % (H, W))
    return n


def jpeg_encode(x, quality=75, subsampling='4:2:0'):
    """Baseline JPEG files of a batch of images, encoded on the device (lwg_jpeg_encode, csrc/jpeg.hip): x (N,3,H,W) CUDA float
    tensor in [-1,1] -> (bytes uint8 (N, stride), lengths int32 (N,)), both CUDA tensors; frame n's file is bytes[n, :lengths[n]]
    and equals what PIL writes (`quality`, `subsampling`, optimize=False) for the uint8 image of cv_utils.save_cv2_img(normalize=True).
    Stream-ordered, no synchronisation; H and W must be multiples of 16."""
    from .. import _lib
    if not x.is_cuda:
        raise RuntimeError("jpeg_encode: the images must be a CUDA tensor (no CPU path)")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("jpeg_encode: (n, 3, H, W) expected, got %s" % (tuple(x.shape),))
    sub = _jpeg_subsampling(subsampling)
    x = x.float().contiguous()
    n, _, h, w = x.shape
    lib = _lib.load()
    stride, ws_bytes = lib.lwg_jpeg_stream_bytes(h, w, sub), lib.lwg_jpeg_workspace_bytes(n, h, w, sub)
    out = torch.empty((n, max(stride, 1)), device=x.device, dtype=torch.uint8)
    lengths = torch.empty((n,), device=x.device, dtype=torch.int32)
    ws = torch.empty((max(ws_bytes, 16),), device=x.device, dtype=torch.uint8)
    _lib.check(lib.lwg_jpeg_encode(_lib.ptr(x), n, h, w, int(quality), sub, _lib.ptr(out), out.stride(0), _lib.ptr(lengths),
                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return out, lengths


def jpeg_bytes(x, quality=75, subsampling='4:2:0'):
    """jpeg_encode, then the files as a list of `bytes`: the lengths come to the host first, then only out[:, :max(lengths)]
    (about 13 KB a frame at 256 x 256 and quality 75, against 786 KB of float32), sliced per frame on the host."""
    out, lengths = jpeg_encode(x, quality=quality, subsampling=subsampling)
    lens = lengths.cpu().tolist()
    host = out[:, :max(lens)].cpu().numpy()
    return [host[i, :n].tobytes() for i, n in enumerate(lens)]


def load_pickle_file(pkl_path):
    """utils/util.py:235-239."""
    with open(pkl_path, 'rb') as f:
        return pickle.load(f, encoding='latin1')


def mkdir(path):
    import os
    os.makedirs(path, exist_ok=True)
    return path
