"""Op-level convolution and its gradients on MI355X (liblwg, train.hip): thin tensor wrappers over
lwg_conv2d_{forward, backward_data, backward_weight}.  Activations are NHWC fp32 CUDA tensors, weights keep PyTorch's
layouts ((Cout,Cin,k,k); (Cin,Cout,3,3) for the transposed conv).  Building blocks of the generator-side training step
(SURVEY.md 8f row 4); the inference path does not go through here."""
import ctypes

import torch

from . import _lib


class _Desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("N", "H", "W", "Cin", "Cout", "k", "stride", "pad", "transposed", "precision")]


PRECISIONS = {"fp32": 0, "bf16x3": 1}


def _desc(x_shape, cin, cout, k, stride, pad, transposed, precision="fp32"):
    n, h, w, _ = x_shape
    return _Desc(n, h, w, cin, cout, k, stride, pad, int(transposed), PRECISIONS[precision])


def _ws(d, dev):
    nbytes = _lib.load().lwg_conv2d_workspace_bytes(ctypes.byref(d))
    if not nbytes:
        raise _lib.LwgError(-2, _lib.load().lwg_last_error().decode(errors="replace"))
    return torch.empty(nbytes // 4 + 1, device=dev, dtype=torch.float32), nbytes


def _out_hw(h, w, k, stride, pad, transposed):
    return (2 * h, 2 * w) if transposed else ((h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)


def _chk(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("lwg ops take contiguous float32 CUDA tensors (no CPU fallback)")


@torch.no_grad()
def conv2d_forward(x, w, bias=None, stride=1, pad=0, transposed=False, precision="fp32"):
    """x (N,H,W,Cin) -> (N,Ho,Wo,Cout); F.conv2d / F.conv_transpose2d(stride 2, padding 1, output_padding 1).
    precision 'bf16x3': the inference path's split-bf16 kernel where the layer fits it (include/lwg.h)."""
    _chk(x, w, bias)
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    d = _desc(x.shape, cin, cout, w.shape[2], stride, pad, transposed, precision)
    ho, wo = _out_hw(x.shape[1], x.shape[2], w.shape[2], stride, pad, transposed)
    y = torch.empty((x.shape[0], ho, wo, cout), device=x.device, dtype=torch.float32)
    ws, nb = _ws(d, x.device)
    _lib.check(_lib.load().lwg_conv2d_forward(ctypes.byref(d), _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y),
                                              _lib.ptr(ws), nb, _lib.stream_ptr()))
    return y


@torch.no_grad()
def conv2d_backward_data(dy, w, x_shape, stride=1, pad=0, transposed=False, precision="fp32"):
    """Gradient wrt the input: dy (N,Ho,Wo,Cout) -> dx of shape x_shape (N,H,W,Cin)."""
    _chk(dy, w)
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    d = _desc(x_shape, cin, cout, w.shape[2], stride, pad, transposed, precision)
    dx = torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    ws, nb = _ws(d, dy.device)
    _lib.check(_lib.load().lwg_conv2d_backward_data(ctypes.byref(d), _lib.ptr(dy), _lib.ptr(w), _lib.ptr(dx), _lib.ptr(ws), nb,
                                                    _lib.stream_ptr()))
    return dx


@torch.no_grad()
def _out(out, shape, device):
    """`out` when it is a usable destination (contiguous fp32 tensor of `shape` on `device`), else a fresh tensor."""
    if out is None:
        return torch.empty(tuple(shape), device=device, dtype=torch.float32)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError("out= must be a contiguous fp32 tensor of shape %s on %s" % (tuple(shape), device))
    return out


@torch.no_grad()
def conv2d_backward_weight(x, dy, w_shape, stride=1, pad=0, transposed=False, with_bias=False, precision="fp32", out=None):
    """Gradient wrt the weight (PyTorch layout `w_shape`) and, optionally, the bias.  `out`: write dw there (e.g. the
    parameter's slice of a flat gradient buffer) instead of into a fresh tensor."""
    _chk(x, dy)
    cin, cout = (w_shape[0], w_shape[1]) if transposed else (w_shape[1], w_shape[0])
    d = _desc(x.shape, cin, cout, w_shape[2], stride, pad, transposed, precision)
    dw = _out(out, w_shape, x.device)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if with_bias else None
    ws, nb = _ws(d, x.device)
    _lib.check(_lib.load().lwg_conv2d_backward_weight(ctypes.byref(d), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(db),
                                                      _lib.ptr(ws), nb, _lib.stream_ptr()))
    return (dw, db) if with_bias else dw


def _heads_ws(n, h, w, dev):
    nbytes = _lib.load().lwg_heads_workspace_bytes(n, h, w)
    return torch.empty(nbytes // 4 + 1, device=dev, dtype=torch.float32), nbytes


@torch.no_grad()
def heads_forward(x, w):
    """Regression heads: x (N,H,W,64), w (>=4,64,7,7) -> (tanh(conv rows 0-2) (N,3,H,W), sigmoid(conv row 3) (N,1,H,W)).
    PRECONDITION x >= 0 (post-ReLU activations, what the generator feeds its heads): the kernel is the inference path's,
    which folds the preceding ReLU into its operand load -- negative entries are read as 0 (include/lwg.h)."""
    _chk(x, w)
    n, h, wd, c = x.shape
    if c != 64 or tuple(w.shape[1:]) != (64, 7, 7) or w.shape[0] < 4:
        raise RuntimeError("heads_forward: x (N,H,W,64) and w (>=4,64,7,7) expected")
    color = torch.empty((n, 3, h, wd), device=x.device, dtype=torch.float32)
    mask = torch.empty((n, 1, h, wd), device=x.device, dtype=torch.float32)
    ws, nb = _heads_ws(n, h, wd, x.device)
    _lib.check(_lib.load().lwg_heads_forward(_lib.ptr(x), n, h, wd, _lib.ptr(w), int(w.shape[0]), _lib.ptr(color), _lib.ptr(mask),
                                             _lib.ptr(ws), nb, _lib.stream_ptr()))
    return color, mask


@torch.no_grad()
def heads_inference(x, scale_shift, w, precision="bf16x3", bg=None, outputs=("color", "mask", "pred"), bands=0):
    """The inference path's heads on their own (lwg_heads_inference): x (N,H,W,64) RAW, scale_shift (N,64,2), w (>=4,64,7,7),
    bg (1 or N,3,H,W) or None -> dict of the requested outputs: color (N,3,H,W) = tanh, mask (N,1,H,W) = sigmoid of the 7x7 conv of
    relu(x * scale + shift), pred = mask*bg + (1-mask)*color.  bands > 0 forces the bf16x3 kernel's row bands (0: the launcher's
    choice).  Outputs start as NaN, so a pixel the kernel does not write shows."""
    _chk(x, scale_shift, w, bg)
    n, h, wd, c = x.shape
    if c != 64 or tuple(w.shape[1:]) != (64, 7, 7) or tuple(scale_shift.shape) != (n, 64, 2):
        raise RuntimeError("heads_inference: x (N,H,W,64), scale_shift (N,64,2) and w (>=4,64,7,7) expected")
    if bg is not None and (bg.shape[0] not in (1, n) or tuple(bg.shape[1:]) != (3, h, wd)):
        raise RuntimeError("heads_inference: bg (1 or N,3,H,W) expected")
    chans = {"color": 3, "mask": 1, "pred": 3}
    out = {k: torch.full((n, chans[k], h, wd), float("nan"), device=x.device, dtype=torch.float32) for k in outputs}
    lib = _lib.load()
    nb = lib.lwg_heads_inference_workspace_bytes(n, h, wd)
    ws = torch.empty(nb // 4 + 4, device=x.device, dtype=torch.float32)
    _lib.check(lib.lwg_heads_inference(_lib.ptr(x), n, h, wd, _lib.ptr(scale_shift), _lib.ptr(w), int(w.shape[0]),
                                       PRECISIONS[precision], _lib.ptr(bg), 1 if bg is None else int(bg.shape[0]),
                                       _lib.ptr(out.get("color")), _lib.ptr(out.get("mask")), _lib.ptr(out.get("pred")), int(bands),
                                       _lib.ptr(ws), nb, _lib.stream_ptr()))
    return out


@torch.no_grad()
def stem_forward(x, w, precision="bf16x3", with_partials=True, max_workgroups=0):
    """The generator's 7x7 stem on its own (lwg_stem_forward): x (N,H,W,8) NHWC8, w (64,cin,7,7) on the CPU (the entry point packs
    and uploads it), cin <= 6 -> (y (N,H,W,64) raw, partials (N*H*W/128,64,2) = per-tile (mean, M2), or None).  max_workgroups > 0
    caps the persistent grid of the bf16x3 kernel (0: the launcher's choice).  Outputs start as NaN."""
    _chk(x)
    if w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError("stem_forward: w is a contiguous float32 CPU tensor")
    n, h, wd, c = x.shape
    if c != 8 or w.shape[0] != 64 or tuple(w.shape[2:]) != (7, 7):
        raise RuntimeError("stem_forward: x (N,H,W,8) and w (64,cin,7,7) expected")
    y = torch.full((n, h, wd, 64), float("nan"), device=x.device, dtype=torch.float32)
    partials = torch.full((n * h * wd // 128, 64, 2), float("nan"), device=x.device, dtype=torch.float32) if with_partials else None
    _lib.check(_lib.load().lwg_stem_forward(_lib.ptr(x), n, h, wd, _lib.ptr(w), int(w.shape[1]), PRECISIONS[precision], _lib.ptr(y),
                                            _lib.ptr(partials), int(max_workgroups), _lib.stream_ptr()))
    return y, partials


def conv_variant_name(variant):
    """Kernel family name of a variant number (lwg_generator_profile_variant_name)."""
    return _lib.load().lwg_generator_profile_variant_name(int(variant)).decode()


@torch.no_grad()
def norm_conv_forward(x, w, stride=1, pad=0, transposed=False, precision="bf16x3", bn=0, in_scale_shift=None, raw_from=0):
    """One layer of the inference path with its statistics epilogue (lwg_norm_conv_forward): x (N,H,W,Cin) fp32, w in PyTorch
    layout -> (y raw (N,Ho,Wo,Cout), partials (nphase, N*Hm*Wm/128, Cout, 2) = per-tile (mean, M2), variant number).  bn 0: the
    generator's tile-width rule.  in_scale_shift (N, Cin - raw_from, 2): channels >= raw_from of x are raw and normalised by the
    kernel.  Outputs and workspace start as NaN, so an unwritten element shows."""
    _chk(x, w, in_scale_shift)
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    n, h, wd, _ = x.shape
    d = _desc(x.shape, cin, cout, w.shape[2], stride, pad, transposed, precision)
    ho, wo = _out_hw(h, wd, w.shape[2], stride, pad, transposed)
    hm, wm, nphase = (h, wd, 4) if transposed else (ho, wo, 1)
    if in_scale_shift is not None and tuple(in_scale_shift.shape) != (n, cin - raw_from, 2):
        raise RuntimeError("norm_conv_forward: in_scale_shift (N, Cin - raw_from, 2) expected")
    lib = _lib.load()
    nb = lib.lwg_norm_conv_workspace_bytes(ctypes.byref(d))
    if not nb:
        raise _lib.LwgError(-2, lib.lwg_last_error().decode(errors="replace"))
    nan = float("nan")
    ws = torch.full((nb // 4 + 4,), nan, device=x.device, dtype=torch.float32)
    y = torch.full((n, ho, wo, cout), nan, device=x.device, dtype=torch.float32)
    partials = torch.full((nphase, max(n * hm * wm // 128, 1), cout, 2), nan, device=x.device, dtype=torch.float32)
    variant = ctypes.c_int(-1)
    _lib.check(lib.lwg_norm_conv_forward(ctypes.byref(d), _lib.ptr(x), _lib.ptr(w), int(bn), _lib.ptr(in_scale_shift), int(raw_from),
                                         _lib.ptr(y), _lib.ptr(partials), ctypes.byref(variant), _lib.ptr(ws), nb, _lib.stream_ptr()))
    return y, partials, variant.value


@torch.no_grad()
def norm_finalize(partials, n, gamma, beta, eps=1e-5):
    """partials (nphase, mtiles, C, 2) -> scale_shift (N, C, 2) of InstanceNorm2d(affine, eps, biased variance) (lwg_norm_finalize)."""
    _chk(partials, gamma, beta)
    nphase, mtiles, c, two = partials.shape
    if two != 2 or gamma.numel() != c or beta.numel() != c:
        raise RuntimeError("norm_finalize: partials (nphase, mtiles, C, 2), gamma and beta (C,) expected")
    ss = torch.full((n, c, 2), float("nan"), device=partials.device, dtype=torch.float32)
    _lib.check(_lib.load().lwg_norm_finalize(_lib.ptr(partials), nphase, mtiles, int(n), c, _lib.ptr(gamma), _lib.ptr(beta), float(eps),
                                             _lib.ptr(ss), _lib.stream_ptr()))
    return ss


def _slice_ptr(buf, channel_offset):
    return ctypes.c_void_p(buf.data_ptr() + 4 * int(channel_offset))


@torch.no_grad()
def norm_apply(raw, scale_shift, relu=True, dst=None, dst_offset=0, res=None, res_offset=0, split=False, warps=(),
               align_corners=False, lanes=0):
    """The apply pass on its own (lwg_norm_apply): raw (N,H,W,C), scale_shift (N,C,2) -> dst = [relu](raw*scale + shift) [+ res]
    [+ warps].  dst: an (N,H,W,ld_dst) fp32 buffer written at channel offset dst_offset (None: a fresh NaN-filled (N,H,W,C) one);
    res likewise.  split: dst / res hold the split-bf16 format (per 32 channels [32 bf16 hi | 32 bf16 lo] in the same bytes).
    warps: up to two (src (1 or N,H,W,C), flow (N,H,W,2)).  lanes 4 / 8 picks apply_kernel / apply8_kernel.  Returns dst."""
    _chk(raw, scale_shift, dst, res, *[t for wp in warps for t in wp])
    n, h, w, c = raw.shape
    if tuple(scale_shift.shape) != (n, c, 2):
        raise RuntimeError("norm_apply: scale_shift (N,C,2) expected")
    if dst is None:
        dst = torch.full((n, h, w, c), float("nan"), device=raw.device, dtype=torch.float32)
    for t, off in ((dst, dst_offset), (res, res_offset)):
        if t is not None and (tuple(t.shape[:3]) != (n, h, w) or off < 0 or off + c > t.shape[3]):
            raise RuntimeError("norm_apply: dst / res are (N,H,W,ld) buffers holding channels offset .. offset + C")
    if len(warps) > 2:
        raise RuntimeError("norm_apply: at most two warp terms")
    wa = []
    for src, flow in warps:
        if src.shape[0] not in (1, n) or tuple(src.shape[1:]) != (h, w, c) or tuple(flow.shape) != (n, h, w, 2):
            raise RuntimeError("norm_apply: warp terms are (src (1 or N,H,W,C), flow (N,H,W,2))")
        wa += [_lib.ptr(src), int(src.shape[0]), _lib.ptr(flow)]
    wa += [None, 1, None] * (2 - len(warps))
    _lib.check(_lib.load().lwg_norm_apply(_lib.ptr(raw), n, h, w, c, _lib.ptr(scale_shift), int(relu), _slice_ptr(dst, dst_offset),
                                          int(dst.shape[3]), None if res is None else _slice_ptr(res, res_offset),
                                          0 if res is None else int(res.shape[3]), int(split), len(warps), *wa, int(align_corners),
                                          int(lanes), _lib.stream_ptr()))
    return dst


@torch.no_grad()
def heads_backward_weight(x, dy8, out=None):
    """x (N,H,W,64), dy8 (N,H,W,8) (gradient wrt the pre-activation head outputs, channels 4-7 zero) -> dw (8,64,7,7)."""
    _chk(x, dy8)
    n, h, wd, c = x.shape
    if c != 64 or tuple(dy8.shape) != (n, h, wd, 8):
        raise RuntimeError("heads_backward_weight: x (N,H,W,64) and dy8 (N,H,W,8) expected")
    dw = _out(out, (8, 64, 7, 7), x.device)
    ws, nb = _heads_ws(n, h, wd, x.device)
    _lib.check(_lib.load().lwg_heads_backward_weight(_lib.ptr(x), _lib.ptr(dy8), n, h, wd, _lib.ptr(dw), _lib.ptr(ws), nb,
                                                     _lib.stream_ptr()))
    return dw


@torch.no_grad()
def instance_norm_forward(x, gamma, beta, relu=False):
    """x (N,H,W,C) -> (y, stats): F.instance_norm(weight, bias, eps=1e-5) [+ ReLU]; stats (N,C,2) = (mean, rstd)."""
    _chk(x, gamma, beta)
    n, h, w, c = x.shape
    y = torch.empty_like(x)
    stats = torch.empty((n, c, 2), device=x.device, dtype=torch.float32)
    scratch = torch.empty(_lib.load().lwg_instance_norm_scratch_bytes(n, h * w, c) // 8 + 1, device=x.device, dtype=torch.float64)
    _lib.check(_lib.load().lwg_instance_norm_forward(_lib.ptr(x), n, h * w, c, _lib.ptr(gamma), _lib.ptr(beta), int(relu),
                                                     _lib.ptr(y), _lib.ptr(stats), _lib.ptr(scratch), _lib.stream_ptr()))
    return y, stats


@torch.no_grad()
def instance_norm_backward(x, y, dy, stats, gamma, out_dgamma=None, out_dbeta=None):
    """-> (dx, dgamma, dbeta); pass y (the forward output) when the forward applied the ReLU, else None."""
    _chk(x, y, dy, stats, gamma)
    n, h, w, c = x.shape
    dx = torch.empty_like(x)
    dgamma = _out(out_dgamma, (c,), x.device)
    dbeta = _out(out_dbeta, (c,), x.device)
    scratch = torch.empty(_lib.load().lwg_instance_norm_scratch_bytes(n, h * w, c) // 8 + 1, device=x.device, dtype=torch.float64)
    _lib.check(_lib.load().lwg_instance_norm_backward(_lib.ptr(x), _lib.ptr(y), _lib.ptr(dy), _lib.ptr(stats), _lib.ptr(gamma), n,
                                                      h * w, c, _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(scratch),
                                                      _lib.stream_ptr()))
    return dx, dgamma, dbeta


class GridSamplePlan(object):
    """The scatter of one flow field turned into per-texel contribution lists in a fixed order (lwg_grid_sample_plan): built once
    per (grid, source shape), applied to any number of gradient tensors of that shape (any channel count)."""

    def __init__(self, grid, x_shape, align_corners=False):
        _chk(grid)
        lib = _lib.load()
        self.xn, self.h, self.w = int(x_shape[0]), int(x_shape[1]), int(x_shape[2])
        self.n, self.ho, self.wo = int(grid.shape[0]), int(grid.shape[1]), int(grid.shape[2])
        nbytes = lib.lwg_grid_sample_plan_bytes(self.xn, self.h, self.w, self.n, self.ho, self.wo)
        if not nbytes:
            raise ValueError("grid_sample plan: bad dimensions %s for a grid of %s" % (tuple(x_shape), tuple(grid.shape)))
        self.buf = torch.empty(nbytes // 4, device=grid.device, dtype=torch.int32)
        self.nbytes = nbytes
        _lib.check(lib.lwg_grid_sample_plan(_lib.ptr(grid), self.xn, self.h, self.w, self.n, self.ho, self.wo, int(align_corners),
                                            _lib.ptr(self.buf), nbytes, _lib.stream_ptr()))

    def matches(self, x_shape, dy_shape):
        return (int(x_shape[0]), int(x_shape[1]), int(x_shape[2])) == (self.xn, self.h, self.w) and \
            tuple(int(v) for v in dy_shape[:3]) == (self.n, self.ho, self.wo)


@torch.no_grad()
def grid_sample_backward(dy, grid, x_shape, align_corners=False, plan=None, deterministic=True):
    """Gradient of F.grid_sample(x, grid) (bilinear, zeros) wrt x: dy (n,Ho,Wo,C) NHWC, grid (n,Ho,Wo,2) -> dx of NHWC
    shape x_shape (xn,H,W,C), xn in {1, n} (1: one source shared by the batch, gradients summed).  Deterministic (default): a
    gather over a GridSamplePlan (pass `plan` to share one between the warps of a pyramid level), contributions added in a fixed
    order -- bit-reproducible; deterministic=False: one scatter kernel with float atomics (what torch does)."""
    _chk(dy, grid)
    xn, h, w, c = x_shape
    n, ho, wo, _ = dy.shape
    dx = torch.zeros(tuple(x_shape), device=dy.device, dtype=torch.float32)
    if not deterministic:
        _lib.check(_lib.load().lwg_grid_sample_backward(_lib.ptr(dy), _lib.ptr(grid), xn, c, h, w, n, ho, wo, int(align_corners),
                                                        _lib.ptr(dx), _lib.stream_ptr()))
        return dx
    if plan is None:
        plan = GridSamplePlan(grid, x_shape, align_corners)
    elif not plan.matches(x_shape, dy.shape):
        raise ValueError("grid_sample_backward: the plan was built for other dimensions")
    _lib.check(_lib.load().lwg_grid_sample_backward_planned(_lib.ptr(dy), c, xn, h, w, n, ho, wo, _lib.ptr(plan.buf), plan.nbytes,
                                                            _lib.ptr(dx), _lib.stream_ptr()))
    return dx


@torch.no_grad()
def adam_update(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """In-place torch.optim.Adam step on flat (contiguous) tensors."""
    _chk(param, grad, exp_avg, exp_avg_sq)
    _lib.check(_lib.load().lwg_adam_update(_lib.ptr(param), _lib.ptr(grad), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), param.numel(),
                                           int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), _lib.stream_ptr()))


def adam_step_state(step=0, betas=(0.9, 0.999), device="cuda"):
    """The device-resident step state of adam_update_device_step after `step` steps: int64 tensor of three words
    [t, bits of float64(beta1^t), bits of float64(beta2^t)] (include/lwg.h)."""
    import numpy as np
    pows = np.array([float(betas[0]) ** int(step), float(betas[1]) ** int(step)], dtype=np.float64).view(np.int64)
    return torch.tensor([int(step), int(pows[0]), int(pows[1])], dtype=torch.int64, device=device)


def adam_update_device_step(param, grad, exp_avg, exp_avg_sq, step_state, lr, betas=(0.9, 0.999), eps=1e-8):
    """adam_update with the step count in `step_state` (adam_step_state(); advanced by the call on the stream): the form that
    can be captured in a graph and replayed (include/lwg.h, lwg_adam_update_device_step).  `int(step_state[0])` is the count."""
    _chk(param, grad, exp_avg, exp_avg_sq)
    if not step_state.is_cuda or step_state.dtype != torch.int64 or step_state.numel() != 3 or not step_state.is_contiguous():
        raise RuntimeError("adam_update_device_step: step_state must be adam_step_state(): three int64 words on the device")
    _lib.check(_lib.load().lwg_adam_update_device_step(_lib.ptr(param), _lib.ptr(grad), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                                       param.numel(), _lib.ptr(step_state), float(lr), float(betas[0]), float(betas[1]),
                                                       float(eps), _lib.stream_ptr()))


def adam_update_scheduled(param, grad, exp_avg, exp_avg_sq, step_state, lr_table, betas=(0.9, 0.999), eps=1e-8):
    """adam_update_device_step with the learning rate on the device as well: `lr_table` (float32, one rate per step) is read by
    the kernel at lr_table[min(t, len) - 1] for the advanced count t (include/lwg.h, lwg_adam_update_scheduled) -- a captured
    iteration replays through a decaying rate without being captured again."""
    _chk(param, grad, exp_avg, exp_avg_sq, lr_table)
    if not step_state.is_cuda or step_state.dtype != torch.int64 or step_state.numel() != 3 or not step_state.is_contiguous():
        raise RuntimeError("adam_update_scheduled: step_state must be adam_step_state(): three int64 words on the device")
    if lr_table.dim() != 1 or lr_table.numel() < 1:
        raise RuntimeError("adam_update_scheduled: lr_table must be a non-empty 1-d float32 tensor")
    _lib.check(_lib.load().lwg_adam_update_scheduled(_lib.ptr(param), _lib.ptr(grad), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                                     param.numel(), _lib.ptr(step_state), _lib.ptr(lr_table), lr_table.numel(),
                                                     float(betas[0]), float(betas[1]), float(eps), _lib.stream_ptr()))


@torch.no_grad()
def grid_sample_nhwc(x, grid, align_corners=False):
    """F.grid_sample (bilinear, zeros) on NHWC tensors: x (xn,H,W,C) with xn in {1, n}, grid (n,Ho,Wo,2) -> (n,Ho,Wo,C)."""
    _chk(x, grid)
    xn, h, w, c = x.shape
    n, ho, wo, _ = grid.shape
    y = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().lwg_grid_sample_nhwc(_lib.ptr(x), xn, c, h, w, _lib.ptr(grid), n, ho, wo, int(align_corners), _lib.ptr(y),
                                                _lib.stream_ptr()))
    return y


def crop_boxes(boxes, n, size, device):
    """The (n,4) int64 device tensor lwg_crop_resize reads, rows (min_x, max_x, min_y, max_y) with exclusive ends.  A CUDA tensor
    goes through untouched (nothing is read back: the call stays asynchronous and capturable; the kernel clamps to the image).
    A CPU tensor or a list is validated here -- shape (n,4), integers, 0 <= min <= max <= size -- and then copied over."""
    if torch.is_tensor(boxes) and boxes.is_cuda:
        if tuple(boxes.shape) != (n, 4) or boxes.dtype != torch.int64 or not boxes.is_contiguous():
            raise ValueError("boxes on the device must be a contiguous int64 tensor of shape (%d, 4)" % n)
        return boxes
    b = boxes if torch.is_tensor(boxes) else torch.as_tensor(boxes)
    if tuple(b.shape) != (n, 4):
        raise ValueError("boxes must have shape (%d, 4), got %s" % (n, tuple(b.shape)))
    if b.dtype.is_floating_point or b.dtype.is_complex or b.dtype == torch.bool:
        raise ValueError("boxes must be integers, got %s" % b.dtype)
    b = b.to(torch.int64)
    lo, hi = b[:, 0::2], b[:, 1::2]
    if bool((lo < 0).any()) or bool((hi > size).any()) or bool((lo > hi).any()):
        raise ValueError("boxes must satisfy 0 <= min <= max <= %d per axis (min_x, max_x, min_y, max_y), got %s"
                         % (size, b.tolist()))
    return b.contiguous().to(device)


def _crop_args(x, boxes):
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError("crop_resize takes square (n,C,S,S) NCHW images, got %s" % (tuple(x.shape),))
    if not (torch.is_tensor(boxes) and boxes.is_cuda):
        crop_boxes(boxes, x.shape[0], x.shape[2], "cpu")   # a bad box is refused before anything touches the device
    _chk(x)
    return crop_boxes(boxes, x.shape[0], x.shape[2], x.device)


@torch.no_grad()
def crop_resize(x, boxes):
    """GlobalLocalDiscriminator.crop_body (networks/discriminator.py:80-96): x (n,C,S,S) NCHW, boxes (n,4) -> each sample's box
    resampled to (S,S), bilinear with align_corners=True.  An empty box gives zeros (include/lwg.h, lwg_crop_resize)."""
    b = _crop_args(x, boxes)
    out = torch.empty_like(x)
    _lib.check(_lib.load().lwg_crop_resize(_lib.ptr(x), x.shape[0], x.shape[1], x.shape[2], _lib.ptr(b), _lib.ptr(out),
                                           _lib.stream_ptr()))
    return out


@torch.no_grad()
def crop_resize_backward(dy, boxes):
    """The adjoint of crop_resize: dy (n,C,S,S) -> dx (n,C,S,S), zero outside each box; deterministic (no atomics)."""
    b = _crop_args(dy, boxes)
    dx = torch.empty_like(dy)
    _lib.check(_lib.load().lwg_crop_resize_backward(_lib.ptr(dy), dy.shape[0], dy.shape[1], dy.shape[2], _lib.ptr(b), _lib.ptr(dx),
                                                    _lib.stream_ptr()))
    return dx
