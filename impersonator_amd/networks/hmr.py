"""HMR: image -> SMPL vector (cam 3, pose 72, shape 10) with the reference's module surface (networks/hmr.py:65-330).

`HumanModelRecovery` here is the FULL class: the pre-activation ResNet-50 (v2), the global average pool and the 3-iteration
`ThetaRegressor`, with the reference's `state_dict` keys and shapes, so that `load_state_dict(torch.load('hmr_tf2pt.pth'))`
works as at models/imitator.py:69-74.  It extends the light class of `batch_smpl.py` (`get_details`, `get_details_swapped`,
`smpl`), which stays what the synthetic configuration and most tests construct.

CUDA input runs liblwg (csrc/hmr.hip: exact fp32 MFMA, BatchNorm folded into the convolutions' prologues and epilogues, no
framework kernel, capturable in a HIP graph); CPU input runs `forward_ops`, the same network as tensor ops in the reference's
order -- the CPU path and the test oracle.  Eval mode only: batch statistics and dropout are not implemented.
"""
import ctypes
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from . import batch_smpl

IMAGE_SIZE = 224
NUM_BLOCKS = (3, 4, 6, 3)


def subsample(inputs, factor):
    """hmr.py:21-35."""
    return inputs if factor == 1 else F.max_pool2d(inputs, [1, 1], stride=factor)


class PreActBottleneck(nn.Module):
    """hmr.py:65-116."""
    expansion = 4

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, self.expansion * planes, kernel_size=1, bias=True)
        self.stride = stride
        if in_planes != self.expansion * planes:
            self.shortcut = nn.Sequential(nn.Conv2d(in_planes, self.expansion * planes, kernel_size=1, stride=stride, bias=True))

    def forward(self, x):
        preact = F.relu(self.bn1(x))
        shortcut_out = self.shortcut(preact) if hasattr(self, 'shortcut') else subsample(x, factor=self.stride)
        conv1_out = F.relu(self.bn2(self.conv1(preact)))
        conv2_out = F.relu(self.bn3(self.conv2(conv1_out)))
        conv3_out = self.conv3(conv2_out)
        return conv3_out + shortcut_out


class PreActResNet(nn.Module):
    """hmr.py:119-165."""

    def __init__(self, block, num_blocks):
        super().__init__()
        self.in_planes = 64
        self.num_blocks = tuple(int(n) for n in num_blocks)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=True)
        self.layer1 = self._make_layer(block, 64, num_blocks[0], stride=2)
        self.layer2 = self._make_layer(block, 128, num_blocks[1], stride=2)
        self.layer3 = self._make_layer(block, 256, num_blocks[2], stride=2)
        self.layer4 = self._make_layer(block, 512, num_blocks[3], stride=1)
        self.post_bn = nn.BatchNorm2d(2048)

    def _make_layer(self, block, planes, num_blocks, stride):
        layers = [block(self.in_planes, planes, 1)]
        self.in_planes = planes * block.expansion
        for i in range(1, num_blocks):
            layers.append(block(self.in_planes, planes, stride=stride if i == num_blocks - 1 else 1))
        return nn.Sequential(*layers)

    def forward(self, x):
        out = self.conv1(x)
        out = F.max_pool2d(out, kernel_size=3, stride=2, ceil_mode=True)
        out = self.layer4(self.layer3(self.layer2(self.layer1(out))))
        out = F.relu(self.post_bn(out))
        out = F.avg_pool2d(out, 7)
        return out.view(out.size(0), -1)


def preActResNet50(num_blocks=NUM_BLOCKS):
    return PreActResNet(PreActBottleneck, list(num_blocks))


class ThetaRegressor(nn.Module):
    """hmr.py:213-252.  `mean_theta` arrives through the state_dict (the reference reads it from an h5 file only when it
    converts the TensorFlow checkpoint)."""

    def __init__(self, input_dim, out_dim, iterations=3):
        super().__init__()
        self.iterations = iterations
        mean = torch.zeros(out_dim, dtype=torch.float32)
        mean[0] = 0.9                                        # hmr.py:207-208
        self.register_buffer('mean_theta', mean)
        fc_blocks = OrderedDict()
        fc_blocks['fc1'] = nn.Linear(input_dim, 1024, bias=True)
        fc_blocks['relu1'] = nn.ReLU()
        fc_blocks['dropout1'] = nn.Dropout(p=0.5)
        fc_blocks['fc2'] = nn.Linear(1024, 1024, bias=True)
        fc_blocks['relu2'] = nn.ReLU()
        fc_blocks['dropout2'] = nn.Dropout(p=0.5)
        fc_blocks['fc3'] = nn.Linear(1024, out_dim, bias=True)
        nn.init.xavier_normal_(fc_blocks['fc3'].weight, gain=0.1)
        nn.init.zeros_(fc_blocks['fc3'].bias)
        self.fc_blocks = nn.Sequential(fc_blocks)

    def forward(self, x):
        theta = self.mean_theta.repeat(x.shape[0], 1)
        for _ in range(self.iterations):
            theta = theta + self.fc_blocks(torch.cat([x, theta], dim=1))
        return theta


def fold_batchnorm(bn):
    """Eval-mode BatchNorm as y = x * scale + shift: scale = gamma / sqrt(var + eps), shift = beta - mean * scale, computed
    in fp64 from the fp32 tensors and rounded once.  -> (scale, shift) fp32 on the CPU."""
    g, b, m, v = (t.detach().double().cpu() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    scale = g / torch.sqrt(v + bn.eps)
    shift = b - m * scale
    return scale.float(), shift.float()


def _conv_matrix(conv):
    """(Cout,Cin,k,k) -> [kh][kw][ci][co], the kernel's reduction-major layout."""
    return conv.weight.detach().float().cpu().permute(2, 3, 1, 0).contiguous().reshape(-1)


def pack_weights(resnet, regressor):
    """Everything `lwg_hmr_set_weights` takes, as one flat fp32 CPU tensor in the order include/lwg.h documents."""
    f = lambda t: t.detach().float().cpu().contiguous().reshape(-1)
    parts = [_conv_matrix(resnet.conv1), f(resnet.conv1.bias)]
    for layer in (resnet.layer1, resnet.layer2, resnet.layer3, resnet.layer4):
        for blk in layer:
            parts += list(fold_batchnorm(blk.bn1)) + [_conv_matrix(blk.conv1)]
            parts += list(fold_batchnorm(blk.bn2)) + [_conv_matrix(blk.conv2)]
            parts += list(fold_batchnorm(blk.bn3)) + [_conv_matrix(blk.conv3), f(blk.conv3.bias)]
            if hasattr(blk, 'shortcut'):
                parts += [_conv_matrix(blk.shortcut[0]), f(blk.shortcut[0].bias)]
    parts += list(fold_batchnorm(resnet.post_bn))
    fc = regressor.fc_blocks
    parts += [f(regressor.mean_theta), f(fc.fc1.weight), f(fc.fc1.bias), f(fc.fc2.weight), f(fc.fc2.bias), f(fc.fc3.weight),
              f(fc.fc3.bias)]
    return torch.cat(parts).contiguous()


class HumanModelRecovery(batch_smpl.HumanModelRecovery):
    """hmr.py:255-330.  Extensions: `smpl_params` (a synthetic body model instead of the pickle), `num_blocks` (a reduced
    ResNet for tests), `max_batch` (images per device launch sequence; larger batches are chunked)."""

    def __init__(self, smpl_pkl_path=None, feature_dim=2048, theta_dim=85, iterations=3, smpl_params=None,
                 num_blocks=NUM_BLOCKS, max_batch=8):
        nn.Module.__init__(self)
        if feature_dim != 2048 or theta_dim != 85 or iterations != 3:
            raise ValueError("the device regressor is built for feature_dim 2048, theta_dim 85, 3 iterations")
        # attribute order = the reference's state_dict order: resnet.*, smpl.*, regressor.*
        self.resnet = preActResNet50(num_blocks)
        self.smpl = batch_smpl.SMPL(smpl_pkl_path, params=smpl_params)
        self.feature_dim, self.theta_dim, self.iterations = feature_dim, theta_dim, iterations
        self.regressor = ThetaRegressor(feature_dim + theta_dim, theta_dim, iterations)
        self.max_batch = max(1, int(max_batch))
        self._handle = None
        self._uploaded_version = None

    # ------------------------------------------------------------------ handle / weights
    def _weights_version(self):
        tensors = list(self.resnet.parameters()) + list(self.resnet.buffers()) + list(self.regressor.parameters()) + \
            list(self.regressor.buffers())
        return tuple(t._version for t in tensors) + tuple(id(t) for t in tensors)

    def _ensure_handle(self):
        lib = _lib.load()
        if self._handle is None:
            h = ctypes.c_void_p()
            nb = (ctypes.c_int * 4)(*self.resnet.num_blocks)
            _lib.check(lib.lwg_hmr_create(ctypes.byref(h), self.max_batch, nb))
            self._handle = h
            self._uploaded_version = None
        ver = self._weights_version()
        if self._uploaded_version != ver:
            blob = pack_weights(self.resnet, self.regressor)
            _lib.check(lib.lwg_hmr_set_weights(self._handle, ctypes.c_void_p(blob.data_ptr()), blob.numel()))
            self._uploaded_version = ver
        return self._handle

    def release(self):
        if self._handle is not None:
            _lib.load().lwg_hmr_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # ------------------------------------------------------------------ forward
    def _check_input(self, inputs):
        if self.training:
            raise RuntimeError("HumanModelRecovery runs in eval mode only (BatchNorm running statistics, no dropout); call .eval()")
        if not torch.is_tensor(inputs) or inputs.dim() != 4 or tuple(inputs.shape[1:]) != (3, IMAGE_SIZE, IMAGE_SIZE):
            raise ValueError("HumanModelRecovery takes images of shape (N, 3, %d, %d), got %s"
                             % (IMAGE_SIZE, IMAGE_SIZE, tuple(inputs.shape) if torch.is_tensor(inputs) else type(inputs)))
        if inputs.dtype != torch.float32:
            raise TypeError("HumanModelRecovery takes float32 images in [-1, 1], got %s" % inputs.dtype)

    def forward(self, inputs, return_features=False):
        """hmr.py:276-300: images (N,3,224,224) in [-1,1] -> thetas (N,85) [, features (N,2048)]."""
        self._check_input(inputs)
        if inputs.is_cuda:
            return self.forward_device(inputs, return_features)
        return self.forward_ops(inputs, return_features)

    def forward_ops(self, inputs, return_features=False):
        """The reference's own sequence of tensor ops (any device, any float dtype the module was cast to)."""
        out = self.resnet.conv1(inputs)
        out = F.max_pool2d(out, kernel_size=3, stride=2, ceil_mode=True)
        out = self.resnet.layer1(out)
        out = self.resnet.layer2(out)
        out = self.resnet.layer3(out)
        out = self.resnet.layer4(out)
        out = F.relu(self.resnet.post_bn(out))
        out = F.avg_pool2d(out, 7)
        features = out.view(out.size(0), -1)
        thetas = self.regressor(features)
        return (thetas, features) if return_features else thetas

    @torch.no_grad()
    def forward_device(self, inputs, return_features=False):
        h = self._ensure_handle()
        lib = _lib.load()
        x = inputs.contiguous()
        n = x.shape[0]
        thetas = torch.empty((n, self.theta_dim), device=x.device, dtype=torch.float32)
        feats = torch.empty((n, self.feature_dim), device=x.device, dtype=torch.float32) if return_features else None
        st = _lib.stream_ptr()
        for s in range(0, n, self.max_batch):
            e = min(n, s + self.max_batch)
            _lib.check(lib.lwg_hmr_forward(h, _lib.ptr(x[s:e]), e - s, IMAGE_SIZE, IMAGE_SIZE, _lib.ptr(thetas[s:e]),
                                           _lib.ptr(feats[s:e]) if return_features else None, st))
        return (thetas, feats) if return_features else thetas


def load_checkpoint(hmr, path):
    """models/imitator.py:69-74 (`hmr.load_state_dict(torch.load(opt.hmr_model))`), accepting DataParallel's `module.` prefix.
    A checkpoint without `smpl.*` entries (one written from `utils.synthetic.hmr_state_dict`) keeps the module's body model."""
    saved = torch.load(path, map_location='cpu')
    sd = OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in saved.items())
    if not any(k.startswith('smpl.') for k in sd):
        for k, v in hmr.smpl.state_dict().items():
            sd['smpl.' + k] = v
    hmr.load_state_dict(sd)
    return hmr
