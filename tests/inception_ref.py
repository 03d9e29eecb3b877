"""The evaluator's InceptionV3 restated as a plain torch.nn module (usable in fp32 and fp64, on any device), its preprocessing,
and the host metric functions' oracle -- what the reference computes in thirdparty/his_evaluators/.../metrics/metrics.py:16-158
(torchvision's inception_v3 cut at the final average pool), 634-781 (FIDMetric, InceptionScoreMetric) and 309-395
(calculate_frechet_distance, fid_score_func, is_score_func), in this project's own words.  torchvision is not needed."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from scipy import linalg

BN_EPS = 1e-3


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1)      # count_include_pad=True: divides by 9 everywhere


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), self.branch_pool(_avg(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        d = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        return torch.cat([self.branch1x1(x), b7, d, self.branch_pool(_avg(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        d = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(b3), self.branch3x3_2b(b3), self.branch3x3dbl_3a(d),
                          self.branch3x3dbl_3b(d), self.branch_pool(_avg(x))], 1)


STAGES = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2",
          "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
          "Mixed_7c")


class InceptionFeatures(nn.Module):
    """inception_v3 up to the global average pool, with torchvision's module names (so its state_dict keys load as they are);
    `transform_input`, AuxLogits and fc do not exist here, as the reference never runs them"""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)

    def forward(self, x, stages=None):
        """-> (N,2048); `stages`: a list that receives the 18 stage outputs (NCHW) in the order of STAGES"""
        for name in STAGES:
            x = F.max_pool2d(x, kernel_size=3, stride=2) if name.startswith("maxpool") else getattr(self, name)(x)
            if stages is not None:
                stages.append(x)
        return F.adaptive_avg_pool2d(x, 1)[:, :, 0, 0]


def build(state_dict, dtype=torch.float64, device="cpu"):
    """the module in eval mode with the state_dict's tensors (numpy arrays or tensors; AuxLogits.*, fc.* ignored)"""
    net = InceptionFeatures()
    own = net.state_dict()
    net.load_state_dict({k: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v) for k, v in state_dict.items() if k in own})
    return net.to(device=device, dtype=dtype).eval()


def preprocess(frames, size=299):
    """metrics.py:645-669 / 715-740 on [0,1] frames: `out *= 2; out -= 1`, then the bilinear resize; size 0: no resize.  In the
    dtype of `frames`."""
    out = frames.clone()
    out *= 2
    out -= 1
    if size:
        out = F.interpolate(out, size=(size, size), mode="bilinear", align_corners=False)
    return out


# ------------------------------------------------------------------------------------------------ host metrics, fp64
def frechet_distance(mu1, s1, mu2, s2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + Tr(s1 + s2 - 2 sqrt(s1 s2)), with the reference's two escapes: a non-finite square root is taken
    again with eps on both diagonals; a complex one is accepted when its diagonal is real to 1e-3 and its real part is used"""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    s1, s2 = np.atleast_2d(s1), np.atleast_2d(s2)
    assert mu1.shape == mu2.shape and s1.shape == s2.shape
    diff = mu1 - mu2
    root, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(root).all():
        off = np.eye(s1.shape[0]) * eps
        root = linalg.sqrtm((s1 + off).dot(s2 + off))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component %g" % np.max(np.abs(root.imag)))
        root = root.real
    return diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(root)


def fid(a, b):
    if len(a) == 0 or len(b) == 0:
        return 0
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return frechet_distance(np.mean(a, axis=0), np.cov(a, rowvar=False), np.mean(b, axis=0), np.cov(b, rowvar=False))


def softmax(features):
    """over the 2048 pool features, as the reference does with output_blocks=[3]"""
    return F.softmax(torch.as_tensor(np.asarray(features, np.float64)), dim=1).numpy()


def is_of_batch(probs):
    kl = probs * (np.log(probs) - np.log(np.expand_dims(np.mean(probs, 0), 0)))
    return np.exp(np.mean(np.sum(kl, 1)))


def inception_score(features, batch_size=32):
    features = np.asarray(features, np.float64)
    scores = [is_of_batch(softmax(features[i * batch_size:(i + 1) * batch_size]))
              for i in range(int(math.ceil(len(features) / batch_size)))]
    return np.mean(scores), np.std(scores)


# ------------------------------------------------------------------------------------------------ the whole-network cases
SEED = 0
CASES = (("raw_107x91", 3, 107, 91, 0), ("resized_64x48", 1, 64, 48, 299))     # (name, n, H, W, resize)


def case_frames(index):
    """[0,1] frames of a case: smooth images (utils/synthetic.smooth_image) mapped from [-1,1]"""
    from impersonator_amd.utils import synthetic
    _, n, h, w, _ = CASES[index]
    return ((synthetic.smooth_image(500 + index, (n, 3, h, w)).astype(np.float64) + 1) / 2).astype(np.float32)
