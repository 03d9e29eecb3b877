"""Paired evaluation on the device: SSIM, PSNR, LPIPS and the scale-shape-pose error of generated frames against ground truth,
the paired protocol of the reference's evaluate.py (thirdparty/his_evaluators/.../metrics/metrics.py: SSIMMetric, PSNRMetric,
PerceptualMetric, ScaleShapePoseError) over csrc/eval.hip and csrc/lpips.hip.  No float frame goes to the host: a frame leaves
the device as four fp64 numbers (plus three for SSPE, plus one for LPIPS).  There is no CPU fallback; a missing kernel is an error.

The arithmetic is stated in include/lwg.h (lwg_eval_pair_stats); tests/metrics_ref.py restates it in numpy.

Set metrics, for the protocols without a ground-truth frame: FID and Inception Score (FIDMetric, InceptionScoreMetric of the same
file) from InceptionV3 features computed on the device (csrc/inception.hip) -- SetEvaluator, FIDMetric, InceptionScoreMetric and
the host-side fp64 functions frechet_distance, fid_from_features, inception_score at the end of this module.
"""
import math

import numpy as np
import torch

from .. import _lib
from ..ops import _chk

HMR_SIZE = 224


def _mode(mode):
    if mode not in (0, 1, 2):
        raise ValueError("mode must be 0 ([-1,1] as it is), 1 ([0,1] input) or 2 ([-1,1] through 8 bits), got %r" % (mode,))
    return int(mode)


@torch.no_grad()
def pair_stats(pred, ref, mode=0, out=None):
    """pred, ref (N,3,H,W) contiguous float32 CUDA tensors -> (N,4) float64 CUDA tensor [mssim, mse, ref_min, ref_max] per frame.
    mode 0: values in [-1,1] as they are; 1: values in [0,1], mapped 2*x-1 as the reference's `preprocess` does; 2: values in
    [-1,1] passed through the 8 bits the frame writer (cv_utils.save_cv2_img, truncating) and the evaluator's loader put between
    generator and metric -- the quantisation only: JPEG loss is not modelled.
    Only launches: no synchronisation.  `out`: an (N,4) float64 row block to write into (PairedEvaluator's device-side rows)."""
    _chk(pred, ref)
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != ref.shape:
        raise ValueError("pair_stats takes two (N,3,H,W) tensors of one shape, got %s and %s" % (tuple(pred.shape), tuple(ref.shape)))
    n, _, h, w = pred.shape
    lib = _lib.load()
    stats = out if out is not None else torch.empty((n, 4), device=pred.device, dtype=torch.float64)
    if tuple(stats.shape) != (n, 4) or stats.dtype != torch.float64 or not stats.is_contiguous() or not stats.is_cuda:
        raise ValueError("out must be a contiguous (N,4) float64 CUDA tensor")
    nbytes = lib.lwg_eval_workspace_bytes(n, h, w)
    ws = torch.empty(max(nbytes, 8), device=pred.device, dtype=torch.uint8)
    _lib.check(lib.lwg_eval_pair_stats(_lib.ptr(pred), _lib.ptr(ref), n, h, w, _mode(mode), _lib.ptr(stats), _lib.ptr(ws), nbytes,
                                       _lib.stream_ptr()))
    return stats


@torch.no_grad()
def resize_bilinear(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) for a contiguous float32 CUDA (N,C,H,W) tensor."""
    _chk(x)
    if x.dim() != 4:
        raise ValueError("resize_bilinear takes an (N,C,H,W) tensor, got %s" % (tuple(x.shape),))
    ho, wo = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    n, c, h, w = x.shape
    y = torch.empty((n, c, ho, wo), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().lwg_resize_bilinear(_lib.ptr(x), n, c, h, w, ho, wo, _lib.ptr(y), _lib.stream_ptr()))
    return y


@torch.no_grad()
def sspe_terms(a, b, out=None):
    """a, b (N,85) contiguous float32 CUDA SMPL vectors -> (N,3) float64 CUDA tensor: |d[0]|, sum |d[75:85]|, sum |d[0:75]|
    of d = a - b per frame (the reference's scale, shape and pose terms; its "pose" slice covers the three camera values again)."""
    _chk(a, b)
    if a.dim() != 2 or a.shape[1] != 85 or a.shape != b.shape:
        raise ValueError("sspe_terms takes two (N,85) tensors, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    n = a.shape[0]
    terms = out if out is not None else torch.empty((n, 3), device=a.device, dtype=torch.float64)
    if tuple(terms.shape) != (n, 3) or terms.dtype != torch.float64 or not terms.is_contiguous() or not terms.is_cuda:
        raise ValueError("out must be a contiguous (N,3) float64 CUDA tensor")
    _lib.check(_lib.load().lwg_eval_sspe_terms(_lib.ptr(a), _lib.ptr(b), n, _lib.ptr(terms), _lib.stream_ptr()))
    return terms


def psnr_from_stats(stats):
    """Host, fp64: (N,4) rows of pair_stats -> (N,) PSNR as scikit-image 0.16.2's peak_signal_noise_ratio gives it for float
    images without a data_range: 1 when the reference image has no negative value, else 2; +inf for identical images.
    ValueError when the reference image leaves [-1,1] (scikit-image raises there)."""
    stats = np.asarray(stats, np.float64).reshape(-1, 4)
    out = np.empty(len(stats), np.float64)
    for i, (_, mse, lo, hi) in enumerate(stats):
        if lo < -1 or hi > 1:
            raise ValueError("im_true has intensity values outside the range expected for its data type: [%g, %g] (frame %d)"
                             % (lo, hi, i))
        data_range = 1.0 if lo >= 0 else 2.0
        out[i] = math.inf if mse == 0 else 10.0 * math.log10(data_range * data_range / mse)
    return out


def _as_batch(x):
    """a list of (3,H,W) tensors (what the reference's calculate_score iterates over) is stacked; a tensor passes through"""
    if not torch.is_tensor(x):
        x = torch.stack(list(x))
    return x


class BaseMetric(object):
    LOWER, HIGHER = "lower", "higher"


class SSIMMetric(BaseMetric):
    """metrics.py:450-507.  preds, gts: (N,3,H,W) images in [0,1] on the device (mode 1 maps them to [-1,1])."""

    def calculate_score(self, preds, gts):
        stats = pair_stats(_as_batch(preds), _as_batch(gts), mode=1)
        return float(np.mean(stats[:, 0].cpu().numpy()))

    def quality(self):
        return self.HIGHER


class PSNRMetric(BaseMetric):
    """metrics.py:510-566.  preds, gts: (N,3,H,W) images in [0,1] on the device."""

    def calculate_score(self, preds, gts):
        stats = pair_stats(_as_batch(preds), _as_batch(gts), mode=1)
        return float(np.mean(psnr_from_stats(stats.cpu().numpy())))

    def quality(self):
        return self.HIGHER


class ScaleShapePoseError(BaseMetric):
    """metrics.py:1048-1111 with the regressor on the device: `hmr` is a networks.hmr.HumanModelRecovery.  preds, gts:
    (N,3,H,W) images in [0,1] as the reference's take them (`unit=False`: already in [-1,1], what the generator emits)."""

    def __init__(self, hmr, unit=True):
        if hmr is None or not hasattr(hmr, "regressor"):
            raise ValueError("ScaleShapePoseError needs the HMR regressor (networks.hmr.HumanModelRecovery)")
        self.hmr, self.unit = hmr, bool(unit)

    @torch.no_grad()
    def thetas(self, x):
        """(N,3,H,W) -> (N,85): resize to 224x224 (F.interpolate, bilinear, align_corners=False), then the regressor"""
        x = _as_batch(x)
        _chk(x)
        if self.unit:
            x = x * 2 - 1             # metrics.py:1069-1071, two float32 roundings
        if tuple(x.shape[-2:]) != (HMR_SIZE, HMR_SIZE):
            x = resize_bilinear(x, (HMR_SIZE, HMR_SIZE))
        return self.hmr(x)

    def terms(self, preds, gts, out=None):
        """device-side (N,3) float64 rows [scale, shape, pose]; only launches"""
        return sspe_terms(self.thetas(preds), self.thetas(gts), out=out)

    def calculate_score(self, preds, gts):
        t = self.terms(preds, gts).cpu().numpy()
        return float(t[:, 0].mean() + t[:, 1].mean() + t[:, 2].mean())

    def quality(self):
        return self.LOWER


class PerceptualMetric(BaseMetric):
    """metrics.py:569-640 with the network on the device: `lpips` is a networks.lpips.LPIPS (AlexNet, v0.1).  preds, gts:
    (N,3,H,W) images in [0,1] on the device (mode 1 maps them to [-1,1], as the reference's `preprocess` does)."""

    def __init__(self, lpips):
        if lpips is None or not callable(lpips) or not hasattr(lpips, "max_batch"):
            raise ValueError("PerceptualMetric needs the LPIPS model (networks.lpips.LPIPS)")
        self.lpips = lpips

    def calculate_score(self, preds, gts):
        return float(np.mean(self.lpips(_as_batch(preds), _as_batch(gts), mode=1).cpu().numpy()))

    def quality(self):
        return self.LOWER


class PairedEvaluator(object):
    """Scores a sequence batch by batch without leaving the device.

        ev = PairedEvaluator(("ssim", "psnr"))            # frames in [-1,1] as the generator emits them (mode 0)
        for t, preds in imitator.predict_batches(...):
            ev.update(preds, ground_truth[t:t + len(preds)])
        print(ev.result())

    `update` only launches kernels: it writes the batch's rows into a device-side table (grown by doubling) and makes no
    `.cpu()`, `.item()` or synchronisation call, so it can sit inside the imitation loop.  `result()` makes ONE device->host copy
    and returns per-frame arrays and their means over frames.  The reference averages per-batch means instead
    (BaseMetric.calculate_score over a loader, PerceptualMetric.calculate_score in batches of 32 -- LPIPS included); the two
    agree whenever the frame count is a multiple of the batch size.
    mode: 0, 1 or 2 as in `pair_stats` (2 = "quantize": what an 8-bit writer would have stored).  SSPE is taken on the frames
    as they are (mode 1: after 2*x-1); the quantiser of mode 2 applies to SSIM, PSNR and LPIPS.  All three modes apply to both
    images.
    `hmr`: the regressor for "sspe" (networks.hmr.HumanModelRecovery); asking for "sspe" without it raises here.
    `lpips`: the model for "lpips" (networks.lpips.LPIPS); asking for "lpips" without it raises here, in the same way."""

    METRICS = ("ssim", "psnr", "sspe", "lpips")
    COLS = 8   # mssim, mse, ref_min, ref_max | scale, shape, pose | lpips

    def __init__(self, metrics=("ssim", "psnr", "sspe"), hmr=None, mode=0, lpips=None):
        metrics = tuple(metrics)
        unknown = [m for m in metrics if m not in self.METRICS]
        if unknown or not metrics:
            raise ValueError("metrics must be among %s, got %s" % (self.METRICS, metrics))
        self.metrics, self.mode = metrics, _mode(mode)
        self._sspe = None
        if "sspe" in metrics:
            if hmr is None:
                raise ValueError('"sspe" needs hmr=<networks.hmr.HumanModelRecovery>: the SMPL vectors come from the regressor')
            self._sspe = ScaleShapePoseError(hmr, unit=self.mode == 1)
        self._lpips = None
        if "lpips" in metrics:
            if lpips is None:
                raise ValueError('"lpips" needs lpips=<networks.lpips.LPIPS>: the distance comes from the AlexNet model')
            self._lpips = PerceptualMetric(lpips).lpips
        self._pixel = "ssim" in metrics or "psnr" in metrics
        self._stats = self._terms = self._dists = None
        self._n = 0

    def _rows(self, name, cols, n, device):
        """a contiguous (n, cols) float64 block at the end of the named device-side table (grown by doubling, stream-ordered)"""
        table = getattr(self, name)
        if table is None or self._n + n > table.shape[0]:
            grown = torch.empty((max(64, 2 * (self._n + n)), cols), device=device, dtype=torch.float64)
            if table is not None:
                grown[:self._n].copy_(table[:self._n])
            setattr(self, name, grown)
            table = grown
        return table[self._n:self._n + n]

    @torch.no_grad()
    def update(self, pred, ref):
        n = int(pred.shape[0])
        if self._pixel:
            pair_stats(pred, ref, self.mode, out=self._rows("_stats", 4, n, pred.device))
        if self._sspe is not None:
            self._sspe.terms(pred, ref, out=self._rows("_terms", 3, n, pred.device))
        if self._lpips is not None:
            self._lpips(pred, ref, self.mode, out=self._rows("_dists", 1, n, pred.device).view(n))
        self._n += n

    def __len__(self):
        return self._n

    def result(self):
        """{"frames": n, "ssim": mean, "psnr": mean, "sspe": mean, "lpips": mean, "per_frame": {name: (n,) float64 array}}; the one
        host copy.
        PSNR's ValueError for a reference image outside [-1,1] is raised here, when the numbers are read."""
        n = self._n
        cols = [t[:n] for t in (self._stats, self._terms, self._dists) if t is not None]
        if n == 0 or not cols:
            return {"frames": 0, "per_frame": {}}
        host = torch.cat(cols, dim=1).cpu().numpy()
        out, per, k = {"frames": n}, {}, 0
        if self._stats is not None:
            if "ssim" in self.metrics:
                per["ssim"] = host[:, 0].copy()
            if "psnr" in self.metrics:
                per["psnr"] = psnr_from_stats(host[:, 0:4])
                per["mse"] = host[:, 1].copy()
            k = 4
        if self._terms is not None:
            per["sspe_scale"], per["sspe_shape"], per["sspe_pose"] = (host[:, k + j].copy() for j in range(3))
            per["sspe"] = host[:, k] + host[:, k + 1] + host[:, k + 2]
            k += 3
        if self._dists is not None:
            per["lpips"] = host[:, k].copy()
        for name in self.metrics:
            out[name] = float(np.mean(per[name]))
        out["per_frame"] = per
        return out


# ------------------------------------------------------------------------------------------------ set metrics: FID and IS
INCEPTION_SIZE = 299


def frechet_distance(mu1, s1, mu2, s2, eps=1e-6):
    """Host, fp64 (metrics.py:309-361, calculate_frechet_distance): |mu1 - mu2|^2 + Tr(s1) + Tr(s2) - 2 Tr(sqrtm(s1 s2)).
    A square root that is not finite is taken again with eps added to both diagonals; a complex one (a singular product gives
    one) must have a diagonal that is real to 1e-3 -- ValueError otherwise -- and its real part is used."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(s1, np.float64)), np.atleast_2d(np.asarray(s2, np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape:
        raise ValueError("the two sets have different feature dimensions: %s / %s and %s / %s" % (mu1.shape, s1.shape, mu2.shape, s2.shape))
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(s1.shape[0]) * eps
        covmean = linalg.sqrtm((s1 + offset).dot(s2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


def fid_from_features(a, b):
    """Host, fp64 (metrics.py:363-379, fid_score_func): a (Na,d), b (Nb,d) feature sets -> their Frechet distance from np.mean
    and np.cov(rowvar=False); 0 when either set is empty."""
    if len(a) == 0 or len(b) == 0:
        return 0
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return frechet_distance(np.mean(a, axis=0), np.cov(a, rowvar=False), np.mean(b, axis=0), np.cov(b, rowvar=False))


def inception_score(features, batch_size=32):
    """Host, fp64 (metrics.py:381-395, 671-698): per batch of `batch_size` rows (the last may be short), the softmax over the
    features AS THEY ARE -- the reference's network ends at the 2048 pool features, not at 1000 logits, and that is reproduced --
    then exp(mean_i sum_j p_ij (log p_ij - log mean_i p_ij)); -> (mean, std) over the batches.  (0, 0) for an empty set."""
    features = np.asarray(features, np.float64)
    if len(features) == 0:
        return 0.0, 0.0
    scores = []
    for s in range(0, len(features), int(batch_size)):
        z = features[s:s + int(batch_size)]
        z = z - z.max(axis=1, keepdims=True)
        e = np.exp(z)
        p = e / e.sum(axis=1, keepdims=True)
        kl = p * (np.log(p) - np.log(np.expand_dims(np.mean(p, 0), 0)))
        scores.append(np.exp(np.mean(np.sum(kl, 1))))
    return float(np.mean(scores)), float(np.std(scores))


def _inception(inception, who):
    if inception is None or not callable(inception) or not hasattr(inception, "max_batch"):
        raise ValueError("%s needs the InceptionV3 model (networks.inception.InceptionV3)" % who)
    return inception


class FIDMetric(BaseMetric):
    """metrics.py:704-781 with the network on the device: `inception` is a networks.inception.InceptionV3.  preds, gts:
    (N,3,H,W) images in [0,1] on the device (mode 1 maps them to [-1,1], then the resize to 299 x 299)."""

    def __init__(self, inception):
        self.inception = _inception(inception, "FIDMetric")

    def features(self, x):
        return self.inception(_as_batch(x), mode=1, resize=INCEPTION_SIZE).cpu().numpy().astype(np.float64)

    def calculate_score(self, preds, gts):
        return fid_from_features(self.features(preds), self.features(gts))

    def quality(self):
        return self.LOWER


class InceptionScoreMetric(BaseMetric):
    """metrics.py:634-701 with the network on the device.  preds: (N,3,H,W) images in [0,1] on the device -> (mean, std)."""

    def __init__(self, inception):
        self.inception = _inception(inception, "InceptionScoreMetric")

    def calculate_score(self, preds, batch_size=32):
        feats = self.inception(_as_batch(preds), mode=1, resize=INCEPTION_SIZE).cpu().numpy()
        return inception_score(feats, batch_size)

    def quality(self):
        return self.HIGHER


class SetEvaluator(object):
    """FID and Inception Score of a sequence, batch by batch, without leaving the device: the unpaired protocols of the reference
    (cross-imitation, appearance transfer, novel views) have no ground-truth frame, only two sets.

        ev = SetEvaluator(inception)                       # frames in [-1,1] as the generator emits them (mode 0)
        for t, preds in imitator.predict_batches(...):
            ev.update(preds, real_frames[t:t + len(preds)])       # or ev.update(preds): Inception Score only
        print(ev.result())

    `update` only launches kernels: the (n,2048) features go to the end of a device-side table (grown by doubling) and no
    `.cpu()`, `.item()` or synchronisation call is made.  `result()` makes ONE device->host copy per table and computes the
    metrics on the host in fp64: {"frames", "is", "is_std"} and, when refs were given, {"fid", "is_ref"}.
    mode: 0, 1 or 2 as in `pair_stats`, applied to preds and refs alike before the resize to 299 x 299."""

    def __init__(self, inception, mode=0):
        self.inception, self.mode = _inception(inception, "SetEvaluator"), _mode(mode)
        self._pred = self._ref = None
        self._n = {"_pred": 0, "_ref": 0}

    def _rows(self, name, n, device):
        table, used = getattr(self, name), self._n[name]
        if table is None or used + n > table.shape[0]:
            grown = torch.empty((max(64, 2 * (used + n)), 2048), device=device, dtype=torch.float32)
            if table is not None:
                grown[:used].copy_(table[:used])
            setattr(self, name, grown)
            table = grown
        self._n[name] = used + n
        return table[used:used + n]

    @torch.no_grad()
    def update(self, pred, ref=None):
        self.inception(pred, mode=self.mode, out=self._rows("_pred", int(pred.shape[0]), pred.device), resize=INCEPTION_SIZE)
        if ref is not None:
            self.inception(ref, mode=self.mode, out=self._rows("_ref", int(ref.shape[0]), ref.device), resize=INCEPTION_SIZE)

    def __len__(self):
        return self._n["_pred"]

    def features(self):
        """-> (pred, ref) float64 host arrays (ref None when no refs were given); one device->host copy per table"""
        host = lambda name: None if getattr(self, name) is None else getattr(self, name)[:self._n[name]].cpu().numpy().astype(np.float64)
        return host("_pred"), host("_ref")

    def result(self, batch_size=32):
        pred, ref = self.features()
        if pred is None or len(pred) == 0:
            return {"frames": 0}
        mean, std = inception_score(pred, batch_size)
        out = {"frames": len(pred), "is": mean, "is_std": std}
        if ref is not None:
            out["fid"] = float(fid_from_features(pred, ref))
            out["is_ref"] = inception_score(ref, batch_size)[0]
        return out
