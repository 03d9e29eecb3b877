"""GPU: novel views in batches.  lwg_rigid_views against Viewer.rotate_trans (bit for bit) and float64 NumPy; lwg_image_grid_u8
against torchvision's make_grid + save_image written out as torch CPU operations (exact bytes, every rounding boundary of the
uint8 conversion and both clamps in the data); Viewer.views and Viewer.view_graph against Viewer.view (bit for bit), and
Viewer.views against the reference's own outputs (tests/golden/tasks_golden.npz)."""
import math

import numpy as np
import pytest
import torch

from impersonator_amd import demo
from impersonator_amd.utils import cv_utils, util
from tests import helpers

pytestmark = pytest.mark.gpu

SIZE, BATCH = 128, 2
# five views = blocks of 2 + 2 + 1: distinct rotations, a translation that is not zero and differs per view
RTS = [(0.0, 0.6, 0.0), (0.2, -1.1, 0.1), (0.17, 2.4, 0.17), (-0.3, 3.9, 0.05), (0.1, 5.5, -0.2)]
TS = [(0.02, 0.0, 0.0), (0.0, -0.03, 0.01), (0.05, 0.02, 0.0), (-0.04, 0.0, 0.02), (0.01, 0.01, -0.01)]

_cache = {}


def _viewer():
    """One personalised synthetic Viewer for the module (128 x 128, batch_size 2); tests set `bg_replace` / `front_warp` themselves."""
    if "vw" not in _cache:
        vw, smpl, img, bg = demo.build_synthetic_imitator(batch_size=BATCH, seed=0, image_size=SIZE, affine="random", model="viewer")
        vw.personalize(img, src_smpl=smpl, bg_img=bg)
        _cache["vw"] = vw
    vw = _cache["vw"]
    vw._opt.bg_replace, vw._opt.front_warp = False, False
    return vw


# ---------------------------------------------------------------------------------------------------------------- rigid kernel
@pytest.mark.parametrize("nv", [257, 1])
def test_rigid_views_equals_rotate_trans_and_float64(nv):
    vw = _viewer()
    g = torch.Generator().manual_seed(nv)
    X = (torch.rand(1, nv, 3, generator=g) * 2 - 1).cuda()
    rts, ts = RTS[:3], TS[:3]
    out = vw.rotate_trans_batch(rts, ts, X)
    assert out.shape == (3, nv, 3) and out.dtype == torch.float32
    x64 = X[0].cpu().numpy().astype(np.float64)
    for k in range(3):
        one = vw.rotate_trans(rts[k], ts[k], X)
        assert torch.equal(out[k], one[0]), k
        R = np.asarray(cv_utils.euler2matrix(rts[k]), dtype=np.float32).astype(np.float64)
        ref = x64 @ R + np.asarray(ts[k], dtype=np.float32).astype(np.float64)
        err = float(np.abs(out[k].cpu().numpy().astype(np.float64) - ref).max())
        print("nv=%d view %d: max |out - float64| = %.3g" % (nv, k, err))
        assert err <= 1e-6, (k, err)
    # one translation for every view
    shared = vw.rotate_trans_batch(rts, ts[0], X)
    assert torch.equal(shared[2], vw.rotate_trans(rts[2], ts[0], X)[0])
    with pytest.raises(RuntimeError):
        vw.rotate_trans_batch(rts, ts, X.cpu())


# ----------------------------------------------------------------------------------------------------------------- grid kernel
def oracle_grid(x, nrow=8, padding=2, pad_value=0.0, normalize=False):
    """torchvision.utils.make_grid + save_image's conversion on the CPU: (n,3,H,W) float -> (grid_h, grid_w, 3) uint8."""
    x = x.detach().cpu().float().clone()
    if normalize:
        x = (x + 1) / 2.0
    n, _, H, W = x.shape
    if n == 1:
        grid = x[0]
    else:
        xmaps = min(nrow, n)
        ymaps = int(math.ceil(float(n) / xmaps))
        h, w = H + padding, W + padding
        grid = x.new_full((3, h * ymaps + padding, w * xmaps + padding), pad_value)
        for k in range(n):
            r, c = k // xmaps, k % xmaps
            grid[:, r * h + padding:r * h + padding + H, c * w + padding:c * w + padding + W] = x[k]
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def _neighbours(v):
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-4)), np.nextafter(v, np.float32(4))])


def _value_pool():
    """A sweep of [-1.25, 1.25] (both clamps) and, for every grey level k, the float32 neighbours of the inputs at which the
    conversion steps -- 2k/255 - 1 and 2(k + 0.5)/255 - 1 for the normalised path, k/255 and (k + 0.5)/255 for the plain one."""
    if "pool" not in _cache:
        k = np.arange(256, dtype=np.float64)
        pool = np.concatenate([np.linspace(-1.25, 1.25, 64).astype(np.float32),
                               _neighbours(2 * k / 255 - 1), _neighbours(2 * (k + 0.5) / 255 - 1),
                               _neighbours(k / 255), _neighbours((k + 0.5) / 255)]).astype(np.float32)
        assert np.isfinite(pool).all()
        _cache["pool"] = pool
    return _cache["pool"]


GRID_CASES = [(1, 4, 6, 8, 2), (3, 5, 7, 8, 2), (5, 6, 10, 4, 2), (16, 8, 8, 8, 2), (4, 3, 3, 2, 0), (7, 9, 5, 3, 1)]


@pytest.mark.parametrize("pad_value", [0.0, 0.5])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("case", GRID_CASES)
def test_image_grid_u8_exact_bytes(case, normalize, pad_value):
    n, H, W, nrow, padding = case
    pool = _value_pool()
    count = n * 3 * H * W
    # cyclic fill; every case starts elsewhere in the pool so that the small ones see the boundary values too
    start = (GRID_CASES.index(case) * 389) % len(pool)
    x = torch.from_numpy(pool[(start + np.arange(count)) % len(pool)].reshape(n, 3, H, W).copy())
    ref = oracle_grid(x, nrow, padding, pad_value, normalize)
    out = util.image_grid_u8(x.cuda(), nrow=nrow, padding=padding, pad_value=pad_value, normalize=normalize)
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == tuple(ref.shape)
    assert tuple(out.shape[:2]) == util.image_grid_shape(n, H, W, nrow, padding)
    got = out.cpu()
    bad = int((got != ref).sum())
    assert bad == 0, "%d of %d bytes differ, first at %s" % (bad, ref.numel(), (got != ref).nonzero()[0].tolist())
    if n == 16:
        assert ref.min() == 0 and ref.max() == 255 and len(torch.unique(ref)) == 256      # every level and both clamps occur


def test_save_image_grid_writes_the_bytes(tmp_path):
    from PIL import Image
    x = torch.from_numpy(_value_pool()[:5 * 3 * 6 * 10].reshape(5, 3, 6, 10).copy())
    path = str(tmp_path / "grid.png")
    util.save_image_grid(x.cuda(), path, nrow=4, normalize=True)
    assert np.array_equal(np.asarray(Image.open(path)), oracle_grid(x, 4, 2, 0.0, True).numpy())
    with pytest.raises(RuntimeError):
        util.image_grid_u8(x)          # no CPU path


# ------------------------------------------------------------------------------------------------------------ views equals view
@pytest.mark.parametrize("bg_replace,front_warp", [(False, False), (True, False), (False, True)])
def test_views_equals_view(bg_replace, front_warp):
    vw = _viewer()
    vw._opt.bg_replace, vw._opt.front_warp = bg_replace, front_warp
    singles = [vw.view(rt, t).clone() for rt, t in zip(RTS, TS)]
    fim_last, T_last = vw.tsf_info['fim'].clone(), vw.T.clone()
    preds = vw.views(RTS, TS)
    assert preds.shape == (5, 3, SIZE, SIZE)
    for i, one in enumerate(singles):
        assert torch.equal(preds[i], one[0]), "view %d differs by %g" % (i, float((preds[i] - one[0]).abs().max()))
    assert float((singles[0] - singles[3]).abs().max()) > 1e-2          # the views are different pictures
    # the last block is view 4 alone
    assert vw.tsf_info['fim'].shape == (1, SIZE, SIZE) and torch.equal(vw.tsf_info['fim'], fim_last)
    assert torch.equal(vw.T, T_last) and torch.equal(vw.tsf_info['T'], T_last)
    # a (3,) translation serves every view
    shared = vw.views(RTS[:3], TS[1])
    assert torch.equal(shared[2], vw.view(RTS[2], TS[1])[0])


def test_views_matches_the_reference_golden():
    """Same set-up as tests/test_gpu_tasks.py::test_viewer_matches_the_reference_golden, through the batched methods: the rotated
    meshes on their own (1e-6), then `views` from the golden meshes so that the face-index maps are those of the same vertices."""
    g, sc = helpers.golden("tasks_golden.npz"), helpers.task_scene()
    vw, _, _, _ = demo.build_synthetic_imitator(batch_size=2, seed=0, affine="random", model="viewer")
    t = lambda a: torch.from_numpy(a).cuda()
    vw.hmr = helpers.FixedHMR([(t(sc["cam_a"]), t(sc["verts_a"]))])
    vw.personalize(sc["img_a"][0], src_smpl=np.zeros(85, np.float32))
    rts, ts = [v[0] for v in sc["views"]], [v[1] for v in sc["views"]]
    golden_meshes = torch.cat([t(g["view%d_mesh" % i]).reshape(1, -1, 3) for i in range(len(rts))])
    meshes = vw.rotate_trans_batch(rts, ts, vw.src_info["verts"])
    for i in range(len(rts)):
        assert float((meshes[i] - golden_meshes[i]).abs().max()) <= 1e-6, i
    vw.rotate_trans_batch = lambda rts, ts, X: golden_meshes
    for replace in (False, True):
        vw._opt.bg_replace = replace
        preds = vw.views(rts, ts).cpu().numpy()
        for i, view in enumerate(sc["views"]):
            if view[2] == replace:
                err = float(np.abs(preds[i] - g["view%d_preds" % i].reshape(preds[i].shape)).max())
                print("view %d (bg_replace=%s): max |views - reference| = %.3g" % (i, replace, err))
                assert err <= 1e-3, (i, err)
    vw.generator.release()


# ------------------------------------------------------------------------------------------------------------------ view_graph
def test_view_graph_replays_to_the_bits_of_view():
    vw = _viewer()
    order = [0, 1, 2, 0]          # three different views, then the first again
    eager = []
    for k in order[:3]:
        p = vw.view(RTS[k], TS[k]).clone()
        eager.append((p, vw.tsf_info['fim'].clone()))
    run = vw.view_graph(batch=1)
    for k in order:
        # eager work between the replays: whatever the graph reads must be its own, not memory the allocator hands out again
        vw.view(RTS[4], TS[4])
        junk = [torch.full((1, 3, SIZE, SIZE), 7.0, device="cuda") for _ in range(8)]
        del junk
        out = run(RTS[k], TS[k])
        torch.cuda.synchronize()
        assert out.shape == (1, 3, SIZE, SIZE)
        assert torch.equal(out, eager[k][0]), k
        assert torch.equal(vw.tsf_info['fim'], eager[k][1]), k
    # a graph of two views per replay
    run2 = vw.view_graph(batch=2)
    out = run2(RTS[1:3], TS[1:3])
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[1][0][0]) and torch.equal(out[1], eager[2][0][0])
    with pytest.raises(ValueError):
        run2(RTS[:3], TS[:3])
