"""GPU checks of the textured-rendering half of SMPLRenderer (csrc/render.hip) on synthetic.body_mesh() at image_size 64 and 100
(rasters of 128 and 200 with anti-aliasing; 200 leaves partial 32x8 tiles): the shading against the float64 restatement of
tests/render_ref.py evaluated on the CPU oracle rasteriser's maps, silhouettes / face-index maps / texture extraction bit for
bit, and the launch discipline.  tests/test_render_host.py shows that these inputs discriminate."""
import functools

import numpy as np
import pytest
import torch

from impersonator_amd.utils import synthetic
from oracle import raster as oracle_raster
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

# max |render - float64 restatement|.  The float32 evaluation of the reference's own expression stands 2.6e-7 .. 4.6e-7 from its
# float64 evaluation on these inputs, the light adds 1.2e-7, and the blend is continuous in tif (a one-ulp difference cannot
# jump): 5e-6 is about ten times that distance, room for the light multiplied after the blend and for the order of the average.
RENDER_BOUND = 5e-6
SIZES = (64, 100)


@functools.lru_cache(maxsize=None)
def _scene(image_size):
    return rr.scene(image_size)


@functools.lru_cache(maxsize=None)
def _oracle(image_size, raster_size, far):
    """the CPU oracle's (fim, wim, depth) of the scene at raster_size; computed once per shape, never modified"""
    out = oracle_raster.rasterize_fim_wim(_scene(image_size)["f2verts"], raster_size, 0.1, far)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _mesh():
    rest, faces = synthetic.body_mesh()
    return faces, synthetic.uv_seg_map_fn(rest, faces)


def _renderer(image_size, **kw):
    from impersonator_amd.utils.nmr import SMPLRenderer
    faces, map_fn = _mesh()
    return SMPLRenderer(image_size=image_size, faces=faces, map_fn=map_fn, **kw).cuda()


def _inputs(image_size):
    sc = _scene(image_size)
    return sc, torch.from_numpy(sc["cam"]).cuda(), torch.from_numpy(sc["verts"]).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# 6 ------------------------------------------------------------------------------------------------------------- premise
@pytest.mark.parametrize("image_size", SIZES)
def test_premise_rasteriser_equals_the_oracle_at_the_render_planes(image_size):
    """what the shading reads: projected faces, and fim / wim / depth at near 0.1 / far 25 at the super-sampled size"""
    sc, cam, verts = _inputs(image_size)
    S = 2 * image_size
    r = _renderer(S)
    f2v, _, _ = r.render_fim_wim(cam, verts)
    assert np.array_equal(_bits(f2v), sc["f2verts"].view(np.uint32))
    fim, wim, depth = r.rasterize(f2v, near=0.1, far=25.0, return_depth=True)
    ofim, owim, odepth = _oracle(image_size, S, 25.0)
    assert np.array_equal(fim.cpu().numpy(), ofim)
    assert np.array_equal(_bits(wim), owim.view(np.uint32)) and np.array_equal(_bits(depth), odepth.view(np.uint32))
    assert 0.05 < (ofim >= 0).mean() < 0.9


# 7 -------------------------------------------------------------------------------------------------------------- render
@pytest.mark.parametrize("background", ["tuple", "per_sample"])
@pytest.mark.parametrize("light", ["default", "ambient"])
@pytest.mark.parametrize("tex_size", [3, 2])
@pytest.mark.parametrize("anti_aliasing", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("image_size", SIZES)
def test_render_matches_fp64_on_the_oracle_maps(image_size, anti_aliasing, tex_size, light, background):
    sc, cam, verts = _inputs(image_size)
    bs, nf = sc["f2verts"].shape[:2]
    r = _renderer(image_size, anti_aliasing=anti_aliasing, tex_size=tex_size)
    if light == "ambient":
        r.set_ambient_light()
    bg = (0.2, -0.3, 0.5) if background == "tuple" else np.random.default_rng(7).uniform(-1, 1, (bs, 3)).astype(np.float32)
    r.set_bgcolor(bg if background == "tuple" else torch.from_numpy(bg).cuda())
    tex = rr.random_textures(bs, nf, tex_size, seed=tex_size)
    tex_dev = torch.from_numpy(tex).cuda()
    img, fim = r.render(cam, verts, tex_dev)
    assert fim is None and tuple(img.shape) == (bs, 3, image_size, image_size)
    assert torch.equal(tex_dev.cpu(), torch.from_numpy(tex))                      # the light is not applied in place
    S = 2 * image_size if anti_aliasing else image_size
    ofim, owim, odepth = _oracle(image_size, S, 25.0)
    want = rr.render(sc["f2verts"], sc["raw"], ofim, owim, odepth, tex, bg, tex_size, anti_aliasing,
                     light=rr.AMBIENT_LIGHT if light == "ambient" else rr.DEFAULT_LIGHT)
    err = np.abs(img.cpu().numpy().astype(np.float64) - want).max()
    print("render is=%d aa=%d ts=%d %s %s: max abs error %.3e" % (image_size, anti_aliasing, tex_size, light, background, err))
    assert err <= RENDER_BOUND, err


def test_render_known_answer_triangle():
    """the hand-computed pixels of render_ref.triangle_scene: the eps clamp at a vertex, depth / z at the centroid"""
    from impersonator_amd.utils.nmr import SMPLRenderer
    sc = rr.triangle_scene()
    r = SMPLRenderer(image_size=rr.TRIANGLE_SIZE, faces=sc["faces"], map_fn=np.zeros((2, 3), np.float32), anti_aliasing=False,
                     tex_size=2, background_color=(0.25, -0.5, 0.75)).cuda()
    img, fim = r.render(torch.from_numpy(sc["cam"]).cuda(), torch.from_numpy(sc["verts"]).cuda(),
                        torch.from_numpy(sc["textures"]).cuda(), get_fim=True)
    ofim, owim, odepth = oracle_raster.rasterize_fim_wim(sc["f2verts"], rr.TRIANGLE_SIZE, 0.1, 25.0)
    assert np.array_equal(fim.cpu().numpy(), ofim) and int((ofim >= 0).sum()) == 28
    want = rr.render(sc["f2verts"], sc["raw"], ofim, owim, odepth, sc["textures"], (0.25, -0.5, 0.75), 2, False)
    got = img.cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= RENDER_BOUND
    y, x = sc["vertex_pixel"]
    assert np.abs(got[0, :, y, x] - np.array([0.999, 0, 0])).max() <= 1e-6
    y, x = sc["centroid_pixel"]
    assert np.abs(got[0, :, y, x] - np.array([4 / 7, 2 / 7, 1 / 7])).max() <= RENDER_BOUND
    assert np.array_equal(got[0, :, 0, 7], np.float32([0.25, -0.5, 0.75]).astype(np.float64))
    with pytest.raises(ValueError):                               # a one-texel cube: the reference reads texel 1 of it
        r.render(torch.from_numpy(sc["cam"]).cuda(), torch.from_numpy(sc["verts"]).cuda(), torch.ones(1, 1, 1, 1, 1, 3).cuda())


# 8, 9 ------------------------------------------------------------------------------------- silhouettes, face-index map
@pytest.mark.parametrize("anti_aliasing", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("image_size", SIZES)
def test_silhouettes_are_the_pooled_coverage_of_the_oracle(image_size, anti_aliasing):
    sc, cam, verts = _inputs(image_size)
    r = _renderer(image_size, anti_aliasing=anti_aliasing)
    alpha = r.render_silhouettes(cam, verts)
    ofim, _, _ = _oracle(image_size, 2 * image_size if anti_aliasing else image_size, 100.0)
    want = rr.silhouette(ofim, anti_aliasing)
    assert tuple(alpha.shape) == want.shape and np.array_equal(_bits(alpha), want.view(np.uint32))
    levels = set(np.unique(alpha.cpu().numpy()).tolist())
    assert levels <= {0.0, 0.25, 0.5, 0.75, 1.0} and {0.0, 1.0} <= levels
    if anti_aliasing:
        assert levels & {0.25, 0.5, 0.75}


@pytest.mark.parametrize("image_size", SIZES)
def test_get_fim_is_the_oracles_map_at_1x(image_size):
    sc, cam, verts = _inputs(image_size)
    r = _renderer(image_size)
    _, fim = r.render(cam, verts, r.debug_textures().cuda(), get_fim=True)
    assert fim.dtype == torch.int32 and np.array_equal(fim.cpu().numpy(), _oracle(image_size, image_size, 25.0)[0])


# 10, 11 ---------------------------------------------------------------------------------- sampling grid, extraction
def _sampler_inputs():
    sc, _, verts = _inputs(64)
    cam = sc["cam"].copy()
    cam[1, 0] = 1.3                   # part of this mesh leaves [-1,1]: those points clamp
    return sc, cam, verts


@pytest.mark.parametrize("tex_size", [3, 2])
def test_dynamic_sampler_matches_fp64_and_clamps_exactly(tex_size):
    sc, cam, verts = _sampler_inputs()
    r = _renderer(64, tex_size=tex_size)
    got = r.dynamic_sampler(torch.from_numpy(cam).cuda(), verts, None).cpu().numpy()
    coords = r.coords.cpu().numpy()
    want = rr.face_sampler(cam, sc["verts"], sc["faces"], coords)
    assert got.shape == want.shape == (3, 13776, tex_size * tex_size, 2)
    err = np.abs(got.astype(np.float64) - want).max()
    print("dynamic_sampler ts=%d: max abs error %.3e" % (tex_size, err))
    assert err <= 1e-6, err
    raw = rr.face_sampler(cam, sc["verts"], sc["faces"], coords, clamp=False)
    out = np.abs(raw) > 1 + 1e-5
    assert out.sum() > 100 and np.array_equal(got[out], np.sign(raw[out]).astype(np.float32))
    assert np.abs(got).max() == 1.0


@pytest.mark.parametrize("shared_image", [False, True], ids=["per_sample", "shared"])
@pytest.mark.parametrize("align_corners", [False, True], ids=["align0", "align1"])
def test_extract_tex_is_grid_sample_rearranged(align_corners, shared_image):
    sc, cam, verts = _sampler_inputs()
    r = _renderer(64, align_corners=align_corners)
    sampler = r.dynamic_sampler(torch.from_numpy(cam).cuda(), verts, None)
    img = torch.from_numpy(synthetic.image(11, (1 if shared_image else 3, 3, 48, 80))).cuda()
    tex = r.extract_tex(img, sampler)
    assert tuple(tex.shape) == (3, 13776, 3, 3, 3, 3)
    flat = r.grid_sample(img, sampler)                                        # (bs,3,nf,T*T)
    want = flat.view(3, 3, 13776, 3, 3).permute(0, 2, 3, 4, 1)[:, :, :, :, None, :].expand(-1, -1, -1, -1, 3, -1)
    assert np.array_equal(_bits(tex), _bits(want))
    assert bool((tex[:, :, :, :, 0:1] == tex).all())                          # constant along k
    ref = rr.extract_tex(img.cpu().numpy(), sampler.cpu().numpy(), 3, align_corners)
    # ... and it is the bilinear sample at all.  Float32 places the sample point within ~1.8e-5 px in x (g + 1 rounds at
    # ulp(2)/2 = 1.2e-7, times W = 80, plus the product's and the halving's own roundings below ulp(128) = 7.6e-6) and
    # ~1.1e-5 px in y (H = 48); neighbouring texels of the U(-1,1) image differ by at most 2, so the value moves by at most
    # 2 * 1.8e-5 + 2 * 1.1e-5 = 5.8e-5; the four products and three sums add ~5e-7.
    assert np.abs(tex.cpu().numpy() - ref).max() <= 6e-5


# 12 --------------------------------------------------------------------------------------------------------- identities
def test_forward_is_extract_then_render_and_shared_textures_repeat():
    sc, cam, verts = _inputs(64)
    bs = cam.shape[0]
    r = _renderer(64)
    r.set_ambient_light()
    frames = torch.from_numpy(synthetic.smooth_image(3, (bs, 3, 64, 64))).cuda()
    images, textures, fim = r.forward(cam, verts, frames, dynamic=True, get_fim=True)
    tex2 = r.extract_tex_from_image(frames, cam, verts)
    images2, fim2 = r.render(cam, verts, tex2, get_fim=True)
    assert np.array_equal(_bits(textures), _bits(tex2)) and np.array_equal(_bits(images), _bits(images2))
    assert torch.equal(fim, fim2) and float(images.abs().max()) > 0.1
    assert len(r.forward(cam, verts, frames)) == 2

    one = torch.from_numpy(rr.random_textures(1, 13776, 3, seed=1)).cuda()
    a, _ = r.render(cam, verts, one)
    b, _ = r.render(cam, verts, one.expand(bs, -1, -1, -1, -1, -1).contiguous())
    c, _ = r.render(cam, verts, one[0])
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))

    with pytest.raises(RuntimeError, match="uv_sampler"):
        r.forward(cam, verts, frames, dynamic=False)
    static = _renderer(64, uv_sampler=r.dynamic_sampler(cam[0:1], verts[0:1], None)[0].cpu().numpy())
    static.set_ambient_light()
    images3, textures3 = static.forward(cam[0:1], verts[0:1], frames[0:1], dynamic=False)
    assert np.array_equal(_bits(images3), _bits(images[0:1])) and np.array_equal(_bits(textures3), _bits(textures[0:1]))


# 13 -------------------------------------------------------------------------------------------------- launch discipline
def test_render_paths_launch_no_framework_kernel_and_repeat_bit_for_bit():
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    sc, cam, verts = _inputs(64)
    r = _renderer(64)
    r.set_ambient_light()
    tex = torch.from_numpy(rr.random_textures(1, 13776, 3, seed=2)).cuda()
    frames = torch.from_numpy(synthetic.smooth_image(3, (cam.shape[0], 3, 64, 64))).cuda()
    calls = dict(render=lambda: r.render(cam, verts, tex, get_fim=True), render_silhouettes=lambda: (r.render_silhouettes(cam, verts),),
                 extract_tex_from_image=lambda: (r.extract_tex_from_image(frames, cam, verts),))
    expect = dict(render=["project_faces_kernel", "raster_setup_kernel", "raster_tile_kernel", "face_light_kernel",
                          "shade_resolve_kernel", "raster_setup_kernel", "raster_tile_kernel"],
                  render_silhouettes=["project_faces_kernel", "raster_setup_kernel", "raster_tile_kernel", "silhouette_resolve_kernel"],
                  extract_tex_from_image=["face_sampler_kernel", "extract_tex_kernel"])
    for name, fn in calls.items():
        first = [t.clone() for t in fn()]
        torch.cuda.synchronize()
        kept = {k: v.data_ptr() for k, v in r._bufs.items()}
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            again = fn()
            torch.cuda.synchronize()
        for a, b in zip(first, again):
            assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)), name
        assert kept == {k: v.data_ptr() for k, v in r._bufs.items()}, name      # the cached maps are reused, not reallocated
        records = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
        foreign = sorted({k for k in records if "lwg" not in k})
        print("%s: device records %s, others: %s" % (name, records, foreign))
        assert not foreign, (name, foreign)
        assert len(records) == len(expect[name]), (name, records)
        for kernel in set(expect[name]):
            assert sum(kernel in rec for rec in records) == expect[name].count(kernel), (name, kernel, records)
