"""CPU checks of the textured-rendering half of SMPLRenderer: the float64 restatements of tests/render_ref.py against the live
reference where it is pure torch / numpy, a hand-computed known answer for the texture sampling, the discriminating power of
the GPU tests' inputs (every mutant of the restatement must move the result far beyond the GPU tests' bound), and the refusals
of the new entry points and of `create_coords`."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from impersonator_amd import _lib
from impersonator_amd.utils import mesh
from impersonator_amd.utils.nmr import SMPLRenderer
from oracle import raster as oracle_raster
from oracle import reference_loader
from tests import render_ref as rr

RENDER_BOUND = 5e-6          # the bound of tests/test_gpu_render.py::test_render_matches_fp64_on_the_oracle_maps
needs_reference = pytest.mark.skipif(not reference_loader.available(), reason="reference tree not present")


def _reference_lighting():
    path = os.path.join(reference_loader.REFERENCE_ROOT, "thirdparty", "neural_renderer", "neural_renderer", "lighting.py")
    spec = importlib.util.spec_from_file_location("_ref_nr_lighting", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.lighting


# 1 ---------------------------------------------------------------------------------------------------------------- lighting
@needs_reference
@pytest.mark.parametrize("light", [rr.DEFAULT_LIGHT, rr.AMBIENT_LIGHT, dict(rr.AMBIENT_LIGHT, int_amb=0, color_dir=(0.2, 1, 0.5))],
                         ids=["default", "ambient", "directional_only"])
def test_light_restatement_equals_the_reference(light):
    lighting = _reference_lighting()
    rng = np.random.default_rng(0)
    faces = rng.uniform(-1, 1, (2, 50, 3, 3)).astype(np.float32)
    faces[0, 0, 1] = faces[0, 0, 0]                      # exactly degenerate: zero normal, divided by the 1e-5 floor
    faces[1, 3] = 0.0
    want = lighting(torch.from_numpy(faces), torch.ones(2, 50, 1, 1, 1, 3), light["int_amb"], light["int_dir"],
                    list(light["color_amb"]), list(light["color_dir"]), list(light["direction"]))[:, :, 0, 0, 0].numpy()
    got = rr.face_light(faces, **light)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
    if light["int_dir"] != 0:
        assert np.array_equal(got[0, 0], np.full(3, np.float64(np.float32(light["int_amb"]))))   # degenerate: ambient only
    else:
        assert np.array_equal(got, np.ones_like(got))      # the class defaults: light is exactly 1


# 2 ------------------------------------------------------------------------------------------------- sampling grids
def _write_uv_obj(path, nf=12, seed=0):
    rng = np.random.default_rng(seed)
    nvt = 10
    with open(path, "w") as fh:
        for _ in range(nvt):
            fh.write("v %f %f %f\n" % tuple(rng.uniform(-1, 1, 3)))
        for _ in range(nvt):
            fh.write("vt %f %f\n" % tuple(rng.uniform(-0.1, 1.1, 2)))       # some outside the unit square: clipped
        fh.write("vn 0 0 1\n")
        for _ in range(nf):
            a = rng.integers(1, nvt + 1, 3)
            b = rng.integers(1, nvt + 1, 3)
            fh.write("f %d/%d/1 %d/%d/1 %d/%d/1\n" % (a[0], b[0], a[1], b[1], a[2], b[2]))


@needs_reference
@pytest.mark.parametrize("tex_size", [2, 3, 4])
def test_uvsampler_coords_and_sampler_equal_the_reference(tmp_path, monkeypatch, tex_size):
    ref = reference_loader.load()
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)     # create_coords of the reference calls .cuda()
    obj = str(tmp_path / "uv.obj")
    _write_uv_obj(obj)
    want = ref.nmr.mesh.create_uvsampler(obj, tex_size=tex_size)
    got = mesh.create_uvsampler(obj, tex_size=tex_size)
    assert got.shape == want.shape == (12, tex_size * tex_size, 2)
    assert np.array_equal(got, want)
    assert got.min() == -1.0 and got.max() == 1.0                            # the clip is exercised

    coords = SMPLRenderer.create_coords(tex_size)
    assert torch.equal(coords, ref.nmr.SMPLRenderer.create_coords(tex_size))
    pts = torch.from_numpy(np.random.default_rng(1).uniform(-1.2, 1.2, (2, 7, 3, 2)).astype(np.float32))
    want_s = ref.nmr.SMPLRenderer.points_to_sampler(coords, pts)
    assert torch.equal(SMPLRenderer.points_to_sampler(coords, pts), want_s)
    assert bool((want_s.abs() == 1).any())
    # the restatement's own projection + gather + combination, through a camera and a face list
    cam = np.array([[0.9, 0.05, -0.1], [1.3, 0.0, 0.1]], np.float32)
    verts = np.random.default_rng(2).uniform(-1, 1, (2, 9, 3)).astype(np.float32)
    faces = np.random.default_rng(3).integers(0, 9, (7, 3)).astype(np.int32)
    proj = ref.nmr.SMPLRenderer.batch_orth_proj_idrot(torch.from_numpy(cam), torch.from_numpy(verts))
    assert torch.equal(SMPLRenderer.batch_orth_proj_idrot(torch.from_numpy(cam), torch.from_numpy(verts)), proj)
    want_d = ref.nmr.SMPLRenderer.points_to_sampler(coords, proj[:, torch.from_numpy(faces).long()]).numpy()
    assert np.abs(rr.face_sampler(cam, verts, faces, coords.numpy()) - want_d).max() <= 1e-6


# 3 --------------------------------------------------------------------------------------------------- known answer
@functools.lru_cache(maxsize=None)
def _triangle_maps():
    sc = rr.triangle_scene()
    return sc, oracle_raster.rasterize_fim_wim(sc["f2verts"], rr.TRIANGLE_SIZE, 0.1, 25.0)


def _triangle_render(mutant=None):
    sc, (fim, wim, depth) = _triangle_maps()
    return sc, rr.render(sc["f2verts"], sc["raw"], fim, wim, depth, sc["textures"], (0.25, -0.5, 0.75), 2, False, mutant=mutant)


def test_sampling_known_answer_on_one_triangle():
    sc, img = _triangle_render()
    _, (fim, _, _) = _triangle_maps()
    assert int((fim >= 0).sum()) == 28 and fim[0][sc["vertex_pixel"]] == 0 and fim[0][sc["centroid_pixel"]] == 0
    y, x = sc["vertex_pixel"]
    hi = float(np.float32(1) - np.float32(1e-3))
    assert np.abs(img[0, :, y, x] - np.array([hi, 0, 0])).max() <= 1e-12           # w = (1,0,0) exactly
    y, x = sc["centroid_pixel"]
    assert np.abs(img[0, :, y, x] - np.array([4 / 7, 2 / 7, 1 / 7])).max() <= 2e-6   # depths are 1, 2, 4 up to float32 rounding
    assert np.array_equal(img[0, :, 0, 7], np.float32([0.25, -0.5, 0.75]).astype(np.float64))   # uncovered: the background
    # what each mistake would give at these two pixels
    _, m = _triangle_render("no_eps")
    assert np.array_equal(m[0, :, sc["vertex_pixel"][0], sc["vertex_pixel"][1]], [1.0, 0.0, 0.0])
    _, m = _triangle_render("transpose_axes")
    assert np.abs(m[0, :, y, x] - np.array([1 / 7, 2 / 7, 4 / 7])).max() <= 2e-6
    _, m = _triangle_render("no_depth_ratio")
    assert np.abs(m[0, :, y, x] - 1 / 3).max() <= 2e-6
    _, m = _triangle_render("no_flip")
    assert np.array_equal(m[0, :, 7 - sc["vertex_pixel"][0], sc["vertex_pixel"][1]], [hi, 0.0, 0.0])


# 4 ------------------------------------------------------------------------------------------- the inputs discriminate
@functools.lru_cache(maxsize=None)
def _body_maps():
    sc = rr.scene(64)
    return sc, oracle_raster.rasterize_fim_wim(sc["f2verts"], 128, 0.1, 25.0)


@pytest.mark.parametrize("mutant", rr.RENDER_MUTANTS)
def test_every_render_mutant_moves_the_gpu_tests_inputs(mutant):
    """On the body-mesh inputs of the GPU tests (image_size 64, anti-aliased: the oracle rasteriser at S = 128; fully random
    textures; set_ambient_light) each mutant moves the picture by more than 100x the GPU tests' bound.  The eps clamp is the
    exception: it acts only where w * depth / z exceeds 1 - eps / (ts - 1), no pixel of the body mesh comes closer than 0.9913
    (asserted below), so that mutant is held to the same factor on the known-answer triangle, which the GPU tests render too."""
    sc, (fim, wim, depth) = _body_maps()
    bs, nf = sc["f2verts"].shape[:2]
    moved = 0.0
    for ts in (3, 2):
        tex = rr.random_textures(bs, nf, ts, seed=ts)
        args = (sc["f2verts"], sc["raw"], fim, wim, depth, tex, (0.2, -0.3, 0.5), ts, True)
        base = rr.render(*args, light=rr.AMBIENT_LIGHT)
        d = np.abs(rr.render(*args, light=rr.AMBIENT_LIGHT, mutant=mutant) - base).max()
        print("tex_size %d %s: moves the picture by %.3e" % (ts, mutant, d))
        moved = d if ts == 3 else min(moved, d)
    if mutant != "no_eps":
        assert moved > 100 * RENDER_BOUND, moved
        return
    cov = fim >= 0
    b = np.nonzero(cov)[0]
    top = (wim[cov].astype(np.float64) * depth[cov].astype(np.float64)[:, None] / sc["f2verts"][b, fim[cov], :, 2]).max()
    assert moved == 0.0 and top < 0.995, (moved, top)
    sc, base = _triangle_render()
    _, out = _triangle_render("no_eps")
    assert np.abs(out - base).max() > 100 * RENDER_BOUND


def test_sampler_mutant_moves_the_gpu_tests_inputs():
    sc = rr.scene(64)
    coords = SMPLRenderer.create_coords(3).numpy()
    base = rr.face_sampler(sc["cam"], sc["verts"], sc["faces"], coords)
    d = np.abs(rr.face_sampler(sc["cam"], sc["verts"], sc["faces"], coords, mutant="sampler_yflip") - base).max()
    assert d > 100 * 1e-6, d


# 5 ------------------------------------------------------------------------------------------------------ refusals
def test_create_coords_sizes():
    for t in (2, 3, 4, 5, 6, 8):
        c = SMPLRenderer.create_coords(t)
        assert tuple(c.shape) == (2, t * t) and float(c.min()) == 0.0 and abs(float(c.max()) - 1.0) < 1e-6
    for t in (1, 7):
        with pytest.raises(ValueError):
            SMPLRenderer.create_coords(t)
    assert torch.equal(SMPLRenderer.create_coords(2), torch.tensor([[0., 0., 1., 1.], [0., 1., 0., 1.]]))
    with pytest.raises(ValueError):
        mesh.create_uvsampler("unused", tex_size=1)


def test_renderer_surface_without_a_device():
    from impersonator_amd.utils import synthetic
    rest, faces = synthetic.body_mesh()
    r = SMPLRenderer(image_size=16, faces=faces, map_fn=synthetic.uv_seg_map_fn(rest, faces))
    assert (r.light_intensity_ambient, r.light_intensity_directional, r.light_direction) == (1, 0, [0, 1, 0])
    assert r.rasterizer_eps == 1e-3 and r.img2uv_sampler is None and tuple(r.coords.shape) == (2, 9)
    r.set_ambient_light()
    assert (r.light_intensity_ambient, r.light_intensity_directional, r.light_direction) == (0.7, 0.3, (1, 0.5, 1))
    r.set_bgcolor()
    assert r.background_color == (-1, -1, -1)
    assert tuple(r.debug_textures().shape) == (13776, 3, 3, 3, 3)
    r.set_tex_size(2)
    assert r.tex_size == 2 and tuple(r.coords.shape) == (2, 4) and tuple(r.debug_textures().shape) == (13776, 2, 2, 2, 3)
    with pytest.raises(ValueError):
        r.set_tex_size(7)
    for name in ("render_depth", "infer_face_index_map"):
        with pytest.raises(NotImplementedError):
            getattr(r, name)(None, None)
    with pytest.raises(RuntimeError, match="GPU only"):       # no CPU fallback
        r.render(torch.zeros(1, 3), torch.zeros(1, 6890, 3), r.debug_textures())
    with pytest.raises(ValueError):                            # tex_size 7: the renderer is built, its coords are not
        SMPLRenderer(image_size=16, faces=faces, map_fn=synthetic.uv_seg_map_fn(rest, faces), tex_size=7).dynamic_sampler(
            torch.zeros(1, 3), torch.zeros(1, 6890, 3))
    grid = SMPLRenderer.create_meshgrid(5)
    assert tuple(grid.shape) == (5, 5, 2) and grid[0, 4].tolist() == [1.0, -1.0]
    pts = torch.arange(24, dtype=torch.float32).view(2, 6, 2)
    assert torch.equal(r.points_to_faces(pts, torch.tensor([[[0, 5, 2]], [[1, 1, 3]]]))[1, 0], pts[1][[1, 1, 3]])
    assert torch.equal(SMPLRenderer.compute_barycenter(torch.tensor([[[[0., 0.], [2., 0.], [0., 4.]]]])), torch.tensor([[[1., 0.]]]))
    dst_fim = torch.full((1, 16, 16), -1)
    dst_fim[0, 2, 3] = 1
    T = r.cal_transform(torch.tensor([[[0.5, -0.5], [0.25, 0.75]]]), torch.zeros(1, 16, 16), dst_fim)
    assert T[0, 2, 3].tolist() == [0.25, 0.75] and float(T.sum()) == -2.0 * (16 * 16 * 2 - 2) + 1.0
    assert tuple(r.project_to_image(torch.tensor([[2., 0.5, 0.]]), torch.ones(1, 4, 3)).shape) == (1, 4, 2)


def test_new_entry_points_refuse_null_and_bad_sizes_without_a_device():
    lib = _lib.load()
    p, tri = ctypes.c_void_p(4096), (ctypes.c_float * 3)(1, 1, 1)
    light = lambda verts=p, faces=p, bs=1, nv=3, nf=1, ca=tri, out=p: lib.lwg_face_light(verts, faces, bs, nv, nf, 1.0, 0.0, ca, tri,
                                                                                       tri, out, None)
    shade = lambda f2v=p, fim=p, wim=p, depth=p, tex=p, tb=1, lit=p, bg=p, bb=1, bs=2, nf=1, s=8, ts=2, out=p: lib.lwg_shade_resolve(
        f2v, fim, wim, depth, tex, tb, lit, bg, bb, bs, nf, s, 1, ts, 1e-3, out, None)
    sil = lambda fim=p, bs=1, s=8, out=p: lib.lwg_silhouette_resolve(fim, bs, s, 1, out, None)
    samp = lambda cam=p, verts=p, faces=p, coords=p, bs=1, nv=3, nf=1, tt=9, out=p: lib.lwg_face_sampler(cam, verts, faces, coords, bs,
                                                                                                      nv, nf, tt, out, None)
    ext = lambda img=p, ib=1, h=4, w=4, grid=p, bs=2, nf=1, ts=3, out=p: lib.lwg_extract_tex(img, ib, h, w, grid, bs, nf, ts, 0, out,
                                                                                         None)
    nulls = [(light, ("verts", "faces", "ca", "out")), (shade, ("f2v", "fim", "wim", "depth", "tex", "lit", "bg", "out")),
             (sil, ("fim", "out")), (samp, ("cam", "verts", "faces", "coords", "out")), (ext, ("img", "grid", "out"))]
    for fn, names in nulls:
        for name in names:
            assert fn(**{name: None}) == -1 and b"NULL" in lib.lwg_last_error(), name
    for fn, kws in ((light, (dict(bs=0), dict(nv=0), dict(nf=-1))), (shade, (dict(bs=0), dict(nf=0), dict(s=0))),
                    (sil, (dict(bs=0), dict(s=-4))), (samp, (dict(bs=0), dict(nv=0), dict(nf=0), dict(tt=0))),
                    (ext, (dict(h=0), dict(w=0), dict(bs=0), dict(nf=0), dict(ts=0)))):
        for kw in kws:
            assert fn(**kw) == -1 and b"positive" in lib.lwg_last_error(), kw
    assert shade(ts=1) == -1 and b"tex_size" in lib.lwg_last_error()
    assert shade(tb=3) == -1 and shade(bb=3) == -1 and ext(ib=3) == -1
    assert shade(s=5000) == -2 and sil(s=5000) == -2                 # 10000^2 sub-pixels: beyond the rasteriser's own limit
