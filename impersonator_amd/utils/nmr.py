"""SMPLRenderer on MI355X: the reference's geometry glue (utils/nmr.py:103-662) over liblwg.

Keeps the method names, argument order and return types of the methods on the Imitator.forward()
path -- `render_fim_wim`, `encode_fim`, `encode_front_fim`, `cal_bc_transform`, `get_vis_f2pts` --
and adds `transfer()`, the fused per-frame sequence of models/imitator.py:250-260.

The textured-rendering half (utils/nmr.py:179-244,295-310,354-504,587-615,661-662) -- `render`, `forward`,
`render_silhouettes`, `extract_tex`, `extract_tex_from_image`, `dynamic_sampler`, the light / background / texture-size
setters and the small tensor helpers -- draws the posed mesh: Liquid-Warping-Block inference does not use it, checking
an SMPL estimate by eye and the texture-warping baseline (W_T) do.  Forward only (no gradient of the renderer).  It runs
the rasteriser unchanged at the super-sampled size and shades its maps with the kernels of csrc/render.hip.
Limits the reference has too, reported instead of failing later: `create_coords` raises ValueError for a `tex_size`
whose `torch.arange(0, 1 + step, step)` does not have `tex_size` entries (1 and 7 among the small sizes), and `render`
refuses one-texel cubes (the reference's sampling reads texel 1 of them).
"""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib


def orthographic_proj_withz_idrot(X, cam, offset_z=0.):
    """utils/nmr.py:10-28 (kept for API compatibility; the device path fuses it into the face gather)."""
    scale = cam[:, 0].contiguous().view(-1, 1, 1)
    trans = cam[:, 1:3].contiguous().view(cam.size(0), 1, -1)
    proj_xy = scale * (X[:, :, :2] + trans)
    proj_z = X[:, :, 2, None] + offset_z
    return torch.cat((proj_xy, proj_z), 2)


class SMPLRenderer(nn.Module):
    # rasteriser defaults of neural_renderer (rasterize.py:8-13): render_fim_wim does not forward the
    # renderer's own near/far (nmr.py:277), so these are the values the reference effectively uses.
    RASTER_NEAR = 0.1
    RASTER_FAR = 100.0

    def __init__(self, face_path='assets/pretrains/smpl_faces.npy', uv_map_path='assets/pretrains/mapper.txt',
                 map_name='uv_seg', tex_size=3, image_size=256, anti_aliasing=True, fill_back=False,
                 background_color=(0, 0, 0), viewing_angle=30, near=0.1, far=25.0, has_front=False,
                 faces=None, map_fn=None, front_map_fn=None, back_map_fn=None, align_corners=False, uv_sampler=None):
        """Same signature as utils/nmr.py:104-107.  The trailing keyword arguments (extension) supply the
        face list and the face->condition tables directly; without them they are read from `face_path` and
        from `<uv_map_path stem>_<map_name>.npy` tables (see utils/mesh.py of this package).  `uv_sampler`
        (nf, tex_size**2, 2) is the static UV sampling grid of `forward(dynamic=False)`; without it the grid is built
        from `uv_map_path` when that file exists (mesh.create_uvsampler)."""
        super().__init__()
        self.background_color = background_color
        self.anti_aliasing = anti_aliasing
        self.image_size = image_size
        self.fill_back = fill_back
        self.map_name = map_name
        self.tex_size = tex_size
        self.align_corners = bool(align_corners)

        if faces is None:
            if not os.path.exists(face_path):
                raise FileNotFoundError("SMPL face list %s not found (README.md:48-68 of the reference: a download); "
                                        "pass faces=/map_fn= explicitly, e.g. from impersonator_amd.utils.synthetic" % face_path)
            faces = np.load(face_path)
        faces = np.asarray(faces)
        self.base_nf = faces.shape[0]
        if self.fill_back:
            faces = np.concatenate((faces, faces[:, ::-1]), axis=0)
        self.nf = faces.shape[0]
        self.register_buffer('faces', torch.tensor(np.ascontiguousarray(faces.astype(np.int32))).int().contiguous())

        if map_fn is None:
            from . import mesh
            map_fn = mesh.create_mapping(map_name, uv_map_path, contain_bg=True, fill_back=fill_back)
            if has_front and front_map_fn is None:
                front_map_fn = mesh.create_mapping('front', uv_map_path, contain_bg=True, fill_back=fill_back)
        self.register_buffer('map_fn', torch.as_tensor(np.ascontiguousarray(map_fn)).float().contiguous())
        if back_map_fn is not None:
            self.register_buffer('back_map_fn', torch.as_tensor(np.ascontiguousarray(back_map_fn)).float().contiguous())
        else:
            self.back_map_fn = None
        if front_map_fn is not None:
            self.register_buffer('front_map_fn', torch.as_tensor(np.ascontiguousarray(front_map_fn)).float().contiguous())
        else:
            self.front_map_fn = None

        # texture sampling grids (nmr.py:135,146-149).  A tex_size the reference cannot build coords for leaves them unset;
        # dynamic_sampler then raises create_coords' error.
        try:
            coords = self.create_coords(tex_size)
        except ValueError:
            coords = None
        self.register_buffer('coords', coords, persistent=False)
        if uv_sampler is None and tex_size >= 2 and os.path.exists(uv_map_path):
            from . import mesh
            built = mesh.create_uvsampler(uv_map_path, tex_size=tex_size)
            if built.shape[0] == self.nf:      # the file describes this face list (not so with fill_back or faces=)
                uv_sampler = built
        if uv_sampler is not None:
            uv_sampler = torch.as_tensor(np.ascontiguousarray(uv_sampler)).float().contiguous()
            if tuple(uv_sampler.shape) != (self.nf, tex_size * tex_size, 2):
                raise ValueError("uv_sampler must be (nf, tex_size**2, 2) = (%d, %d, 2), got %s"
                                 % (self.nf, tex_size * tex_size, tuple(uv_sampler.shape)))
        self.register_buffer('img2uv_sampler', uv_sampler, persistent=False)

        # light (nmr.py:164-170)
        self.light_intensity_ambient = 1
        self.light_intensity_directional = 0
        self.light_color_ambient = [1, 1, 1]
        self.light_color_directional = [1, 1, 1]
        self.light_direction = [0, 1, 0]
        self.rasterizer_eps = 1e-3

        self.near = near
        self.far = far
        self.proj_func = orthographic_proj_withz_idrot
        self.viewing_angle = viewing_angle
        self.eye = [0, 0, -(1. / np.tan(np.radians(self.viewing_angle)) + 1)]  # nmr.py:177
        self._eye_z = float(np.float32(self.eye[2]))
        self._ws = None
        self._bufs = {}       # render path: f2verts, the super-sampled maps and the light, kept between calls like _ws
        self._bg = None       # (colour tuple, device) -> its (1,3) device tensor

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _cuda(t, dtype=torch.float32):
        if not t.is_cuda:
            raise RuntimeError("impersonator_amd runs on the GPU only (got a %s tensor); there is no CPU fallback" % t.device)
        return t.to(dtype).contiguous()

    def _workspace(self, bs, nf, device):
        need = _lib.load().lwg_rasterize_workspace_bytes(bs, nf, self.image_size)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def _faces_for(self, faces):
        if faces is None:
            return self.faces
        if faces.dim() == 3:
            # the reference accepts a per-sample face list (nmr.py:264-266); the SMPL topology is shared
            if not bool((faces == faces[0:1]).all()):
                raise NotImplementedError("per-sample face topologies are not supported")
            faces = faces[0]
        return faces.int().contiguous()

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def render_fim_wim(self, cam, vertices, faces=None):
        """utils/nmr.py:263-278 -> (f2verts (bs,nf,3,3), fim int32 (bs,is,is), wim (bs,is,is,3))."""
        lib = _lib.load()
        cam, vertices = self._cuda(cam), self._cuda(vertices)
        fidx = self._faces_for(faces).to(vertices.device)
        bs, nv = vertices.shape[:2]
        nf, s, dev = fidx.shape[0], self.image_size, vertices.device
        f2verts = torch.empty((bs, nf, 3, 3), device=dev, dtype=torch.float32)
        fim = torch.empty((bs, s, s), device=dev, dtype=torch.int32)
        wim = torch.empty((bs, s, s, 3), device=dev, dtype=torch.float32)
        st = _lib.stream_ptr()
        _lib.check(lib.lwg_project_faces(_lib.ptr(vertices), _lib.ptr(cam), _lib.ptr(fidx), bs, nv, nf, self._eye_z,
                                         _lib.ptr(f2verts), st))
        ws = self._workspace(bs, nf, dev)
        _lib.check(lib.lwg_rasterize_fim_wim(_lib.ptr(f2verts), bs, nf, s, self.RASTER_NEAR, self.RASTER_FAR,
                                             _lib.ptr(fim), _lib.ptr(wim), None, _lib.ptr(ws), ws.numel(), st))
        return f2verts, fim, wim

    @torch.no_grad()
    def rasterize(self, faces, near=None, far=None, return_depth=False):
        """nr.rasterize_face_index_map_and_weight_map (rasterize.py:543-571) on given (bs,nf,3,3) faces."""
        lib = _lib.load()
        faces = self._cuda(faces)
        bs, nf = faces.shape[:2]
        s, dev = self.image_size, faces.device
        fim = torch.empty((bs, s, s), device=dev, dtype=torch.int32)
        wim = torch.empty((bs, s, s, 3), device=dev, dtype=torch.float32)
        depth = torch.empty((bs, s, s), device=dev, dtype=torch.float32) if return_depth else None
        ws = self._workspace(bs, nf, dev)
        _lib.check(lib.lwg_rasterize_fim_wim(_lib.ptr(faces), bs, nf, s,
                                             self.RASTER_NEAR if near is None else near,
                                             self.RASTER_FAR if far is None else far,
                                             _lib.ptr(fim), _lib.ptr(wim), _lib.ptr(depth), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr()))
        return (fim, wim, depth) if return_depth else (fim, wim)

    @torch.no_grad()
    def encode_fim(self, cam, vertices, fim=None, transpose=True, map_fn=None):
        """utils/nmr.py:328-341 -> (fim_enc, fim)."""
        if fim is None:
            _, fim, _ = self.render_fim_wim(cam, vertices)
        table = self.map_fn if map_fn is None else map_fn
        return self._lookup(fim, table, transpose), fim

    @torch.no_grad()
    def encode_front_fim(self, fim, transpose=True, front_fn=True):
        """utils/nmr.py:343-352."""
        table = self.front_map_fn if front_fn else self.back_map_fn
        if table is None:
            raise RuntimeError("renderer was built without the %s map" % ('front' if front_fn else 'back'))
        return self._lookup(fim, table, transpose)

    def _lookup(self, fim, table, transpose):
        fim = self._cuda(fim, torch.int32)
        table = self._cuda(table).to(fim.device)
        bs, h, w = fim.shape
        nrows, nc = table.shape
        out = torch.empty((bs, nc, h, w) if transpose else (bs, h, w, nc), device=fim.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_encode_fim(_lib.ptr(fim), _lib.ptr(table), bs, h * w, nrows, nc, int(bool(transpose)),
                                              _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def cal_bc_transform(self, src_f2pts, dst_fims, dst_wims):
        """utils/nmr.py:617-659 -> T (bs, is, is, 2).  src_f2pts (1|bs, nf, 3, 2)."""
        src = self._cuda(src_f2pts)
        fim = self._cuda(dst_fims, torch.int32)
        wim = self._cuda(dst_wims)
        bs = fim.shape[0]
        T = torch.empty((bs, self.image_size, self.image_size, 2), device=fim.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_cal_bc_transform(_lib.ptr(src), src.shape[0], _lib.ptr(fim), _lib.ptr(wim), bs,
                                                    src.shape[1], self.image_size, _lib.ptr(T), _lib.stream_ptr()))
        return T

    @torch.no_grad()
    def grid_sample(self, x, T):
        """F.grid_sample(x, T) as the reference calls it (models/imitator.py:259, impersonator_trainer.py:62): bilinear,
        zeros padding, the renderer's align_corners; x (1|n, C, H, W), T (n, Ho, Wo, 2)."""
        x, T = self._cuda(x), self._cuda(T)
        n, ho, wo, _ = T.shape
        xn, c, h, w = x.shape
        out = torch.empty((n, c, ho, wo), device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_grid_sample(_lib.ptr(x), xn, c, h, w, _lib.ptr(T), n, ho, wo, int(self.align_corners),
                                               _lib.ptr(out), _lib.stream_ptr()))
        return out

    @staticmethod
    @torch.no_grad()
    def get_vis_f2pts(f2pts, fims):
        """utils/nmr.py:506-546 (--only_vis, hazard H10): faces not in fim.unique()[1:] become -2 -- i.e. the sorted unique
        values minus the SMALLEST one present (the background's -1 whenever a background pixel exists).  CUDA tensors: two
        liblwg launches (lwg_vis_f2pts: flag the values present, select); CPU tensors: the reference's indexing."""
        if f2pts.is_cuda:
            batched = f2pts.dim() == 4
            pts = (f2pts if batched else f2pts[None]).float().contiguous()
            fim = (fims if batched else fims[None]).to(torch.int32).contiguous()
            bs, nf = pts.shape[:2]
            per_face = pts[0, 0].numel()
            lib = _lib.load()
            ws = torch.empty(lib.lwg_vis_f2pts_workspace_bytes(bs, nf), dtype=torch.uint8, device=pts.device)
            out = torch.empty_like(pts)
            _lib.check(lib.lwg_vis_f2pts(_lib.ptr(pts), bs, nf, per_face, _lib.ptr(fim), fim.shape[1], fim.shape[2], _lib.ptr(out),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
            return out if batched else out[0]

        def vis(orig, fim):
            out = torch.zeros_like(orig) - 2.0
            ids = fim.unique()[1:].long()
            out[ids] = orig[ids]
            return out
        if f2pts.dim() == 4:
            return torch.stack([vis(f2pts[i], fims[i]) for i in range(f2pts.shape[0])], dim=0)
        return vis(f2pts, fims)

    @torch.no_grad()
    def source_p2verts(self, f2verts):
        """models/imitator.py:105-107 (hazard H9) as one launch: negates y of `f2verts` (bs,nf,3,3) IN PLACE -- the reference
        does it through the `p2verts = f2verts[..., 0:2]` view -- and returns the contiguous (bs,nf,3,2) copy of that view
        which the per-frame flow kernel reads."""
        f2verts = self._cuda(f2verts)
        bs, nf = f2verts.shape[:2]
        p2 = torch.empty((bs, nf, 3, 2), device=f2verts.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_source_p2verts(_lib.ptr(f2verts), bs, nf, _lib.ptr(p2), _lib.stream_ptr()))
        return p2

    @torch.no_grad()
    def mask_compose(self, img, mask, tail, invert=False):
        """torch.cat([img * (1 - mask if invert else mask), tail], dim=1) in one launch (models/imitator.py:127-128,135):
        img (n,3,H,W), mask (n,1,H,W), tail (n,ct,H,W)."""
        img, mask, tail = self._cuda(img), self._cuda(mask), self._cuda(tail)
        n, _, h, w = img.shape
        ct = tail.shape[1]
        out = torch.empty((n, 3 + ct, h, w), device=img.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_mask_compose(_lib.ptr(img), _lib.ptr(mask), int(bool(invert)), _lib.ptr(tail), ct, n, h, w,
                                                _lib.ptr(out), _lib.stream_ptr()))
        return out

    # ------------------------------------------------------------------ textured rendering (csrc/render.hip)
    def set_ambient_light(self, int_dir=0.3, int_amb=0.7, direction=(1, 0.5, 1)):
        """utils/nmr.py:179-183."""
        self.light_intensity_directional = int_dir
        self.light_intensity_ambient = int_amb
        if direction is not None:
            self.light_direction = direction

    def set_bgcolor(self, color=(-1, -1, -1)):
        """utils/nmr.py:185-186: a colour triple, or a per-sample (bs,3) tensor."""
        self.background_color = color

    def set_tex_size(self, tex_size):
        """utils/nmr.py:188-190.  Also sets `self.tex_size`, which the reference leaves behind (its extract_tex then reshapes
        with the old size); coords land on the device the module is on."""
        coords = self.create_coords(tex_size)
        self.coords = coords.to(self.faces.device)
        self.tex_size = tex_size

    def debug_textures(self):
        """utils/nmr.py:661-662: white cubes (nf,ts,ts,ts,3) on the host; `render` takes them with or without a leading 1."""
        return torch.ones((self.nf, self.tex_size, self.tex_size, self.tex_size, 3), dtype=torch.float32)

    def _buf(self, name, shape, dtype, device):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.device != device:
            t = self._bufs[name] = torch.empty(shape, dtype=dtype, device=device)
        return t

    def _background(self, bs, device):
        """(1|bs, 3) device tensor of `background_color`; a colour triple is uploaded once and kept."""
        bg = self.background_color
        if torch.is_tensor(bg):
            bg = self._cuda(bg.to(device))
            bg = bg[None] if bg.dim() == 1 else bg
        else:
            key = (tuple(float(c) for c in np.asarray(bg, dtype=np.float64).reshape(-1)), device)
            if self._bg is None or self._bg[0] != key:
                self._bg = (key, torch.tensor([key[0]], dtype=torch.float32).to(device))
            bg = self._bg[1]
        if bg.dim() != 2 or bg.shape[1] != 3 or bg.shape[0] not in (1, bs):
            raise ValueError("background_color must be a colour triple or a (bs,3) tensor, got shape %s" % (tuple(bg.shape),))
        return bg

    def _raster_scene(self, cam, vertices, faces, size, near, far, want_depth):
        """project + rasterise at `size` into the module's cached buffers -> (f2verts, fim, wim, depth | None, face list)."""
        lib = _lib.load()
        fidx = self._faces_for(faces).to(vertices.device)
        bs, nv = vertices.shape[:2]
        nf, dev, st = fidx.shape[0], vertices.device, _lib.stream_ptr()
        f2verts = self._buf('f2verts', (bs, nf, 3, 3), torch.float32, dev)
        fim = self._buf('fim', (bs, size, size), torch.int32, dev)
        wim = self._buf('wim', (bs, size, size, 3), torch.float32, dev)
        depth = self._buf('depth', (bs, size, size), torch.float32, dev) if want_depth else None
        _lib.check(lib.lwg_project_faces(_lib.ptr(vertices), _lib.ptr(cam), _lib.ptr(fidx), bs, nv, nf, self._eye_z,
                                         _lib.ptr(f2verts), st))
        ws = self._workspace(bs, nf, dev)
        _lib.check(lib.lwg_rasterize_fim_wim(_lib.ptr(f2verts), bs, nf, size, near, far, _lib.ptr(fim), _lib.ptr(wim),
                                             _lib.ptr(depth), _lib.ptr(ws), ws.numel(), st))
        return f2verts, fim, wim, depth, fidx

    @torch.no_grad()
    def render(self, cam, vertices, textures, faces=None, get_fim=False):
        """utils/nmr.py:210-244 -> (images (bs,3,is,is), fim int32 (bs,is,is) or None).  textures (bs,nf,ts,ts,ts,3), or with a
        leading 1 / without the batch axis: one texture set shared by the batch (extension).  Lighting (on the raw vertices),
        texture sampling, background and the 2x2 average of anti-aliasing are one shading pass over the rasteriser's maps at
        near / far = self.near / self.far; the textures are read, never modified."""
        lib = _lib.load()
        cam, vertices, textures = self._cuda(cam), self._cuda(vertices), self._cuda(textures)
        if textures.dim() == 5:
            textures = textures[None]
        bs, nv = vertices.shape[:2]
        ts = textures.shape[2] if textures.dim() == 6 else 0
        if ts < 2:
            raise ValueError("render needs textures (bs|1, nf, ts, ts, ts, 3) with ts >= 2, got %s (the reference's sampling "
                             "reads texel 1 of a one-texel cube)" % (tuple(textures.shape),))
        s, dev, st = self.image_size, vertices.device, _lib.stream_ptr()
        aa = bool(self.anti_aliasing)
        f2verts, fim, wim, depth, fidx = self._raster_scene(cam, vertices, faces, s * 2 if aa else s, self.near, self.far, True)
        nf = fidx.shape[0]
        if tuple(textures.shape[1:]) != (nf, ts, ts, ts, 3) or textures.shape[0] not in (1, bs):
            raise ValueError("textures must be (%d|1, %d, ts, ts, ts, 3), got %s" % (bs, nf, tuple(textures.shape)))
        bg = self._background(bs, dev)
        light = self._buf('light', (bs, nf, 3), torch.float32, dev)
        triple = lambda v: (ctypes.c_float * 3)(*[float(c) for c in np.asarray(v, dtype=np.float64).reshape(3)])
        _lib.check(lib.lwg_face_light(_lib.ptr(vertices), _lib.ptr(fidx), bs, nv, nf, float(self.light_intensity_ambient),
                                      float(self.light_intensity_directional), triple(self.light_color_ambient),
                                      triple(self.light_color_directional), triple(self.light_direction), _lib.ptr(light), st))
        images = torch.empty((bs, 3, s, s), device=dev, dtype=torch.float32)
        _lib.check(lib.lwg_shade_resolve(_lib.ptr(f2verts), _lib.ptr(fim), _lib.ptr(wim), _lib.ptr(depth), _lib.ptr(textures),
                                         textures.shape[0], _lib.ptr(light), _lib.ptr(bg), bg.shape[0], bs, nf, s, int(aa), ts,
                                         float(self.rasterizer_eps), _lib.ptr(images), st))
        fim1 = None
        if get_fim:   # nmr.py:241: a second raster at 1x with the same planes
            fim1 = torch.empty((bs, s, s), device=dev, dtype=torch.int32)
            wim1 = self._buf('wim1', (bs, s, s, 3), torch.float32, dev)
            ws = self._workspace(bs, nf, dev)
            _lib.check(lib.lwg_rasterize_fim_wim(_lib.ptr(f2verts), bs, nf, s, self.near, self.far, _lib.ptr(fim1),
                                                 _lib.ptr(wim1), None, _lib.ptr(ws), ws.numel(), st))
        return images, fim1

    @torch.no_grad()
    def forward(self, cam, vertices, uv_imgs, dynamic=True, get_fim=False):
        """utils/nmr.py:192-208 -> (images, textures[, fim]).  dynamic: the textures are sampled from `uv_imgs` at the projected
        mesh itself; otherwise through the static UV grid `img2uv_sampler`."""
        if dynamic:
            samplers = self.dynamic_sampler(cam, vertices, None)
        else:
            if self.img2uv_sampler is None:
                raise RuntimeError("forward(dynamic=False) needs the static UV sampling grid: build the renderer with uv_sampler= "
                                   "or with a uv_map_path that exists (mesh.create_uvsampler)")
            samplers = self.img2uv_sampler.to(vertices.device)[None].expand(cam.shape[0], -1, -1, -1).contiguous()
        textures = self.extract_tex(uv_imgs, samplers)
        images, fim = self.render(cam, vertices, textures, None, get_fim=get_fim)
        return (images, textures, fim) if get_fim else (images, textures)

    @torch.no_grad()
    def render_silhouettes(self, cam, vertices, faces=None):
        """utils/nmr.py:295-310 -> alpha (bs,is,is): coverage at the rasteriser's default planes, averaged over the 2x2
        sub-pixels with anti-aliasing."""
        cam, vertices = self._cuda(cam), self._cuda(vertices)
        bs, s, aa = vertices.shape[0], self.image_size, bool(self.anti_aliasing)
        _, fim, _, _, _ = self._raster_scene(cam, vertices, faces, s * 2 if aa else s, self.RASTER_NEAR, self.RASTER_FAR, False)
        alpha = torch.empty((bs, s, s), device=vertices.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_silhouette_resolve(_lib.ptr(fim), bs, s, int(aa), _lib.ptr(alpha), _lib.stream_ptr()))
        return alpha

    def render_depth(self, cam, vertices):
        raise NotImplementedError      # utils/nmr.py:280-281

    def infer_face_index_map(self, cam, vertices):
        raise NotImplementedError      # utils/nmr.py:312-313

    @torch.no_grad()
    def extract_tex_from_image(self, images, cam, vertices):
        """utils/nmr.py:354-362: per-face texture cubes sampled from `images` (1|bs,3,h,w) under the projected mesh."""
        return self.extract_tex(images, self.dynamic_sampler(cam, vertices, None))

    @torch.no_grad()
    def extract_tex(self, uv_img, uv_sampler):
        """utils/nmr.py:364-380: uv_img (1|bs,3,h,w), uv_sampler (bs,nf,T*T,2) -> (bs,nf,T,T,T,3); F.grid_sample with the
        renderer's align_corners, repeated along the third texture axis."""
        uv_img, uv_sampler = self._cuda(uv_img), self._cuda(uv_sampler)
        t = self.tex_size
        if uv_sampler.dim() != 4 or uv_sampler.shape[2] != t * t or uv_sampler.shape[3] != 2:
            raise ValueError("uv_sampler must be (bs, nf, %d, 2) for tex_size %d, got %s" % (t * t, t, tuple(uv_sampler.shape)))
        bs, nf = uv_sampler.shape[:2]
        if uv_img.dim() != 4 or uv_img.shape[1] != 3 or uv_img.shape[0] not in (1, bs):
            raise ValueError("uv_img must be (%d|1, 3, h, w), got %s" % (bs, tuple(uv_img.shape)))
        tex = torch.empty((bs, nf, t, t, t, 3), device=uv_img.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_extract_tex(_lib.ptr(uv_img), uv_img.shape[0], uv_img.shape[2], uv_img.shape[3],
                                               _lib.ptr(uv_sampler), bs, nf, t, int(self.align_corners), _lib.ptr(tex),
                                               _lib.stream_ptr()))
        return tex

    @torch.no_grad()
    def dynamic_sampler(self, cam, vertices, faces=None):
        """utils/nmr.py:382-388 -> (bs,nf,T*T,2): batch_orth_proj_idrot, points_to_faces and points_to_sampler in one launch."""
        if self.coords is None:
            self.create_coords(self.tex_size)      # raises: the reference cannot build coords for this tex_size either
        cam, vertices = self._cuda(cam), self._cuda(vertices)
        fidx = self._faces_for(faces).to(vertices.device)
        coords = self._cuda(self.coords.to(vertices.device))
        bs, nv = vertices.shape[:2]
        nf, tt = fidx.shape[0], coords.shape[1]
        sampler = torch.empty((bs, nf, tt, 2), device=vertices.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_face_sampler(_lib.ptr(cam), _lib.ptr(vertices), _lib.ptr(fidx), _lib.ptr(coords), bs, nv, nf,
                                                tt, _lib.ptr(sampler), _lib.stream_ptr()))
        return sampler

    # the reference's small tensor helpers, as plain torch (any device)
    def project_to_image(self, cam, vertices):
        """utils/nmr.py:390-396: the projected x, y without the y flip."""
        return self.proj_func(vertices, cam)[:, :, 0:2]

    def points_to_faces(self, points, faces=None):
        """utils/nmr.py:398-415: points (bs,nv,2), faces (bs,nf,3) or the renderer's own -> (bs,nf,3,2)."""
        bs = points.shape[0]
        if faces is None:
            faces = self.faces[None].expand(bs, -1, -1)
        idx = faces.long().to(points.device)
        return torch.stack([points[b][idx[b]] for b in range(bs)], dim=0)

    @staticmethod
    def compute_barycenter(f2vts):
        """utils/nmr.py:417-432: (N,F,3,2) -> (N,F,2), v2 + (v0 - v2)/2 + (v1 - v2)/2."""
        v0, v1, v2 = f2vts[:, :, 0], f2vts[:, :, 1], f2vts[:, :, 2]
        return v2 + 0.5 * (v0 - v2) + 0.5 * (v1 - v2)

    @staticmethod
    def batch_orth_proj_idrot(camera, X):
        """utils/nmr.py:434-449: camera (N,3), X (N,P,3) -> s * (X_xy + t), (N,P,2)."""
        return camera[:, None, 0:1] * (X[:, :, :2] + camera[:, None, 1:])

    @staticmethod
    def points_to_sampler(coords, faces):
        """utils/nmr.py:451-470: coords (2,T*T), faces (bs,nf,3,2) -> (bs,nf,T*T,2) in [-1,1]."""
        v2 = faces[:, :, 2]
        edges = torch.stack((faces[:, :, 0] - v2, faces[:, :, 1] - v2), dim=-1)      # (bs,nf,2,2)
        samples = torch.matmul(edges, coords) + v2[..., None]                      # (bs,nf,2,T*T)
        return samples.permute(0, 1, 3, 2).clamp(min=-1.0, max=1.0)

    @staticmethod
    def create_coords(tex_size=3):
        """utils/nmr.py:472-488 -> (2, tex_size**2) barycentric sample points, on the host.  The reference's
        `torch.arange(0, 1 + step, step)` is kept; where its length is not tex_size (the end point is or is not reached in
        float arithmetic: tex_size 1 and 7 among the small sizes) every later reshape of the reference fails, so: ValueError."""
        step = 1 if tex_size == 1 else 1 / (tex_size - 1)
        alpha_beta = torch.arange(0, 1 + step, step, dtype=torch.float32)
        if alpha_beta.numel() != tex_size:
            raise ValueError("tex_size %d is not usable: arange(0, 1 + step, step) has %d entries" % (tex_size, alpha_beta.numel()))
        xv, yv = torch.meshgrid([alpha_beta, alpha_beta], indexing='ij')
        return torch.stack([xv.flatten(), yv.flatten()], dim=0)

    @staticmethod
    def create_meshgrid(image_size):
        """utils/nmr.py:490-504 -> (is,is,2) pixel grid in [-1,1], last axis (x, y)."""
        factor = (torch.arange(0, image_size, dtype=torch.float32) / (image_size - 1) - 0.5) * 2
        xv, yv = torch.meshgrid([factor, factor], indexing='ij')
        return torch.stack([yv, xv], dim=-1)

    def cal_transform(self, bc_f2pts, src_fim, dst_fim):
        """utils/nmr.py:587-615: T (bs,is,is,2) = bc_f2pts[b, dst_fim] on covered pixels, -2 elsewhere."""
        bs = src_fim.shape[0]
        T = torch.zeros(bs, self.image_size, self.image_size, 2, device=bc_f2pts.device) - 2
        for i in range(bs):
            covered = dst_fim[i] != -1
            T[i][covered] = bc_f2pts[i, dst_fim[i][covered].long()]
        return T

    # ------------------------------------------------------------------ fused per-frame path
    @torch.no_grad()
    def transfer(self, cam, vertices, src_p2verts, src_img):
        """models/imitator.py:250-260 in one launch sequence.  cam (bs,3), vertices (bs,nv,3), shared source
        src_p2verts (1,nf,3,2), src_img (1,3,is,is).  Returns a dict with the reference's tsf_info entries
        (f2verts, fim, wim, cond, T, tsf_img) and `tsf_inputs` = cat(tsf_img, cond) as an NCHW-shaped view of
        the NHWC8 buffer the generator reads directly."""
        lib = _lib.load()
        cam, vertices = self._cuda(cam), self._cuda(vertices)
        p2v, img = self._cuda(src_p2verts), self._cuda(src_img)
        bs, nv = vertices.shape[:2]
        nf, s, dev = self.nf, self.image_size, vertices.device
        nc = self.map_fn.shape[1]
        if p2v.shape[0] != 1 or img.shape[0] != 1:
            raise ValueError("transfer() warps ONE source onto a batch of target poses")
        out = dict(
            f2verts=torch.empty((bs, nf, 3, 3), device=dev), fim=torch.empty((bs, s, s), device=dev, dtype=torch.int32),
            wim=torch.empty((bs, s, s, 3), device=dev), cond=torch.empty((bs, nc, s, s), device=dev),
            T=torch.empty((bs, s, s, 2), device=dev), tsf_img=torch.empty((bs, 3, s, s), device=dev))
        x0 = torch.empty((bs, s, s, 8), device=dev) if nc == 3 else None
        ws = self._workspace(bs, nf, dev)
        _lib.check(lib.lwg_transfer_frame(
            _lib.ptr(vertices), _lib.ptr(cam), _lib.ptr(self.faces), bs, nv, nf, s, self._eye_z, self.RASTER_NEAR,
            self.RASTER_FAR, _lib.ptr(self.map_fn), nc, _lib.ptr(p2v), _lib.ptr(img), int(self.align_corners),
            _lib.ptr(out['f2verts']), _lib.ptr(out['fim']), _lib.ptr(out['wim']), _lib.ptr(out['cond']),
            _lib.ptr(out['T']), _lib.ptr(out['tsf_img']), _lib.ptr(x0), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        if x0 is not None:
            out['tsf_inputs'] = x0.permute(0, 3, 1, 2)[:, :3 + nc]
        else:
            out['tsf_inputs'] = torch.cat([out['tsf_img'], out['cond']], dim=1)
        return out

    @torch.no_grad()
    def animate_inputs(self, fim, wim, side, src_f2p, ref_f2p, src_img, ref_img, map_fn=None):
        """The per-frame geometry of models/animator.py in one launch (lwg_animate_inputs): the driven pose's fim (bs,is,is) /
        wim (bs,is,is,3), the per-row side bytes (nf+1), the two masked face-vertex tables (1,nf,3,2) and images (1,3,is,is).
        Returns dict(cond, T_src, T_ref, tsf_img, tsf_inputs); with a 3-channel condition map `tsf_inputs` is an NCHW-shaped
        view of the NHWC8 buffer the generator reads directly (as `transfer`), otherwise a plain NCHW tensor."""
        lib = _lib.load()
        fim, wim = self._cuda(fim, torch.int32), self._cuda(wim)
        src_f2p, ref_f2p = self._cuda(src_f2p), self._cuda(ref_f2p)
        src_img, ref_img = self._cuda(src_img), self._cuda(ref_img)
        table = self.map_fn if map_fn is None else self._cuda(map_fn)
        side = self._cuda(side, torch.uint8)
        bs, s, dev = fim.shape[0], self.image_size, fim.device
        nf, nc = src_f2p.shape[-3], table.shape[1]
        if src_f2p.numel() != nf * 6 or ref_f2p.numel() != nf * 6 or src_img.numel() != 3 * s * s or ref_img.numel() != 3 * s * s:
            raise ValueError("animate_inputs() composes ONE source and ONE reference onto a batch of target poses")
        if side.numel() != nf + 1 or table.shape[0] != nf + 1 or tuple(fim.shape[1:]) != (s, s):
            raise ValueError("animate_inputs(): side / map_fn need nf + 1 = %d rows, fim (bs, %d, %d)" % (nf + 1, s, s))
        out = dict(cond=torch.empty((bs, nc, s, s), device=dev), T_src=torch.empty((bs, s, s, 2), device=dev),
                   T_ref=torch.empty((bs, s, s, 2), device=dev), tsf_img=torch.empty((bs, 3, s, s), device=dev))
        x0 = torch.empty((bs, s, s, 8), device=dev) if nc == 3 else None
        x = torch.empty((bs, 3 + nc, s, s), device=dev) if nc != 3 else None
        _lib.check(lib.lwg_animate_inputs(
            _lib.ptr(fim), _lib.ptr(wim), bs, nf, s, _lib.ptr(table), nc, _lib.ptr(side), _lib.ptr(src_f2p), _lib.ptr(ref_f2p),
            _lib.ptr(src_img), _lib.ptr(ref_img), int(self.align_corners), _lib.ptr(out['T_src']), _lib.ptr(out['T_ref']),
            _lib.ptr(out['cond']), _lib.ptr(out['tsf_img']), _lib.ptr(x), _lib.ptr(x0), _lib.stream_ptr()))
        out['tsf_inputs'] = x0.permute(0, 3, 1, 2)[:, :3 + nc] if x0 is not None else x
        return out


def eye_z(viewing_angle=30):
    return -(1. / math.tan(math.radians(viewing_angle)) + 1)
