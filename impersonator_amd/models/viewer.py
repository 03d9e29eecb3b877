"""Viewer (novel view synthesis) on MI355X -- reference surface: models/viewer.py:240-314.

Same kernels as the Imitator: rotate the personalised source mesh, render -> cond -> T -> warped source ->
generator.inference -> blend (viewer.py:273-314).

Extensions: `views` (n views of the source in blocks of `opt.batch_size`), `view_graph` (one HIP-graph replay per view) and
`rotate_trans_batch` (one mesh under n rigid transforms in one launch), all bit-identical to `view` / `rotate_trans`."""
import torch

from ..utils import cv_utils
from .imitator import Imitator


class Viewer(Imitator):
    def __init__(self, opt, **kwargs):
        super().__init__(opt, **kwargs)
        self._name = 'Viewer'
        self.T = None

    def rotate_trans(self, rt, t, X):
        """viewer.py:240-247: X @ R + t with R = euler2matrix(rt) -- one liblwg launch (lwg_rotate_translate): the rotation and
        the translation are twelve host floats handed to the kernel by value."""
        import numpy as np
        from .. import _lib
        if not X.is_cuda:
            raise RuntimeError("Viewer.rotate_trans: the mesh must be a CUDA tensor (no CPU path)")
        R = np.ascontiguousarray(np.asarray(cv_utils.euler2matrix(rt), dtype=np.float32).reshape(3, 3))
        tv = np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(3))
        x = X.float().contiguous()
        out = torch.empty_like(x)
        _lib.check(_lib.load().lwg_rotate_translate(_lib.ptr(x), x.numel() // 3, R.ctypes.data, tv.ctypes.data, _lib.ptr(out),
                                                    _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def view(self, rt, t, visualizer=None, name='1'):
        """viewer.py:273-303 -> preds (1,3,is,is)."""
        src_info = self.src_info
        tsf_mesh = self.rotate_trans(rt, t, src_info['verts'])
        out = self.render.transfer(src_info['cam'], tsf_mesh, src_info['p2verts_c'], src_info['img'])
        self.T = out['T']
        self.tsf_info = dict(verts=tsf_mesh, cam=src_info['cam'], fim=out['fim'], wim=out['wim'], cond=out['cond'],
                             tsf_img=out['tsf_img'], T=out['T'])
        bg = src_info['bg'] if getattr(self._opt, 'bg_replace', False) else torch.zeros_like(src_info['bg'])
        enc, res = src_info['feats']
        preds, _, tsf_mask = self.generator.inference(enc, res, out['tsf_inputs'], out['T'], bg_img=bg)
        if self._opt.front_warp:
            preds = self.warp_front(preds, tsf_mask)
        if visualizer is not None:
            visualizer.vis_named_img('src_img', src_info['img'])
            visualizer.vis_named_img('pred_' + name, preds)
            visualizer.vis_named_img('cond_' + name, out['cond'])
        return preds

    # ------------------------------------------------------------------ many views of one source (extension)
    @staticmethod
    def rigid_table(rts, ts):
        """(n, 12) float32 host table, row k = [euler2matrix(rts[k]) row-major, t_k]: the twelve float32s `rotate_trans` hands to
        its kernel for view k.  `ts` is (n, 3), or (3,) for one translation shared by every view."""
        import numpy as np
        n = len(rts)
        tv = np.asarray(ts, dtype=np.float32)
        if tv.ndim == 1:
            tv = np.broadcast_to(tv.reshape(1, 3), (n, 3))
        if tv.shape != (n, 3):
            raise ValueError("ts must be (3,) or (%d, 3), got %s" % (n, tv.shape))
        table = np.empty((n, 12), dtype=np.float32)
        for k in range(n):
            table[k, :9] = np.asarray(cv_utils.euler2matrix(rts[k]), dtype=np.float32).reshape(9)
            table[k, 9:] = tv[k]
        return table

    @staticmethod
    def _rigid_views(X, table_dev):
        """(n, nv, 3): the mesh X under every row of the DEVICE table (n, 12) -- one lwg_rigid_views launch."""
        from .. import _lib
        x = X.float().contiguous()
        n, nv = table_dev.shape[0], x.numel() // 3
        out = torch.empty((n, nv, 3), device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().lwg_rigid_views(_lib.ptr(x), nv, _lib.ptr(table_dev), n, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def rotate_trans_batch(self, rts, ts, X):
        """`rotate_trans` for n views of ONE mesh X (1, nv, 3) -> (n, nv, 3): the rotations are built on the host exactly as
        `rotate_trans` builds them, uploaded once as an (n, 12) table, and applied by one launch (lwg_rigid_views).  Slice k is
        bit-identical to rotate_trans(rts[k], ts[k], X)."""
        if not X.is_cuda:
            raise RuntimeError("Viewer.rotate_trans_batch: the mesh must be a CUDA tensor (no CPU path)")
        if X.dim() == 3 and X.shape[0] != 1:
            raise ValueError("rotate_trans_batch transforms ONE mesh, got a batch of %d" % X.shape[0])
        table = torch.from_numpy(self.rigid_table(rts, ts)).to(X.device)
        return self._rigid_views(X, table)

    def _view_block(self, meshes, bg):
        """viewer.py:276-299 for a block of transformed meshes (n, nv, 3); sets `tsf_info` / `T`, returns preds (n, 3, s, s)."""
        src_info = self.src_info
        n = meshes.shape[0]
        cam = src_info['cam'].reshape(1, 3).expand(n, -1).contiguous()
        out = self.render.transfer(cam, meshes, src_info['p2verts_c'], src_info['img'])
        self.T = out['T']
        self.tsf_info = dict(verts=meshes, cam=cam, fim=out['fim'], wim=out['wim'], cond=out['cond'],
                             tsf_img=out['tsf_img'], T=out['T'])
        enc, res = src_info['feats']
        preds, _, tsf_mask = self.generator.inference(enc, res, out['tsf_inputs'], out['T'], bg_img=bg)
        if self._opt.front_warp:
            preds = self.warp_front(preds, tsf_mask)
        return preds, out

    def _view_bg(self):
        bg = self.src_info['bg']
        return bg if getattr(self._opt, 'bg_replace', False) else torch.zeros_like(bg)

    @torch.no_grad()
    def views(self, rts, ts, visualizer=None):
        """(extension) `view` for n views at once -> preds (n, 3, is, is), view k bit-identical to view(rts[k], ts[k]): a
        turntable is one mesh under n rigid transforms, and every kernel downstream is batch-invariant.  The views are processed
        in blocks of `opt.batch_size` (the last one may be shorter), each block one launch sequence: lwg_rigid_views ->
        render.transfer -> generator.inference (-> warp_front).  Afterwards `tsf_info` and `T` describe the last block."""
        if self.src_info is None:
            raise RuntimeError("views: personalize a source first")
        n = len(rts)
        if n == 0:
            raise ValueError("views: no view given")
        import numpy as np
        rts = [rts[k] for k in range(n)]
        tv = np.asarray(ts, dtype=np.float32)
        tv = np.broadcast_to(tv.reshape(1, 3), (n, 3)) if tv.ndim == 1 else tv
        bs = max(1, int(self._opt.batch_size))
        bg = self._view_bg()
        preds = []
        for s in range(0, n, bs):
            meshes = self.rotate_trans_batch(rts[s:s + bs], tv[s:s + bs], self.src_info['verts'])
            p, out = self._view_block(meshes, bg)
            preds.append(p)
            if visualizer is not None:
                visualizer.vis_named_img('src_img', self.src_info['img'])
                for i in range(p.shape[0]):
                    visualizer.vis_named_img('pred_%d' % (s + i), p[i:i + 1])
                    visualizer.vis_named_img('cond_%d' % (s + i), out['cond'][i:i + 1])
        return preds[0] if len(preds) == 1 else torch.cat(preds, dim=0)

    @torch.no_grad()
    def view_graph(self, batch=1):
        """(extension) `view` for `batch` views -- lwg_rigid_views + render.transfer + generator.inference (+ warp_front) --
        captured once as a HIP graph and replayed per call: at batch 1 the kernels of a view are launch-bound when they are issued
        one by one from Python, one graph launch is not.  `lwg_rotate_translate` takes its rotation by value, which a capture would
        freeze; the captured kernel reads a static (batch, 12) device table instead, and `run` overwrites that table.
        Returns `run(rts, ts) -> preds` (one rotation (3,) / translation (3,) at batch 1, else `batch` of them): the same values as
        `view`, bit for bit (same kernels, same order); `preds` and `self.tsf_info` are the graph's own static tensors, overwritten
        by the next call.  The source must be personalised first; personalising another source, or changing the generator's
        precision, `opt.bg_replace` or `opt.front_warp`, needs a new graph."""
        import numpy as np
        if self.src_info is None:
            raise RuntimeError("view_graph: personalize a source first")
        batch = int(batch)
        if batch < 1:
            raise ValueError("view_graph: batch must be positive")
        src_info = self.src_info
        dev = src_info['img'].device
        static_rt = torch.zeros((batch, 12), device=dev, dtype=torch.float32)
        static_rt[:, 0::4] = 1.0                 # identity rotations for the eager passes
        bg = self._view_bg()
        self.generator.reserve(batch)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):            # eager passes first: handles, scratch, per-device kernel attributes exist afterwards
            for _ in range(2):
                self._view_block(self._rigid_views(src_info['verts'], static_rt), bg)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            preds, _ = self._view_block(self._rigid_views(src_info['verts'], static_rt), bg)
        info, T = self.tsf_info, self.T
        tuned = self._tuned

        def run(rts, ts):
            if self._tuned != tuned:
                raise RuntimeError("view_graph: post_personalize changed the weights and the source features since this graph was "
                                   "recorded; record a new one")
            if batch == 1 and np.ndim(rts) == 1:
                rts = [rts]
            if len(rts) != batch:
                raise ValueError("this graph was captured for %d views, got %d" % (batch, len(rts)))
            static_rt.copy_(torch.from_numpy(self.rigid_table(rts, ts)), non_blocking=True)
            graph.replay()
            self.tsf_info, self.T = info, T
            return preds

        run.graph, run.static_rt, run.preds = graph, static_rt, preds
        # what the captured kernels read or scribble on through raw pointers and nothing else would keep alive: the background
        # (a temporary when bg_replace is off) and the rasteriser's workspace (the renderer replaces it when a larger batch comes)
        run.keep = (bg, self.render._ws)
        return run
