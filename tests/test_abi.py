"""CPU checks of the drop-in boundary: liblwg.so builds, loads, and exports exactly what include/lwg.h declares.
No compute entry point is called here (no GPU in the build container)."""
import ctypes
import subprocess

import pytest

from impersonator_amd import _lib, build


def test_library_builds_for_gfx950():
    path = build.build()
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-S", path], capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out or "hip_fatbin" in out


def test_every_header_symbol_is_exported_and_bound():
    lib = _lib.load()
    names = _lib.header_symbols()
    assert len(names) >= 25
    assert names == sorted(_lib._PROTOS), "ctypes prototypes out of sync with include/lwg.h"
    for n in names:
        assert hasattr(lib, n), n


def test_version_and_error_text():
    lib = _lib.load()
    assert lib.lwg_version() >= 100
    assert isinstance(lib.lwg_last_error(), bytes)


def test_argument_validation_without_a_device():
    # validation happens before any HIP call, so these paths are exercised on CPU
    lib = _lib.load()
    assert lib.lwg_rasterize_workspace_bytes(8, 13776, 256) > 8 * 256 * 256 * 8
    assert lib.lwg_rasterize_workspace_bytes(0, 1, 1) == 0
    assert lib.lwg_rasterize_fim_wim(None, 1, 1, 8, 0.1, 100.0, None, None, None, None, 0, None) == -1
    assert b"NULL" in lib.lwg_last_error()
    assert lib.lwg_grid_sample(None, 1, 1, 1, 1, None, 1, 1, 1, 0, None, None) == -1
    assert lib.lwg_generator_missing_weights(None) == -1
    # lwg_inpaint_attention: every refusal comes before the first launch (the pointers below are never dereferenced)
    ws_bytes = lib.lwg_inpaint_attention_workspace_bytes
    for n, chunks in ((256, 8), (1024, 16), (2304, 12), (4096, 16)):   # the key chunks lwg_inpaint_create picks
        assert ws_bytes(n, 1, 0) == chunks * n * (128 + 2) * 4 == ws_bytes(n, 1, chunks), n
    assert ws_bytes(1024, 1, 2) == 2 * 1024 * 130 * 4
    assert ws_bytes(1024, 0, 0) == 0 and ws_bytes(0, 1, 0) == 0 and ws_bytes(1000, 1, 0) == 0 and ws_bytes(1024, 1, 3) == 0
    p = ctypes.c_void_p(4096)
    big = 1 << 30
    attn = lambda qkv, bias, x, n, kernel, chunks, split, out, ws, nbytes: lib.lwg_inpaint_attention(
        qkv, bias, x, 0.5, n, kernel, chunks, split, out, ws, nbytes, None)
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    for nulled in range(4):                                       # NULL qkv / bias / x / out
        args = [p, p, p, p]
        args[nulled] = None
        assert attn(args[0], args[1], args[2], 1024, 1, 0, 0, args[3], p, big) == INVALID
        assert b"NULL" in lib.lwg_last_error()
    assert attn(p, p, p, 1024, 1, 0, 0, p, None, 0) == INVALID        # the matrix-core kernel needs its workspace
    assert attn(p, p, p, 0, 0, 0, 0, p, None, 0) == INVALID           # N <= 0
    assert attn(p, p, p, -64, 1, 0, 0, p, p, big) == INVALID
    assert attn(p, p, p, 1024, 2, 0, 0, p, p, big) == INVALID         # no such kernel
    assert attn(p, p, p, 1024, 1, -1, 0, p, p, big) == INVALID
    assert attn(ctypes.c_void_p(4100), p, p, 1024, 0, 0, 0, p, None, 0) == INVALID   # float4 accesses: 16-byte alignment
    assert attn(p, p, p, 96, 0, 0, 0, p, None, 0) == UNSUPPORTED      # vector ALU: 64 queries per workgroup
    assert attn(p, p, p, 1024, 0, 0, 1, p, None, 0) == UNSUPPORTED    # vector ALU: no split-bf16 output
    assert attn(p, p, p, 320, 1, 0, 0, p, p, big) == UNSUPPORTED      # matrix cores: 256 queries per workgroup
    assert attn(p, p, p, 1024, 1, 3, 0, p, p, big) == UNSUPPORTED     # 1024 keys are not 3 chunks of whole 32-key tiles
    assert attn(p, p, p, 1024, 1, 64, 0, p, p, big) == UNSUPPORTED    # 16 keys per chunk: less than a tile
    assert b"key chunks" in lib.lwg_last_error()
    assert attn(p, p, p, 1024, 1, 0, 0, p, p, ws_bytes(1024, 1, 0) - 1) == WORKSPACE
    # lwg_stem_forward (x, N, H, W, w_host, cin, precision, y, partials, max_workgroups, stream): refusals before any HIP call
    stem = lib.lwg_stem_forward
    assert stem(p, 1, 2, 128, None, 6, 1, p, p, 0, None) == INVALID and b"NULL" in lib.lwg_last_error()
    assert stem(None, 1, 2, 128, p, 6, 1, p, p, 0, None) == INVALID
    assert stem(p, 1, 2, 128, p, 6, 1, None, p, 0, None) == INVALID
    for n, h, w in ((0, 2, 128), (1, 0, 128), (1, 2, 0), (-1, 2, 128)):
        assert stem(p, n, h, w, p, 6, 1, p, None, 0, None) == INVALID
    assert stem(p, 1, 2, 128, p, 0, 1, p, None, 0, None) == INVALID          # cin < 1
    assert stem(p, 1, 2, 128, p, 6, 2, p, None, 0, None) == INVALID          # no such precision
    assert stem(p, 1, 2, 128, p, 6, 1, p, None, -1, None) == INVALID         # negative grid cap
    assert stem(ctypes.c_void_p(4104), 1, 2, 128, p, 6, 1, p, None, 0, None) == INVALID   # float4 loads of x
    assert b"aligned" in lib.lwg_last_error()
    for precision in (0, 1):
        assert stem(p, 1, 2, 128, p, 7, precision, p, None, 0, None) == UNSUPPORTED   # NHWC8 carries six channels
        assert stem(p, 1, 2, 192, p, 6, precision, p, None, 0, None) == UNSUPPORTED   # W % 128
        assert stem(p, 1, 3, 128, p, 6, precision, p, None, 0, None) == UNSUPPORTED   # H % 2
    assert b"tile" in lib.lwg_last_error()
    # lwg_heads_inference (x, N, H, W, scale_shift, w, w_rows, precision, bg, bg_bs, color, mask, pred, bands, ws, bytes, stream)
    hws = lib.lwg_heads_inference_workspace_bytes
    assert hws(2, 8, 27) == 49 * 64 * 4 * 4 + 28 * 2 * 64 * 16 and hws(0, 8, 27) == 0 and hws(2, 8, -1) == 0
    heads = lambda x=p, n=2, h=8, w=27, ss=p, wt=p, rows=4, prec=1, bg=p, bg_bs=2, c=p, m=p, pr=p, bands=0, ws=p, nb=big: \
        lib.lwg_heads_inference(x, n, h, w, ss, wt, rows, prec, bg, bg_bs, c, m, pr, bands, ws, nb, None)
    for kw in (dict(x=None), dict(ss=None), dict(wt=None), dict(ws=None), dict(c=None, m=None, pr=None)):
        assert heads(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(n=0), dict(h=0), dict(w=-3), dict(rows=3), dict(prec=2), dict(bands=-1), dict(bg=None), dict(bg_bs=3),
               dict(bg_bs=0), dict(x=ctypes.c_void_p(4104)), dict(ws=ctypes.c_void_p(4104))):
        assert heads(**kw) == INVALID, kw
    assert heads(bg=None) == INVALID and b"background" in lib.lwg_last_error()                  # pred without bg
    assert heads(nb=hws(2, 8, 27) - 1) == WORKSPACE
    assert heads(prec=0, nb=hws(2, 8, 27) - 1) == WORKSPACE
    # lwg_conv2d_backward_weight (desc, x, dy, dw, dbias, ws, bytes, stream): NULL arguments and the dispatcher's own refusals
    # (tests/test_wgrad_plan.py) come before any HIP call
    from impersonator_amd.ops import _Desc
    wgrad = lambda d, x=p, dy=p, dw=p, ws=p: lib.lwg_conv2d_backward_weight(ctypes.byref(d), x, dy, dw, None, ws, big, None)
    d64 = _Desc(1, 32, 32, 64, 64, 3, 1, 1, 0, 1)
    assert big >= lib.lwg_conv2d_workspace_bytes(ctypes.byref(d64)) > 0
    for kw in (dict(x=None), dict(dy=None), dict(dw=None), dict(ws=None)):
        assert wgrad(d64, **kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    assert lib.lwg_conv2d_backward_weight(None, p, p, p, None, p, big, None) == INVALID
    assert wgrad(_Desc(1, 32, 32, 64, 32, 3, 1, 1, 0, 1)) == UNSUPPORTED and b"multiple of 64" in lib.lwg_last_error()
    assert wgrad(_Desc(1, 32, 32, 32, 64, 3, 2, 1, 1, 0)) == UNSUPPORTED      # transposed: Cin is the gradient side
    # lwg_norm_conv_forward (desc, x, w, bn, in_scale_shift, raw_from, y, partials, variant, ws, bytes, stream): NULL arguments,
    # bad sizes and every refusal of the conv dispatcher come before the first launch
    nws = lambda d: lib.lwg_norm_conv_workspace_bytes(ctypes.byref(d))
    nconv = lambda d, x=p, w=p, bn=0, ss=None, raw_from=0, y=p, part=p, ws=p, nb=big: lib.lwg_norm_conv_forward(
        ctypes.byref(d), x, w, bn, ss, raw_from, y, part, None, ws, nb, None)
    halo = _Desc(1, 4, 32, 32, 64, 3, 1, 1, 0, 1)
    assert lib.lwg_norm_conv_workspace_bytes(None) == 0 and nws(_Desc(1, 4, 32, 24, 64, 3, 1, 1, 0, 1)) == 0
    assert big >= nws(halo) > 0 and nws(halo) == nws(_Desc(1, 4, 32, 32, 64, 3, 1, 1, 0, 0))
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(part=None), dict(ws=None)):
        assert nconv(halo, **kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    assert lib.lwg_norm_conv_forward(None, p, p, 0, None, 0, p, p, None, p, big, None) == INVALID
    for kw in (dict(bn=16), dict(bn=-1), dict(x=ctypes.c_void_p(4104)), dict(ws=ctypes.c_void_p(4104)), dict(ss=ctypes.c_void_p(4100))):
        assert nconv(halo, **kw) == INVALID, kw
    assert nconv(_Desc(1, 4, 32, 32, 64, 3, 1, 1, 0, 2)) == INVALID                    # no such precision
    assert nconv(_Desc(0, 4, 32, 32, 64, 3, 1, 1, 0, 1)) == INVALID                    # empty batch
    assert nconv(halo, nb=nws(halo) - 1) == WORKSPACE
    assert nconv(_Desc(1, 10, 10, 32, 64, 3, 1, 1, 0, 0)) == UNSUPPORTED and b"128" in lib.lwg_last_error()   # not whole tiles
    assert nconv(_Desc(1, 4, 32, 32, 96, 3, 1, 1, 0, 1)) == UNSUPPORTED                # Cout not a power of two
    assert nconv(_Desc(1, 4, 32, 32, 64, 3, 1, 1, 0, 1), bn=128) == UNSUPPORTED        # Cout 64 on the 128-channel tile
    assert nconv(_Desc(1, 4, 32, 32, 64, 3, 1, 1, 0, 1), bn=32) == UNSUPPORTED         # 32-channel tiles: exact fp32 only
    assert nconv(_Desc(1, 16, 16, 8, 64, 7, 1, 3, 0, 1)) == UNSUPPORTED                # bf16x3 needs Cin % 32 == 0
    assert nconv(_Desc(1, 16, 16, 8, 64, 7, 1, 3, 0, 0), bn=128) == UNSUPPORTED        # small Cin: 64-channel tile only
    raw64 = _Desc(1, 4, 32, 64, 64, 3, 1, 1, 0, 1)
    assert nconv(raw64, ss=p, raw_from=16) == UNSUPPORTED and b"raw" in lib.lwg_last_error()   # not a 32-channel boundary
    assert nconv(raw64, ss=p, raw_from=64) == UNSUPPORTED and nconv(raw64, ss=p, raw_from=-32) == UNSUPPORTED
    assert nconv(_Desc(1, 4, 32, 64, 64, 1, 1, 0, 0, 1), ss=p, raw_from=0) == UNSUPPORTED      # 1x1: the ring kernel takes no raw input
    assert nconv(_Desc(1, 4, 32, 64, 64, 3, 1, 1, 0, 0), ss=p, raw_from=0) == UNSUPPORTED      # nor does exact fp32
    # lwg_norm_finalize (partials, nphase, mtiles, N, C, gamma, beta, eps, scale_shift, stream)
    fin = lambda part=p, nphase=1, mtiles=6, n=3, c=64, gamma=p, beta=p, eps=1e-5, ss=p: lib.lwg_norm_finalize(
        part, nphase, mtiles, n, c, gamma, beta, eps, ss, None)
    for kw in (dict(part=None), dict(gamma=None), dict(beta=None), dict(ss=None)):
        assert fin(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(nphase=0), dict(nphase=5), dict(mtiles=0), dict(n=0), dict(c=0), dict(eps=-1.0), dict(part=ctypes.c_void_p(4100)),
               dict(ss=ctypes.c_void_p(4100))):
        assert fin(**kw) == INVALID, kw
    assert fin(mtiles=7) == UNSUPPORTED and b"split over" in lib.lwg_last_error()      # tiles of an image are whole
    # lwg_norm_apply (raw, N, H, W, C, scale_shift, relu, dst, ld_dst, res, ld_res, split, nwarp, src0, n0, T0, src1, n1, T1,
    # align_corners, lanes, stream)
    app = lambda raw=p, n=3, h=4, w=32, c=32, ss=p, relu=1, dst=p, ld_dst=32, res=None, ld_res=0, split=0, nwarp=0, s0=None, n0=1, \
        t0=None, s1=None, n1=1, t1=None, align=0, lanes=0: lib.lwg_norm_apply(
            raw, n, h, w, c, ss, relu, dst, ld_dst, res, ld_res, split, nwarp, s0, n0, t0, s1, n1, t1, align, lanes, None)
    for kw in (dict(raw=None), dict(ss=None), dict(dst=None), dict(nwarp=1), dict(nwarp=1, s0=p), dict(nwarp=2, s0=p, t0=p)):
        assert app(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(c=0), dict(nwarp=3), dict(nwarp=-1), dict(lanes=2), dict(split=2), dict(relu=2),
               dict(align=2), dict(ld_dst=16), dict(res=p, ld_res=16), dict(nwarp=1, s0=p, t0=p, n0=2), dict(nwarp=1, s0=p, t0=p, n0=0),
               dict(raw=ctypes.c_void_p(4104)), dict(dst=ctypes.c_void_p(4104)), dict(res=ctypes.c_void_p(4104), ld_res=32),
               dict(nwarp=1, s0=ctypes.c_void_p(4104), t0=p), dict(nwarp=1, s0=p, t0=ctypes.c_void_p(4100))):
        assert app(**kw) == INVALID, kw
    for kw in (dict(c=6, ld_dst=8), dict(c=8, ld_dst=10), dict(c=8, ld_dst=8, res=p, ld_res=10), dict(lanes=8),
               dict(split=1, c=16, ld_dst=32), dict(split=1, ld_dst=48), dict(split=1, dst=ctypes.c_void_p(4096 + 64)),
               dict(split=1, res=p, ld_res=48), dict(split=1, res=ctypes.c_void_p(4096 + 64), ld_res=32)):
        assert app(**kw) == UNSUPPORTED, kw


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = ctypes.c_void_p()
    rc = _lib.load().lwg_generator_create(ctypes.byref(h), 6, 6, 64, 6, 256, 8)
    assert rc == -4 and h.value is None
    from impersonator_amd.networks.generator import ImpersonatorGenerator
    G = ImpersonatorGenerator(bg_dim=4, src_dim=6, tsf_dim=6)
    with pytest.raises(RuntimeError):
        G.encode_src(torch.zeros(1, 6, 256, 256))


def test_product_package_never_imports_the_oracle():
    import os
    root = os.path.dirname(os.path.abspath(build.__file__))
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "raster_ref" not in text, f
