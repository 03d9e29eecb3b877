"""CPU: the numpy restatement of the device JPEG encoder (tests/jpeg_ref.py) equals libjpeg-turbo's output (PIL) byte for
byte, the case list of tests/test_gpu_jpeg.py reaches every branch of the entropy coder, lwg_jpeg_* validate their arguments
before touching a device, and utils/video.py writes an AVI that parses chunk by chunk."""
import ctypes
import io
import struct

import numpy as np
import pytest
from PIL import Image

from impersonator_amd import _lib
from impersonator_amd.utils import video
from tests import jpeg_ref

SIZES = ((16, 16), (32, 48), (48, 32), (64, 64))
QUALITIES = (30, 75, 95, 100)
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def pil_bytes(u8, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format='JPEG', quality=quality, subsampling=subsampling)
    return buf.getvalue()


def segments(data):
    """[(marker, payload)] of a JPEG file up to and including SOS"""
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        marker, size = data[i + 1], struct.unpack('>H', data[i + 2:i + 4])[0]
        out.append((marker, data[i + 4:i + 2 + size]))
        i += 2 + size
        if marker == 0xDA:
            return out


@pytest.mark.parametrize("subsampling", jpeg_ref.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_pil(size, quality, subsampling):
    H, W = size
    for name in jpeg_ref.PATTERNS:
        u8 = np.ascontiguousarray(jpeg_ref.to_u8(jpeg_ref.pattern(name, 1, H, W))[0].transpose(1, 2, 0))
        mine, _ = jpeg_ref.encode(u8, quality, subsampling)
        assert mine == pil_bytes(u8, quality, subsampling), name
        assert len(mine) <= jpeg_ref.stream_bytes(H, W, subsampling)


def test_huffman_tables_are_the_ones_pil_writes():
    data = pil_bytes(np.zeros((16, 16, 3), np.uint8), 75, '4:2:0')
    dht = [payload for marker, payload in segments(data) if marker == 0xC4]
    assert [p[0] for p in dht] == [0x00, 0x10, 0x01, 0x11]
    for payload, (bits, vals) in zip(dht, jpeg_ref.HUFFMAN):
        assert list(payload[1:17]) == bits and list(payload[17:]) == vals
    assert len(jpeg_ref.header(16, 16, 75, 420)) == jpeg_ref.HEADER_BYTES == data.index(b'\xff\xda') + 14
    assert data[:jpeg_ref.HEADER_BYTES] == jpeg_ref.header(16, 16, 75, 420)


def test_to_u8_is_save_cv2_img_rule():
    x = np.linspace(-1, 1, 4001, dtype=np.float32)
    assert np.array_equal(jpeg_ref.to_u8(x), ((x + 1) / 2.0 * 255).astype(np.uint8))
    edge = np.array([-1.0, 1.0, -1.0001, 1.0001, 7.0, -7.0, np.nan, np.inf, -np.inf], np.float32)
    assert jpeg_ref.to_u8(edge).tolist() == [0, 255, 0, 255, 255, 0, 0, 255, 0]


def test_gpu_case_list_reaches_every_branch_of_the_entropy_coder():
    total = dict.fromkeys(jpeg_ref.COUNTERS, 0)
    for n, H, W in jpeg_ref.GPU_SHAPES:
        for quality in jpeg_ref.GPU_QUALITIES:
            for sub in jpeg_ref.SUBSAMPLINGS:
                for name in jpeg_ref.PATTERNS:
                    _, cnt = jpeg_ref.encode_batch(jpeg_ref.pattern(name, n, H, W), quality, sub)
                    for k in total:
                        total[k] += cnt[k]
    print(total)
    assert all(total[k] > 0 for k in jpeg_ref.COUNTERS), total


def test_stream_and_workspace_bytes_need_no_device():
    lib = _lib.load()
    for H, W in ((16, 16), (32, 48), (256, 256), (512, 256)):
        for code, name in ((420, '4:2:0'), (444, '4:4:4')):
            nblocks = (H // 16) * (W // 16) * 6 if code == 420 else (H // 8) * (W // 8) * 3
            want = 623 + 2 * ((nblocks * 1658 + 7) // 8) + 2
            assert lib.lwg_jpeg_stream_bytes(H, W, code) == want == jpeg_ref.stream_bytes(H, W, name)
            assert lib.lwg_jpeg_workspace_bytes(2, H, W, code) > 2 * nblocks * 128
    assert lib.lwg_jpeg_stream_bytes(256, 256, 420) == 637297
    for bad in ((0, 16, 420), (16, -16, 420), (24, 16, 420), (16, 40, 444), (16, 16, 422)):
        assert lib.lwg_jpeg_stream_bytes(*bad) == 0 and lib.lwg_jpeg_workspace_bytes(1, *bad) == 0
    assert lib.lwg_jpeg_workspace_bytes(0, 16, 16, 420) == 0


def test_encode_refuses_before_touching_a_device():
    lib = _lib.load()
    p, big = ctypes.c_void_p(4096), 1 << 30
    enc = lambda x=p, n=1, h=16, w=16, q=75, sub=420, out=p, stride=big, lengths=p, ws=p, nb=big: lib.lwg_jpeg_encode(
        x, n, h, w, q, sub, out, stride, lengths, ws, nb, None)
    for kw in (dict(x=None), dict(out=None), dict(lengths=None), dict(ws=None)):
        assert enc(**kw) == INVALID and b"NULL" in lib.lwg_last_error(), kw
    for kw in (dict(n=0), dict(n=-1), dict(h=0), dict(w=-16), dict(q=0), dict(q=101), dict(sub=422), dict(sub=0),
               dict(x=ctypes.c_void_p(4098)), dict(ws=ctypes.c_void_p(4104)), dict(lengths=ctypes.c_void_p(4097))):
        assert enc(**kw) == INVALID, kw
    for kw in (dict(h=24), dict(w=8), dict(h=250, w=256), dict(h=24, sub=444)):
        assert enc(**kw) == UNSUPPORTED and b"16" in lib.lwg_last_error(), kw
    assert enc(nb=lib.lwg_jpeg_workspace_bytes(1, 16, 16, 420) - 1) == WORKSPACE
    assert enc(stride=lib.lwg_jpeg_stream_bytes(16, 16, 420) - 1) == WORKSPACE
    assert enc(n=3, h=64, w=64, sub=444, nb=lib.lwg_jpeg_workspace_bytes(2, 64, 64, 444)) == WORKSPACE


def test_python_wrappers_refuse_cpu_tensors_and_unknown_subsampling():
    import torch
    from impersonator_amd.utils import util
    with pytest.raises(RuntimeError):
        util.jpeg_encode(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError):
        util.jpeg_stream_bytes(16, 16, '4:2:2')
    with pytest.raises(ValueError):
        util.jpeg_stream_bytes(24, 16)
    assert util.jpeg_stream_bytes(256, 256, 420) == util.jpeg_stream_bytes(256, 256, '4:2:0') == 637297


def test_command_line_flags_default_to_off(monkeypatch):
    import os
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))   # parse() exports --gpu_ids: undone after
    import run_animate
    import run_mesh
    from impersonator_amd.options.jpeg_options import JpegOptions
    opt = JpegOptions().parse([])
    assert (opt.device_jpeg, opt.jpeg_quality, opt.jpeg_subsampling, opt.save_video) == (False, 75, 420, '')
    for cls in (JpegOptions, run_animate.AnimateJpegOptions, run_mesh.MeshOptions):
        opt = cls().parse(['--device_jpeg', '--jpeg_quality', '90', '--jpeg_subsampling', '444'])
        assert (opt.device_jpeg, opt.jpeg_quality, opt.jpeg_subsampling) == (True, 90, 444)


def test_mjpeg_avi_parses_chunk_by_chunk(tmp_path):
    W, H, fps = 48, 32, 12.5
    frames = jpeg_ref.to_u8(jpeg_ref.pattern('smooth', 5, H, W)).transpose(0, 2, 3, 1)
    streams = [jpeg_ref.encode(np.ascontiguousarray(f), 75 + k, '4:2:0')[0] for k, f in enumerate(frames)]   # odd and even sizes
    assert {len(s) & 1 for s in streams} == {0, 1}
    path = str(tmp_path / "out.avi")
    size = video.write_mjpeg_avi(path, streams, fps, (W, H))
    data = open(path, 'rb').read()
    assert size == len(data)
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI ' and struct.unpack('<I', data[4:8])[0] == len(data) - 8

    def chunks(lo, hi):
        out = []
        while lo < hi:
            fourcc, n = data[lo:lo + 4], struct.unpack('<I', data[lo + 4:lo + 8])[0]
            out.append((fourcc, lo + 8, n))
            lo += 8 + n + (n & 1)
        assert lo == hi
        return out

    top = chunks(12, len(data))
    assert [(c[0], data[c[1]:c[1] + 4]) for c in top[:2]] == [(b'LIST', b'hdrl'), (b'LIST', b'movi')] and top[2][0] == b'idx1'
    hdrl = chunks(top[0][1] + 4, top[0][1] + top[0][2])
    assert hdrl[0][0] == b'avih' and hdrl[0][2] == 56
    avih = struct.unpack('<14I', data[hdrl[0][1]:hdrl[0][1] + 56])
    assert avih[0] == 80000 and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (W, H)
    assert hdrl[1][0] == b'LIST' and data[hdrl[1][1]:hdrl[1][1] + 4] == b'strl'
    strl = chunks(hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [(c[0], c[2]) for c in strl] == [(b'strh', 56), (b'strf', 40)]
    strh = data[strl[0][1]:strl[0][1] + 56]
    assert strh[:8] == b'vidsMJPG'
    scale, rate, _, length = struct.unpack('<4I', strh[20:36])
    assert rate / scale == fps and length == 5
    strf = struct.unpack('<IiiHH4s', data[strl[1][1]:strl[1][1] + 20])
    assert strf == (40, W, H, 1, 24, b'MJPG')
    movi_at = top[1][1]                                     # position of the 'movi' fourcc
    movi = chunks(movi_at + 4, movi_at + top[1][2])
    assert len(movi) == 5
    index = data[top[2][1]:top[2][1] + top[2][2]]
    assert len(index) == 16 * 5
    for k, (fourcc, at, n) in enumerate(movi):
        assert fourcc == b'00dc' and data[at:at + n] == streams[k]
        ckid, flags, off, n_idx = struct.unpack('<4sIII', index[16 * k:16 * k + 16])
        assert (ckid, flags, n_idx) == (b'00dc', 0x10, n) and movi_at + off == at - 8
        img = Image.open(io.BytesIO(data[at:at + n]))
        assert img.size == (W, H) and img.mode == 'RGB'
        img.load()
    with pytest.raises(ValueError):
        video.write_mjpeg_avi(path, [], fps, (W, H))
    with pytest.raises(ValueError):
        video.write_mjpeg_avi(path, [b'not a jpeg'], fps, (W, H))
