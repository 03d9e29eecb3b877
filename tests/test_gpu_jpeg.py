"""GPU: the device JPEG encoder (csrc/jpeg.hip, util.jpeg_encode / jpeg_bytes) writes the same bytes as the integer restatement
tests/jpeg_ref.py -- which tests/test_jpeg_host.py ties to libjpeg-turbo -- for every shape, quality, subsampling and pattern of
jpeg_ref's case list; the uint8 rule, determinism across calls and streams, and the drivers' --device_jpeg path end to end."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, features

from impersonator_amd import demo
from impersonator_amd.utils import util
from tests import jpeg_ref

pytestmark = pytest.mark.gpu


def device_streams(x, quality, subsampling):
    """-> ([bytes per frame], lengths list, the raw (N, stride) uint8 host array)"""
    out, lengths = util.jpeg_encode(torch.from_numpy(np.ascontiguousarray(x)).cuda(), quality=quality, subsampling=subsampling)
    assert out.dtype == torch.uint8 and lengths.dtype == torch.int32 and out.shape[0] == lengths.shape[0] == x.shape[0]
    assert out.shape[1] == jpeg_ref.stream_bytes(x.shape[2], x.shape[3], subsampling)
    lens = lengths.cpu().tolist()
    host = out.cpu().numpy()
    return [host[i, :n].tobytes() for i, n in enumerate(lens)], lens, host


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return "lengths %d / %d, first differing byte %s" % (len(a), len(b), int(d[0]) if len(d) else None)


@pytest.mark.parametrize("subsampling", jpeg_ref.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", jpeg_ref.GPU_QUALITIES)
@pytest.mark.parametrize("shape", jpeg_ref.GPU_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_bytes_equal_the_restatement(shape, quality, subsampling):
    n, H, W = shape
    for name in jpeg_ref.PATTERNS:
        x = jpeg_ref.pattern(name, n, H, W)
        want, _ = jpeg_ref.encode_batch(x, quality, subsampling)
        got, lens, _ = device_streams(x, quality, subsampling)
        assert lens == [len(w) for w in want], (name, lens)
        for k in range(n):
            assert got[k] == want[k], (name, k, first_difference(got[k], want[k]))
            img = Image.open(io.BytesIO(got[k]))
            assert img.size == (W, H) and img.mode == 'RGB'
            img.load()
        if n > 1:
            assert len(set(got)) == n, "frames of a batch have different content: so have their streams"


def test_pil_encodes_the_same_bytes():
    """the streams against PIL's own encoder alone, at the project's frame size"""
    if not features.check_feature('libjpeg_turbo'):
        pytest.skip("PIL is not libjpeg-turbo-backed: its encoder is not the one restated (the restatement test is the gate)")
    x = jpeg_ref.pattern('specks', 2, 256, 256)
    u8 = jpeg_ref.to_u8(x).transpose(0, 2, 3, 1)
    for quality, subsampling in ((75, '4:2:0'), (95, '4:4:4')):
        got = util.jpeg_bytes(torch.from_numpy(x).cuda(), quality=quality, subsampling=subsampling)
        for k in range(2):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(u8[k])).save(buf, format='JPEG', quality=quality, subsampling=subsampling)
            assert got[k] == buf.getvalue(), (quality, subsampling, k, first_difference(got[k], buf.getvalue()))


def test_uint8_rule():
    """values exactly +-1, the float32 neighbours of every k / 127.5 - 1, values slightly out of range, NaN: the decoded
    picture is a function of the uint8 image alone, so equal bytes at quality 100 / 4:4:4 mean equal uint8 values"""
    k = np.arange(256, dtype=np.float64)
    edge = (k / 127.5 - 1).astype(np.float32)
    vals = np.concatenate([edge, np.nextafter(edge, np.float32(2)), np.nextafter(edge, np.float32(-2)),
                           np.array([-1.0, 1.0, -1.0000001, 1.0000001, -1.001, 1.001, 3.0, -3.0, np.nan, np.inf, -np.inf, 0.0],
                                    np.float32)]).astype(np.float32)
    assert len(np.unique(jpeg_ref.to_u8(vals))) == 256
    x = np.resize(vals, 3 * 32 * 32).reshape(1, 3, 32, 32).astype(np.float32)
    x[0, 1] = x[0, 1, ::-1]              # other values meet in one pixel
    x[0, 2] = x[0, 2].T
    for quality, sub in ((100, '4:4:4'), (75, '4:2:0')):
        want, _ = jpeg_ref.encode_batch(x, quality, sub)
        got, _, _ = device_streams(x, quality, sub)
        assert got == want, first_difference(got[0], want[0])
    # one value per picture: the DC term alone tells neighbouring uint8 values apart at quality 100
    for v in (np.nextafter(np.float32(1), np.float32(0)), np.float32(np.nan), np.float32(1.0000001), edge[77], np.nextafter(edge[77], np.float32(-2))):
        flat = np.full((1, 3, 16, 16), v, np.float32)
        assert device_streams(flat, 100, '4:4:4')[0] == jpeg_ref.encode_batch(flat, 100, '4:4:4')[0], v


def test_two_calls_and_another_stream_give_identical_bytes():
    x = torch.from_numpy(jpeg_ref.pattern('noise', 3, 64, 64)).cuda()
    first = util.jpeg_bytes(x, quality=75)
    assert util.jpeg_bytes(x, quality=75) == first
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = util.jpeg_bytes(x, quality=75)
    torch.cuda.current_stream().wait_stream(side)
    assert other == first


def test_jpeg_encode_refuses_what_the_library_refuses():
    from impersonator_amd import _lib
    with pytest.raises(_lib.LwgError) as err:
        util.jpeg_encode(torch.zeros(1, 3, 24, 16, device='cuda'))
    assert err.value.code == -2
    with pytest.raises(_lib.LwgError) as err:
        util.jpeg_encode(torch.zeros(1, 3, 16, 16, device='cuda'), quality=0)
    assert err.value.code == -1
    with pytest.raises(ValueError):
        util.jpeg_encode(torch.zeros(1, 1, 16, 16, device='cuda'))


FRAMES, BATCH = 4, 2


@pytest.fixture(scope="module")
def imitated():
    """the synthetic 256 x 256 setup of run_imitator.py --synthetic, personalised; its target SMPLs and the float frames of
    `inference_by_smpls` without the flag (batches of 2)"""
    imitator, src_smpl, src_img, bg_img = demo.build_synthetic_imitator(batch_size=BATCH, opt=demo.default_opt(batch_size=BATCH))
    imitator.personalize(src_img, src_smpl=src_smpl, bg_img=bg_img)
    smpls = demo.synthetic_smpls(FRAMES, seed=0)
    frames = imitator.inference_by_smpls(smpls, cam_strategy="smooth")
    assert len(frames) == FRAMES and frames[0].shape == (256, 256, 3)
    return imitator, smpls, frames


def test_inference_by_smpls_writes_device_jpegs(imitated, tmp_path):
    """4 frames in batches of 2: the pred_%08d.jpg files hold the restatement's bytes for the frames the same call returns
    without the flag; without the flag the files are what they were (PIL's encoding of the same uint8 frames)."""
    imitator, smpls, frames = imitated
    host_dir, dev_dir = str(tmp_path / "host"), str(tmp_path / "dev")
    os.makedirs(host_dir)
    os.makedirs(dev_dir)
    again = imitator.inference_by_smpls(smpls, cam_strategy="smooth", output_dir=host_dir)
    assert all(np.array_equal(a, b) for a, b in zip(again, frames))
    paths = imitator.inference_by_smpls(smpls, cam_strategy="smooth", output_dir=dev_dir, device_jpeg=True)
    assert paths == [os.path.join(dev_dir, 'pred_%.8d.jpg' % t) for t in range(FRAMES)]
    assert sorted(os.listdir(dev_dir)) == sorted(os.listdir(host_dir)) == ['pred_%.8d.jpg' % t for t in range(FRAMES)]
    for t, path in enumerate(paths):
        data = open(path, 'rb').read()
        want, _ = jpeg_ref.encode(jpeg_ref.to_u8(frames[t]), 75, '4:2:0')
        assert data == want, (t, first_difference(data, want))
        if features.check_feature('libjpeg_turbo'):
            # the host writer's file (PIL at its defaults: quality 75, 4:2:0) holds the same bytes
            assert data == open(os.path.join(host_dir, 'pred_%.8d.jpg' % t), 'rb').read()
    other = imitator.inference_by_smpls(smpls[:2], output_dir=dev_dir, device_jpeg=True, jpeg_quality=95, jpeg_subsampling='4:4:4')
    assert open(other[1], 'rb').read() == jpeg_ref.encode(jpeg_ref.to_u8(frames[1]), 95, '4:4:4')[0]
    # the flag without an output_dir changes nothing
    same = imitator.inference_by_smpls(smpls[:2], device_jpeg=True)
    assert np.array_equal(same[1], frames[1])
    # named after the target files, a foreign extension replaced
    named = imitator.inference(['a/first.png', 'b/second.jpg'], tgt_smpls=smpls[:2], output_dir=dev_dir, device_jpeg=True)
    assert named == [os.path.join(dev_dir, 'pred_first.jpg'), os.path.join(dev_dir, 'pred_second.jpg')]
    assert open(named[1], 'rb').read() == jpeg_ref.encode(jpeg_ref.to_u8(frames[1]), 75, '4:2:0')[0]


def test_run_imitator_device_jpeg_and_save_video(imitated, tmp_path):
    """the command line: run_imitator.py --synthetic --device_jpeg writes pred_%08d.jpg with the bytes of the restatement on this
    process's frames of the same model, and --save_video stores exactly those streams in an AVI"""
    import struct
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _, _, frames = imitated
    out_dir, avi = str(tmp_path / "out"), str(tmp_path / "out.avi")
    p = subprocess.run([sys.executable, "run_imitator.py", "--synthetic", "--device_jpeg", "--jpeg_quality", "90", "--num_frames",
                        str(FRAMES), "--batch_size", str(BATCH), "--output_dir", out_dir, "--save_video", avi, "--fps", "10"],
                       cwd=root, env=dict(os.environ, PYTHONPATH=root), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       text=True)
    assert p.returncode == 0, "%s\n%s" % (p.stdout[-2000:], p.stderr[-4000:])
    assert "wrote %d frames to %s" % (FRAMES, out_dir) in p.stdout
    assert sorted(os.listdir(out_dir)) == ['pred_%.8d.jpg' % t for t in range(FRAMES)]
    data = open(avi, 'rb').read()
    at = data.index(b'movi') + 4
    for t in range(FRAMES):
        stream = open(os.path.join(out_dir, 'pred_%.8d.jpg' % t), 'rb').read()
        want, _ = jpeg_ref.encode(jpeg_ref.to_u8(frames[t]), 90, '4:2:0')
        assert stream == want, (t, first_difference(stream, want))
        assert Image.open(io.BytesIO(stream)).size == (256, 256)
        assert data[at:at + 4] == b'00dc' and struct.unpack('<I', data[at + 4:at + 8])[0] == len(stream)
        assert data[at + 8:at + 8 + len(stream)] == stream
        at += 8 + len(stream) + (len(stream) & 1)
    assert data[at:at + 4] == b'idx1'


def test_animate_writes_device_jpegs(tmp_path):
    """Animator.animate under the flag (as run_animate.py --synthetic --device_jpeg --save_res calls it): the files hold the
    restatement's bytes for the frames the same call returns without the flag"""
    from impersonator_amd.utils import synthetic
    size = 128
    an, smpl_a, img_a, bg_a = demo.build_synthetic_imitator(batch_size=2, image_size=size, model="animator",
                                                             opt=demo.default_opt(batch_size=2, image_size=size))
    an.animate_setup(img_a, synthetic.smooth_image(77, (1, 3, size, size))[0], src_smpl=smpl_a,
                     ref_smpl=demo.synthetic_smpls(8, seed=3)[5], src_bg=bg_a, ref_bg=bg_a)
    smpls = demo.synthetic_smpls(3, seed=0)
    frames = an.animate(None, tgt_smpls=smpls, target_part="upper_body")
    paths = an.animate(None, tgt_smpls=smpls, target_part="upper_body", output_dir=str(tmp_path), device_jpeg=True, jpeg_quality=60)
    assert paths == [os.path.join(str(tmp_path), 'pred_%.8d.jpg' % t) for t in range(3)]
    for t, path in enumerate(paths):
        data, (want, _) = open(path, 'rb').read(), jpeg_ref.encode(jpeg_ref.to_u8(frames[t]), 60, '4:2:0')
        assert data == want, (t, first_difference(data, want))


def test_run_mesh_device_jpeg(tmp_path, monkeypatch):
    """run_mesh.py --device_jpeg: the files hold the restatement's bytes for the pictures the renderer gives on the same seeded
    sequence, as [-1,1] images (mesh_* and masked_*; wt_* must open at the right size)"""
    import run_mesh
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))   # parse() exports --gpu_ids: undone after
    args = ["--synthetic", "--num_frames", "2", "--batch_size", "2", "--image_size", "64", "--texture_warp", "--device_jpeg",
            "--jpeg_quality", "90", "--jpeg_subsampling", "444", "--output_dir", str(tmp_path)]
    run_mesh.main(args)
    folder = str(tmp_path / "meshes")
    assert sorted(os.listdir(folder)) == sorted("%s_%08d.jpg" % (kind, t) for kind in ("mesh", "masked", "wt") for t in range(2))
    opt = run_mesh.MeshOptions().parse(args)
    render, verts, cams, frames = run_mesh.synthetic_sequence(opt)
    render.set_ambient_light()
    render.set_bgcolor((0, 0, 0))
    mesh, _ = render.render(cams, verts, render.debug_textures().cuda())
    masked = frames * render.render_silhouettes(cams, verts)[:, None]
    for kind, batch in (("mesh", mesh), ("masked", masked)):
        u8 = jpeg_ref.to_u8((batch.clamp(0, 1) * 2 - 1).cpu().numpy()).transpose(0, 2, 3, 1)
        assert u8.max() > 100
        for t in range(2):
            data, (want, _) = open(os.path.join(folder, "%s_%08d.jpg" % (kind, t)), 'rb').read(), jpeg_ref.encode(
                np.ascontiguousarray(u8[t]), 90, '4:4:4')
            assert data == want, (kind, t, first_difference(data, want))
    for t in range(2):
        img = Image.open(os.path.join(folder, "wt_%08d.jpg" % t))
        assert img.size == (64, 64) and img.mode == 'RGB'
        img.load()
