"""A sequence of JPEG streams as one Motion-JPEG .avi file, written in pure Python (the reference's demo_imitator.py shells out
to ffmpeg for its videos).  The frames are stored as they are -- e.g. the streams of util.jpeg_bytes -- nothing is re-encoded.

RIFF layout: RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh', 'strf' } }, LIST 'movi' { '00dc' per frame }, 'idx1' }.
Chunks are padded to even sizes; 'idx1' offsets count from the 'movi' fourcc, as AVI 1.0 readers expect."""
import struct


def _chunk(fourcc, data):
    return fourcc + struct.pack('<I', len(data)) + data + (b'\0' if len(data) & 1 else b'')


def _list(kind, data):
    return b'LIST' + struct.pack('<I', 4 + len(data)) + kind + data


def write_mjpeg_avi(path, streams, fps, size):
    """streams: the frames' JPEG files as bytes, all of `size` = (width, height); fps: frames per second.  Returns the file size.
    One RIFF chunk, so the file must stay below 4 GiB (about 300 000 frames of 256 x 256 at quality 75)."""
    streams = [bytes(s) for s in streams]
    width, height = int(size[0]), int(size[1])
    if not streams:
        raise ValueError("write_mjpeg_avi: no frames")
    if fps <= 0 or width <= 0 or height <= 0:
        raise ValueError("write_mjpeg_avi: fps and size must be positive")
    for k, s in enumerate(streams):
        if s[:2] != b'\xff\xd8':
            raise ValueError("write_mjpeg_avi: frame %d is not a JPEG stream" % k)
    scale = 1000
    rate = max(1, int(round(fps * scale)))
    largest = max(len(s) for s in streams)
    n = len(streams)
    avih = struct.pack('<14I', int(round(1e6 * scale / rate)), int(largest * rate / scale) + 1, 0, 0x10, n, 0, 1, largest, width, height,
                       0, 0, 0, 0)
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIII4H', 0, 0, 0, 0, scale, rate, 0, n, largest, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack('<IiiHH4sIiiII', 40, width, height, 1, 24, b'MJPG', width * height * 3, 0, 0, 0, 0)
    hdrl = _list(b'hdrl', _chunk(b'avih', avih) + _list(b'strl', _chunk(b'strh', strh) + _chunk(b'strf', strf)))
    movi, index, at = [], [], 4                      # `at`: offset of the next chunk from the 'movi' fourcc
    for s in streams:
        c = _chunk(b'00dc', s)
        index.append(b'00dc' + struct.pack('<III', 0x10, at, len(s)))      # AVIIF_KEYFRAME: every frame stands alone
        movi.append(c)
        at += len(c)
    body = b'AVI ' + hdrl + _list(b'movi', b''.join(movi)) + _chunk(b'idx1', b''.join(index))
    if len(body) >= 1 << 32:
        raise ValueError("write_mjpeg_avi: %d bytes do not fit one RIFF chunk" % len(body))
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', len(body)) + body)
    return 8 + len(body)
