"""Integer restatement in numpy of the baseline JFIF encoder of impersonator_amd/csrc/jpeg.hip (the algorithm is stated in
that file's header comment): uint8 RGB -> the bytes of a .jpg file.  Everything is int64 arithmetic on small integers, so
the result is exact; tests/test_jpeg_host.py checks that it equals libjpeg-turbo's output (PIL, optimize=False) byte for
byte, and tests/test_gpu_jpeg.py that the device encoder equals it.

    encode(u8_hwc, quality=75, subsampling='4:2:0') -> (bytes, counters)
    to_u8(x)                                          the float32 -> uint8 rule of cv_utils.save_cv2_img(normalize=True)
"""
import numpy as np

# ITU-T T.81 Annex K.1, natural (row-major) order
LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64)

# ZIGZAG[k]: natural index of the k-th coefficient in zigzag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)

# ITU-T T.81 Annex K.3: (BITS, HUFFVAL) of the four typical tables
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
HUFFMAN = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)     # the order of the DHT segments
HEADER_BYTES = 623
MAX_BLOCK_BITS = 20 + 63 * 26

COUNTERS = ('zrl', 'no_eob', 'dc_cat11', 'ac_cat10', 'stuffed')


def to_u8(x):
    """cv_utils.save_cv2_img(normalize=True) on float32, each operation rounded separately; clamped, NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        v = ((x + np.float32(1)) / np.float32(2)) * np.float32(255)
        v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(255)))
    return v.astype(np.uint8)


def stream_bytes(H, W, subsampling='4:2:0'):
    """capacity of one frame's stream: header + the worst-case scan with every byte stuffed + EOI"""
    nblocks = (H // 8) * (W // 8) * 3 if _sub(subsampling) == 444 else (H // 16) * (W // 16) * 6
    return HEADER_BYTES + 2 * ((nblocks * MAX_BLOCK_BITS + 7) // 8) + 2


def _sub(subsampling):
    s = {'4:2:0': 420, '4:4:4': 444, 420: 420, 444: 444, 2: 420, 0: 444}.get(subsampling)
    if s is None:
        raise ValueError("subsampling %r" % (subsampling,))
    return s


def quant_table(base, quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def huffman_codes(bits, vals):
    """symbol -> (code, length), Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def ycbcr(u8):
    r, g, b = (u8[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def subsample_420(p):
    H, W = p.shape
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(W // 2) & 1)            # 1, 2, 1, 2, ... along the output row
    return (s + bias[None, :]) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """one pass of the 13-bit integer DCT along the last axis of d (..., 8)"""
    F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
             f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 11 if first else 15
    if first:
        out[..., 0] = (t10 + t11) << 2
        out[..., 4] = (t10 - t11) << 2
    else:
        out[..., 0] = _descale(t10 + t11, 2)
        out[..., 4] = _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F['f0_541']
    out[..., 2] = _descale(z1 + t13 * F['f0_765'], n)
    out[..., 6] = _descale(z1 - t12 * F['f1_847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F['f1_175']
    t4, t5, t6, t7 = t4 * F['f0_298'], t5 * F['f2_053'], t6 * F['f3_072'], t7 * F['f1_501']
    z1, z2, z3, z4 = -z1 * F['f0_899'], -z2 * F['f2_562'], -z3 * F['f1_961'], -z4 * F['f0_390']
    z3, z4 = z3 + z5, z4 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def blocks_of(plane, qt):
    """(H,W) samples 0..255 -> (H/8, W/8, 64) quantised coefficients in zigzag order"""
    H, W = plane.shape
    b = (plane - 128).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)         # (by, bx, row, col)
    b = _dct_pass(b, True)                                                          # rows
    b = _dct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)             # columns
    b = b.reshape(H // 8, W // 8, 64)
    qv = 8 * qt
    q = np.sign(b) * ((np.abs(b) + (qv >> 1)) // qv)
    return q[..., ZIGZAG]


class _Bits(object):
    def __init__(self):
        self.acc, self.n, self.out, self.stuffed = 0, 0, bytearray(), 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _encode_block(w, zz, pred, dc, ac, cnt):
    diff = int(zz[0]) - pred
    size = abs(diff).bit_length()
    cnt['dc_cat11'] += size == 11
    w.put(*dc[size])
    if size:
        w.put(diff if diff >= 0 else diff - 1, size)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            cnt['zrl'] += 1
            run -= 16
        size = abs(v).bit_length()
        cnt['ac_cat10'] += size == 10
        w.put(*ac[(run << 4) | size])
        w.put(v if v >= 0 else v - 1, size)
        run = 0
    if run:
        w.put(*ac[0x00])
    else:
        cnt['no_eob'] += 1
    return int(zz[0])


def header(H, W, quality, sub):
    out = bytearray(b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for i, base in enumerate((LUMA_Q, CHROMA_Q)):
        out += b'\xff\xdb\x00\x43' + bytes([i]) + bytes(quant_table(base, quality)[ZIGZAG].tolist())
    out += b'\xff\xc0\x00\x11\x08' + bytes([H >> 8, H & 255, W >> 8, W & 255, 3,
                                            1, 0x22 if sub == 420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), HUFFMAN):
        out += b'\xff\xc4' + bytes([0, 19 + len(vals), tc_th]) + bytes(bits) + bytes(vals)
    out += b'\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'
    assert len(out) == HEADER_BYTES
    return bytes(out)


def encode(u8_hwc, quality=75, subsampling='4:2:0'):
    """-> (the .jpg file's bytes, counters): counters of the entropy coder's branches, keys COUNTERS"""
    u8 = np.asarray(u8_hwc)
    assert u8.dtype == np.uint8 and u8.ndim == 3 and u8.shape[2] == 3
    H, W = u8.shape[:2]
    assert H % 16 == 0 and W % 16 == 0 and 1 <= quality <= 100
    sub = _sub(subsampling)
    y, cb, cr = ycbcr(u8)
    if sub == 420:
        cb, cr = subsample_420(cb), subsample_420(cr)
    ql, qc = quant_table(LUMA_Q, quality), quant_table(CHROMA_Q, quality)
    Y, Cb, Cr = blocks_of(y, ql), blocks_of(cb, qc), blocks_of(cr, qc)
    dcl, acl, dcc, acc = (huffman_codes(*t) for t in HUFFMAN)
    cnt = dict.fromkeys(COUNTERS, 0)
    w = _Bits()
    pred = [0, 0, 0]
    if sub == 420:
        for my in range(H // 16):
            for mx in range(W // 16):
                for j in range(2):
                    for i in range(2):
                        pred[0] = _encode_block(w, Y[2 * my + j, 2 * mx + i], pred[0], dcl, acl, cnt)
                pred[1] = _encode_block(w, Cb[my, mx], pred[1], dcc, acc, cnt)
                pred[2] = _encode_block(w, Cr[my, mx], pred[2], dcc, acc, cnt)
    else:
        for by in range(H // 8):
            for bx in range(W // 8):
                pred[0] = _encode_block(w, Y[by, bx], pred[0], dcl, acl, cnt)
                pred[1] = _encode_block(w, Cb[by, bx], pred[1], dcc, acc, cnt)
                pred[2] = _encode_block(w, Cr[by, bx], pred[2], dcc, acc, cnt)
    w.flush()
    cnt['stuffed'] = w.stuffed
    cnt = {k: int(v) for k, v in cnt.items()}
    return header(H, W, quality, sub) + bytes(w.out) + b'\xff\xd9', cnt


# ---------------------------------------------------------------------------------------------- test images
PATTERNS = ('noise', 'binary', 'smooth', 'tiles', 'checker', 'specks')


def pattern(name, n, H, W, seed=7):
    """(n,3,H,W) float32 in [-1,1], different content per frame and channel"""
    rng = np.random.RandomState(seed + 1000 * PATTERNS.index(name))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    shape = (n, 3, H, W)

    def sinus(amp):
        f = rng.uniform(0.02, 0.25, size=(n, 3, 2, 1, 1))
        ph = rng.uniform(0, 2 * np.pi, size=(n, 3, 1, 1))
        return amp * np.sin(f[:, :, 0] * yy + f[:, :, 1] * xx + ph)

    if name == 'noise':
        x = rng.uniform(-1, 1, size=shape)
    elif name == 'binary':
        x = rng.randint(0, 2, size=shape) * 2.0 - 1.0
    elif name == 'smooth':
        x = sinus(0.9)
    elif name == 'tiles':
        t = ((yy // 16 + xx // 16) % 2) * 2.0 - 1.0
        sign = rng.randint(0, 2, size=(n, 3, 1, 1)) * 2.0 - 1.0
        x = t[None, None] * sign
    elif name == 'checker':
        t = ((yy + xx) % 2) * 2.0 - 1.0
        sign = rng.randint(0, 2, size=(n, 3, 1, 1)) * 2.0 - 1.0
        x = t[None, None] * sign
    elif name == 'specks':
        x = sinus(0.5) + 0.5 * (rng.uniform(size=shape) < 0.03)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x, dtype=np.float32)


# the device test's cases: (N, H, W) x quality x subsampling x pattern
GPU_SHAPES = ((1, 16, 16), (1, 32, 48), (3, 64, 64))
GPU_QUALITIES = (30, 75, 100)
SUBSAMPLINGS = ('4:2:0', '4:4:4')


def encode_batch(x, quality, subsampling):
    """x (n,3,H,W) float -> ([bytes per frame], summed counters)"""
    u8 = to_u8(x).transpose(0, 2, 3, 1)
    total = dict.fromkeys(COUNTERS, 0)
    streams = []
    for frame in u8:
        data, cnt = encode(np.ascontiguousarray(frame), quality, subsampling)
        streams.append(data)
        for k in COUNTERS:
            total[k] += cnt[k]
    return streams, total
