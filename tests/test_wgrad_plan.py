"""What launch_wgrad (csrc/train.hip) launches, pinned without a device: lwg_wgrad_plan returns the dispatcher's pure plan --
route, kernel-table row, grid, block, LDS bytes, pixel slices S, pixels per slice, reduction -- and every field is compared
with a literal.  S fixes the order in which a weight gradient is summed, i.e. its bits, for the generator and the
discriminator alike; the float64 comparisons of the GPU suite do not see it move.

The literals were recorded from the arithmetic of the dispatcher as it stood before it became a plan (commit f8411fc): its
launch_wgrad, the descriptor mapping of lwg_conv2d_backward_weight and the buffer sizing of lwg_discriminator_create were
copied into a stand-alone host program, the launches replaced by prints and the CU count made an argument, and that program was
run over CASES and the switch cases below.  The only case it answers differently is precision 2, which it ran as fp32."""
import ctypes
import os
import subprocess
import sys

import pytest

from impersonator_amd import _lib
from impersonator_amd.ops import _Desc

ROW3, STEM, PER_TAP = 0, 1, 2                                                       # route
TAP_F32_64, TAP_F32_128, TAP_X3_64, TAP_X3_128, ROW3_64_64, ROW3_64_128, ROW3_128_64, ROW3_128_128, STEM7 = range(9)   # table row
NONE, SLICES4, TAPS_DIRECT, TAPS = range(4)                                         # reduction
INVALID, UNSUPPORTED = -1, -2

# part_floats of lwg_discriminator_create(input_nc 6, ndf 64, n_layers 3, image 256, max_batch 4): the largest layer's
# min(32, ceil(512 / tiles)) filters = 16 x 256*16*128 floats; its backward runs 2 x max_batch = 8 images
D_PART = 8388608

# name -> ((N, H, W, Cin, Cout, k, stride, pad, transposed, precision), part_floats); 0: lwg_conv2d_backward_weight's own
CASES = {}
for _n in (4, 1):   # the 3x3 row route, the four tiles: the layer shapes of tools/wgrad_bench.py at 256 x 256
    CASES.update({
        "row 512->512 @32 n%d" % _n: ((_n, 32, 32, 512, 512, 3, 1, 1, 0, 1), 0),
        "row 512->256 @64 n%d" % _n: ((_n, 64, 64, 512, 256, 3, 1, 1, 0, 1), 0),
        "row 256->128 @128 n%d" % _n: ((_n, 128, 128, 256, 128, 3, 1, 1, 0, 1), 0),
        "row 128->64 @256 n%d" % _n: ((_n, 256, 256, 128, 64, 3, 1, 1, 0, 1), 0),
        "row 64->64 @256 n%d" % _n: ((_n, 256, 256, 64, 64, 3, 1, 1, 0, 1), 0),
        "row 64->128 @64 n%d" % _n: ((_n, 64, 64, 64, 128, 3, 1, 1, 0, 1), 0),
    })
CASES.update({
    # what the row route does not take falls through to the per-tap kernels
    "fall W=24": ((4, 24, 24, 64, 64, 3, 1, 1, 0, 1), 0),
    "fall stride 2": ((4, 64, 64, 64, 64, 3, 2, 1, 0, 1), 0),
    "fall fp32": ((4, 64, 64, 64, 64, 3, 1, 1, 0, 0), 0),
    "fall Hin != Hg": ((4, 34, 34, 64, 64, 3, 1, 0, 0, 1), 0),     # 32 x 32 out of 34 x 34 (no padding: the only way to it)
    # the 7x7 stem
    "stem @256 n4": ((4, 256, 256, 8, 64, 7, 1, 3, 0, 1), 0),
    "stem @32 n1": ((1, 32, 32, 8, 64, 7, 1, 3, 0, 1), 0),         # "no fewer than 8 steps per slice" decides
    "stem fp32": ((4, 256, 256, 8, 64, 7, 1, 3, 0, 0), 0),
    "I=8 k=3": ((4, 64, 64, 8, 64, 3, 1, 1, 0, 1), 0),
    # per tap
    "tap 128->256 s2": ((4, 64, 64, 128, 256, 3, 2, 1, 0, 1), 0),
    "tap 128->256 s2 fp32": ((4, 64, 64, 128, 256, 3, 2, 1, 0, 0), 0),
    "tap 64->128 s2": ((4, 128, 128, 64, 128, 3, 2, 1, 0, 1), 0),
    "tap 64->128 s2 fp32": ((4, 128, 128, 64, 128, 3, 2, 1, 0, 0), 0),
    "tap 256->512 s2 @64": ((4, 64, 64, 256, 512, 3, 2, 1, 0, 1), 0),   # encoder.3 of tools/wgrad_bench.py
    "tap 256->512 s2 @64 n1": ((1, 64, 64, 256, 512, 3, 2, 1, 0, 1), 0),
    "tap 1x1": ((4, 32, 32, 256, 256, 1, 1, 0, 0, 1), 0),
    "tap 1x1 fp32": ((4, 32, 32, 256, 256, 1, 1, 0, 0, 0), 0),
    "tap transposed 128->64": ((4, 64, 64, 128, 64, 3, 2, 1, 1, 1), 0),     # roles swapped: O = 128, I = 64, 128 x 128 in
    "tap transposed 128->64 fp32": ((4, 64, 64, 128, 64, 3, 2, 1, 1, 0), 0),
    "tap transposed 256->128": ((4, 32, 32, 256, 128, 3, 2, 1, 1, 1), 0),   # the 128-wide tile
}
)
for _p in (0, 1):   # the discriminator's five layers (k 4, pad 1; the first on 8 padded channels, the last on 64)
    CASES.update({
        "D 8->64 s2 p%d" % _p: ((8, 256, 256, 8, 64, 4, 2, 1, 0, _p), D_PART),
        "D 64->128 s2 p%d" % _p: ((8, 128, 128, 64, 128, 4, 2, 1, 0, _p), D_PART),
        "D 128->256 s2 p%d" % _p: ((8, 64, 64, 128, 256, 4, 2, 1, 0, _p), D_PART),
        "D 256->512 s1 p%d" % _p: ((8, 32, 32, 256, 512, 4, 1, 1, 0, _p), D_PART),
        "D 512->64 s1 p%d" % _p: ((8, 31, 31, 512, 64, 4, 1, 1, 0, _p), D_PART),
    })
CASES.update({
    # caps: what the partial buffer holds, then the pixels
    "cap one filter row": ((4, 256, 256, 64, 64, 3, 1, 1, 0, 1), 64 * 64 * 9),          # S = 1: straight to the result
    "cap one filter tap": ((4, 128, 128, 64, 128, 3, 2, 1, 0, 1), 64 * 128 * 9),
    "cap one filter stem": ((4, 256, 256, 8, 64, 7, 1, 3, 0, 1), 8 * 64 * 49),
    "cap less than a filter": ((4, 128, 128, 64, 128, 3, 2, 1, 0, 0), 1000),
    "cap three filters row": ((4, 256, 256, 64, 64, 3, 1, 1, 0, 1), 3 * 64 * 64 * 9),
    "cap three filters tap": ((4, 128, 128, 64, 128, 3, 2, 1, 0, 1), 3 * 64 * 128 * 9 + 5),
    "cap three filters stem": ((4, 256, 256, 8, 64, 7, 1, 3, 0, 1), 3 * 8 * 64 * 49),
    "cap pixels row": ((1, 2, 32, 64, 64, 3, 1, 1, 0, 1), 0),        # 64 pixels: two steps
    "cap pixels tap": ((1, 8, 12, 64, 64, 3, 1, 1, 0, 1), 0),        # 96 pixels: three steps
    "cap pixels tap ragged": ((1, 10, 10, 64, 64, 3, 1, 1, 0, 0), 0),   # 100 pixels: four steps, the last of 4 pixels
    "cap pixels one step": ((1, 4, 4, 64, 64, 3, 1, 1, 0, 1), 0),
})

# (case, CU count) -> (route, table row, grid x, y, z, block, LDS bytes, S, pixels per slice, reduction)
EXPECTED = {
    ('row 512->512 @32 n4', 256): (0, 7, 240, 1, 1, 512, 131072, 5, 832, 3),
    ('row 512->512 @32 n4', 304): (0, 7, 288, 1, 1, 512, 131072, 6, 704, 3),
    ('row 512->256 @64 n4', 256): (0, 7, 240, 1, 1, 512, 131072, 10, 1664, 3),
    ('row 512->256 @64 n4', 304): (0, 7, 288, 1, 1, 512, 131072, 12, 1376, 3),
    ('row 256->128 @128 n4', 256): (0, 7, 192, 1, 1, 512, 131072, 32, 2048, 2),
    ('row 256->128 @128 n4', 304): (0, 7, 192, 1, 1, 512, 131072, 32, 2048, 2),
    ('row 128->64 @256 n4', 256): (0, 5, 256, 1, 1, 512, 114688, 85, 3104, 2),
    ('row 128->64 @256 n4', 304): (0, 5, 304, 1, 1, 512, 114688, 100, 2624, 2),
    ('row 64->64 @256 n4', 256): (0, 4, 504, 1, 1, 256, 65536, 168, 1568, 2),
    ('row 64->64 @256 n4', 304): (0, 4, 600, 1, 1, 256, 65536, 200, 1312, 2),
    ('row 64->128 @64 n4', 256): (0, 6, 224, 1, 1, 256, 81920, 74, 224, 2),
    ('row 64->128 @64 n4', 304): (0, 6, 224, 1, 1, 256, 81920, 74, 224, 2),
    ('row 512->512 @32 n1', 256): (0, 7, 192, 1, 1, 512, 131072, 4, 256, 3),
    ('row 512->512 @32 n1', 304): (0, 7, 192, 1, 1, 512, 131072, 4, 256, 3),
    ('row 512->256 @64 n1', 256): (0, 7, 240, 1, 1, 512, 131072, 10, 416, 3),
    ('row 512->256 @64 n1', 304): (0, 7, 288, 1, 1, 512, 131072, 12, 352, 3),
    ('row 256->128 @128 n1', 256): (0, 7, 192, 1, 1, 512, 131072, 32, 512, 2),
    ('row 256->128 @128 n1', 304): (0, 7, 192, 1, 1, 512, 131072, 32, 512, 2),
    ('row 128->64 @256 n1', 256): (0, 5, 248, 1, 1, 512, 114688, 82, 800, 2),
    ('row 128->64 @256 n1', 304): (0, 5, 296, 1, 1, 512, 114688, 98, 672, 2),
    ('row 64->64 @256 n1', 256): (0, 4, 480, 1, 1, 256, 65536, 158, 416, 2),
    ('row 64->64 @256 n1', 304): (0, 4, 568, 1, 1, 256, 65536, 187, 352, 2),
    ('row 64->128 @64 n1', 256): (0, 6, 96, 1, 1, 256, 81920, 32, 128, 2),
    ('row 64->128 @64 n1', 304): (0, 6, 96, 1, 1, 256, 81920, 32, 128, 2),
    ('fall W=24', 256): (2, 2, 1, 1, 135, 256, 32768, 15, 160, 1),
    ('fall W=24', 304): (2, 2, 1, 1, 135, 256, 32768, 15, 160, 1),
    ('fall stride 2', 256): (2, 2, 1, 1, 198, 256, 32768, 22, 192, 1),
    ('fall stride 2', 304): (2, 2, 1, 1, 198, 256, 32768, 22, 192, 1),
    ('fall fp32', 256): (2, 0, 1, 1, 423, 256, 34816, 47, 352, 1),
    ('fall fp32', 304): (2, 0, 1, 1, 423, 256, 34816, 47, 352, 1),
    ('fall Hin != Hg', 256): (2, 2, 1, 1, 198, 256, 32768, 22, 192, 1),
    ('fall Hin != Hg', 304): (2, 2, 1, 1, 198, 256, 32768, 22, 192, 1),
    ('stem @256 n4', 256): (1, 8, 1032, 1, 1, 256, 32768, 147, 1792, 2),
    ('stem @256 n4', 304): (1, 8, 1200, 1, 1, 256, 32768, 171, 1536, 2),
    ('stem @32 n1', 256): (1, 8, 32, 1, 1, 256, 32768, 4, 256, 2),
    ('stem @32 n1', 304): (1, 8, 32, 1, 1, 256, 32768, 4, 256, 2),
    ('stem fp32', 256): (2, 0, 1, 1, 2009, 256, 34816, 41, 6400, 1),
    ('stem fp32', 304): (2, 0, 1, 1, 2401, 256, 34816, 49, 5376, 1),
    ('I=8 k=3', 256): (2, 2, 1, 1, 423, 256, 32768, 47, 352, 1),
    ('I=8 k=3', 304): (2, 2, 1, 1, 423, 256, 32768, 47, 352, 1),
    ('tap 128->256 s2', 256): (2, 3, 1, 2, 198, 256, 65536, 22, 192, 1),
    ('tap 128->256 s2', 304): (2, 3, 1, 2, 198, 256, 65536, 22, 192, 1),
    ('tap 128->256 s2 fp32', 256): (2, 1, 1, 2, 198, 256, 67584, 22, 192, 1),
    ('tap 128->256 s2 fp32', 304): (2, 1, 1, 2, 198, 256, 67584, 22, 192, 1),
    ('tap 64->128 s2', 256): (2, 2, 1, 2, 423, 256, 32768, 47, 352, 1),
    ('tap 64->128 s2', 304): (2, 2, 1, 2, 423, 256, 32768, 47, 352, 1),
    ('tap 64->128 s2 fp32', 256): (2, 0, 1, 2, 423, 256, 34816, 47, 352, 1),
    ('tap 64->128 s2 fp32', 304): (2, 0, 1, 2, 423, 256, 34816, 47, 352, 1),
    ('tap 256->512 s2 @64', 256): (2, 3, 2, 4, 63, 256, 65536, 7, 608, 1),
    ('tap 256->512 s2 @64', 304): (2, 3, 2, 4, 72, 256, 65536, 8, 512, 1),
    ('tap 256->512 s2 @64 n1', 256): (2, 3, 2, 4, 63, 256, 65536, 7, 160, 1),
    ('tap 256->512 s2 @64 n1', 304): (2, 3, 2, 4, 63, 256, 65536, 7, 160, 1),
    ('tap 1x1', 256): (2, 3, 2, 2, 22, 256, 65536, 22, 192, 1),
    ('tap 1x1', 304): (2, 3, 2, 2, 22, 256, 65536, 22, 192, 1),
    ('tap 1x1 fp32', 256): (2, 1, 2, 2, 22, 256, 67584, 22, 192, 1),
    ('tap 1x1 fp32', 304): (2, 1, 2, 2, 22, 256, 67584, 22, 192, 1),
    ('tap transposed 128->64', 256): (2, 2, 1, 2, 423, 256, 32768, 47, 352, 1),
    ('tap transposed 128->64', 304): (2, 2, 1, 2, 423, 256, 32768, 47, 352, 1),
    ('tap transposed 128->64 fp32', 256): (2, 0, 1, 2, 423, 256, 34816, 47, 352, 1),
    ('tap transposed 128->64 fp32', 304): (2, 0, 1, 2, 423, 256, 34816, 47, 352, 1),
    ('tap transposed 256->128', 256): (2, 3, 1, 2, 198, 256, 65536, 22, 192, 1),
    ('tap transposed 256->128', 304): (2, 3, 1, 2, 198, 256, 65536, 22, 192, 1),
    ('D 8->64 s2 p0', 256): (2, 0, 1, 1, 1024, 256, 34816, 64, 2048, 1),
    ('D 8->64 s2 p0', 304): (2, 0, 1, 1, 1216, 256, 34816, 76, 1728, 1),
    ('D 64->128 s2 p0', 256): (2, 0, 1, 2, 512, 256, 34816, 32, 1024, 1),
    ('D 64->128 s2 p0', 304): (2, 0, 1, 2, 608, 256, 34816, 38, 864, 1),
    ('D 128->256 s2 p0', 256): (2, 1, 1, 2, 256, 256, 67584, 16, 512, 1),
    ('D 128->256 s2 p0', 304): (2, 1, 1, 2, 256, 256, 67584, 16, 512, 1),
    ('D 256->512 s1 p0', 256): (2, 1, 2, 4, 64, 256, 67584, 4, 1952, 1),
    ('D 256->512 s1 p0', 304): (2, 1, 2, 4, 64, 256, 67584, 4, 1952, 1),
    ('D 512->64 s1 p0', 256): (2, 0, 8, 1, 128, 256, 34816, 8, 928, 1),
    ('D 512->64 s1 p0', 304): (2, 0, 8, 1, 144, 256, 34816, 9, 800, 1),
    ('D 8->64 s2 p1', 256): (2, 2, 1, 1, 1024, 256, 32768, 64, 2048, 1),
    ('D 8->64 s2 p1', 304): (2, 2, 1, 1, 1216, 256, 32768, 76, 1728, 1),
    ('D 64->128 s2 p1', 256): (2, 2, 1, 2, 512, 256, 32768, 32, 1024, 1),
    ('D 64->128 s2 p1', 304): (2, 2, 1, 2, 608, 256, 32768, 38, 864, 1),
    ('D 128->256 s2 p1', 256): (2, 3, 1, 2, 256, 256, 65536, 16, 512, 1),
    ('D 128->256 s2 p1', 304): (2, 3, 1, 2, 256, 256, 65536, 16, 512, 1),
    ('D 256->512 s1 p1', 256): (2, 3, 2, 4, 64, 256, 65536, 4, 1952, 1),
    ('D 256->512 s1 p1', 304): (2, 3, 2, 4, 64, 256, 65536, 4, 1952, 1),
    ('D 512->64 s1 p1', 256): (2, 2, 8, 1, 128, 256, 32768, 8, 928, 1),
    ('D 512->64 s1 p1', 304): (2, 2, 8, 1, 144, 256, 32768, 9, 800, 1),
    ('cap one filter row', 256): (0, 4, 8, 1, 1, 256, 65536, 1, 262144, 0),
    ('cap one filter row', 304): (0, 4, 8, 1, 1, 256, 65536, 1, 262144, 0),
    ('cap one filter tap', 256): (2, 2, 1, 2, 9, 256, 32768, 1, 16384, 0),
    ('cap one filter tap', 304): (2, 2, 1, 2, 9, 256, 32768, 1, 16384, 0),
    ('cap one filter stem', 256): (1, 8, 8, 1, 1, 256, 32768, 1, 262144, 0),
    ('cap one filter stem', 304): (1, 8, 8, 1, 1, 256, 32768, 1, 262144, 0),
    ('cap less than a filter', 256): (2, 0, 1, 2, 9, 256, 34816, 1, 16384, 0),
    ('cap less than a filter', 304): (2, 0, 1, 2, 9, 256, 34816, 1, 16384, 0),
    ('cap three filters row', 256): (0, 4, 16, 1, 1, 256, 65536, 3, 87392, 2),
    ('cap three filters row', 304): (0, 4, 16, 1, 1, 256, 65536, 3, 87392, 2),
    ('cap three filters tap', 256): (2, 2, 1, 2, 27, 256, 32768, 3, 5472, 1),
    ('cap three filters tap', 304): (2, 2, 1, 2, 27, 256, 32768, 3, 5472, 1),
    ('cap three filters stem', 256): (1, 8, 24, 1, 1, 256, 32768, 3, 87392, 2),
    ('cap three filters stem', 304): (1, 8, 24, 1, 1, 256, 32768, 3, 87392, 2),
    ('cap pixels row', 256): (0, 4, 8, 1, 1, 256, 65536, 1, 64, 0),
    ('cap pixels row', 304): (0, 4, 8, 1, 1, 256, 65536, 1, 64, 0),
    ('cap pixels tap', 256): (2, 2, 1, 1, 27, 256, 32768, 3, 32, 1),
    ('cap pixels tap', 304): (2, 2, 1, 1, 27, 256, 32768, 3, 32, 1),
    ('cap pixels tap ragged', 256): (2, 0, 1, 1, 36, 256, 34816, 4, 32, 1),
    ('cap pixels tap ragged', 304): (2, 0, 1, 1, 36, 256, 34816, 4, 32, 1),
    ('cap pixels one step', 256): (2, 2, 1, 1, 9, 256, 32768, 1, 32, 0),
    ('cap pixels one step', 304): (2, 2, 1, 1, 9, 256, 32768, 1, 32, 0),
}

REFUSED = {
    "O = 32": ((1, 32, 32, 64, 32, 3, 1, 1, 0, 1), UNSUPPORTED, b"multiple of 64"),
    "O = 32 transposed": ((1, 32, 32, 32, 64, 3, 2, 1, 1, 1), UNSUPPORTED, b"multiple of 64"),
    "precision 2": ((1, 32, 32, 64, 64, 3, 1, 1, 0, 2), INVALID, b"precision"),
    "2^32 elements of x": ((4, 4096, 4096, 64, 64, 3, 1, 1, 0, 1), UNSUPPORTED, b"2^32"),
    "2^32 elements of dy": ((4, 4096, 4096, 8, 64, 3, 1, 1, 0, 1), UNSUPPORTED, b"2^32"),
}


def plan(desc, part_floats=0, ncu=256):
    """-> the ten fields as a tuple, or the negative error code"""
    info = (ctypes.c_longlong * 10)()
    d = _Desc(*desc)
    rc = _lib.load().lwg_wgrad_plan(ctypes.byref(d), part_floats, ncu, info)
    return tuple(info) if rc == 0 else rc


@pytest.mark.parametrize("ncu", [256, 304])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_is_the_recorded_one(case, ncu):
    desc, part_floats = CASES[case]
    got = plan(desc, part_floats, ncu)
    print("OBSERVED %s @%d: %r" % (case, ncu, got))
    assert got == EXPECTED[(case, ncu)]


def test_the_cases_reach_every_row_route_and_reduction():
    at = lambda i: {v[i] for v in EXPECTED.values()}
    assert at(0) == {ROW3, STEM, PER_TAP} and at(1) == set(range(9)) and at(9) == {NONE, SLICES4, TAPS_DIRECT, TAPS}
    assert any(a != b for (c, n), a in EXPECTED.items() if n == 256 for b in [EXPECTED[(c, 304)]]), "the CU count is an input"


def test_one_filter_of_partials_means_no_split_and_no_reduce():
    for case in ("cap one filter row", "cap one filter tap", "cap one filter stem", "cap less than a filter"):
        for ncu in (256, 304):
            assert EXPECTED[(case, ncu)][7] == 1 and EXPECTED[(case, ncu)][9] == NONE
    for case in ("cap three filters row", "cap three filters tap", "cap three filters stem"):
        assert 1 <= EXPECTED[(case, 256)][7] <= 3


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals(case):
    desc, code, text = REFUSED[case]
    assert plan(desc) == code
    assert text in _lib.load().lwg_last_error()


def test_fp32_has_no_element_limit():
    desc = list(REFUSED["2^32 elements of x"][0])
    desc[9] = 0
    assert isinstance(plan(tuple(desc)), tuple)


def test_null_arguments_and_cu_count():
    lib = _lib.load()
    info = (ctypes.c_longlong * 10)()
    d = _Desc(*CASES["stem @32 n1"][0])
    assert lib.lwg_wgrad_plan(None, 0, 256, info) == INVALID and b"NULL" in lib.lwg_last_error()
    assert lib.lwg_wgrad_plan(ctypes.byref(d), 0, 256, None) == INVALID and b"NULL" in lib.lwg_last_error()
    assert lib.lwg_wgrad_plan(ctypes.byref(d), 0, 0, info) == INVALID


# ---- the two switches (read once per process: one short child each).  (case, part_floats) -> plan at 256 CUs
_ROW, _STEM = "row 64->64 @256 n4", "stem @256 n4"
SWITCHED = {
    # the per-tap kernel everywhere
    "LWG_WGRAD_ROW3=0": {
        (_ROW, 0): (2, 2, 1, 1, 999, 256, 32768, 111, 2368, 1),
        (_STEM, 0): (2, 2, 1, 1, 2009, 256, 32768, 41, 6400, 1),
        ("row 512->512 @32 n4", 0): (2, 3, 4, 4, 63, 256, 65536, 7, 608, 1),
    },
    # forces S on the 3x3 row route where the cap allows it: not with two filters of partials, not on the other routes
    "LWG_WGRAD_ROW3_SLICES=3": {
        (_ROW, 0): (0, 4, 16, 1, 1, 256, 65536, 3, 87392, 2),
        (_ROW, 2 * 64 * 64 * 9): (0, 4, 8, 1, 1, 256, 65536, 2, 131072, 2),
        ("row 512->512 @32 n4", 0): (0, 7, 144, 1, 1, 512, 131072, 3, 1376, 3),
        (_STEM, 0): (1, 8, 1032, 1, 1, 256, 32768, 147, 1792, 2),
        ("tap 64->128 s2", 0): (2, 2, 1, 2, 423, 256, 32768, 47, 352, 1),
    },
}
_CHILD = ("from tests import test_wgrad_plan as t\n"
          "for case, part in t.SWITCHED[%r]:\n"
          "    print('PLAN', repr((case, part)), '=', repr(t.plan(t.CASES[case][0], part or t.CASES[case][1])))\n")


@pytest.mark.parametrize("switch", sorted(SWITCHED))
def test_switch(switch):
    var, val = switch.split("=")
    assert var not in os.environ, "this suite runs with the switches at their defaults"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _CHILD % switch], cwd=root, env=dict(os.environ, PYTHONPATH=root, **{var: val}),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = {}
    for line in p.stdout.splitlines():
        if line.startswith("PLAN "):
            key, value = line[5:].split(" = ")
            got[eval(key)] = eval(value)
    print("OBSERVED %s: %r" % (switch, got))
    assert got == SWITCHED[switch]
    # and the switch did something: the same cases plan otherwise without it
    assert any(plan(CASES[c][0], part or CASES[c][1]) != v for (c, part), v in SWITCHED[switch].items())
