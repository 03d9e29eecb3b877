// jpeg.hip -- baseline sequential JFIF encoder on the device: a batch of generator outputs -> finished .jpg streams (gfx950).
//
// Every driver that writes pictures copied each frame to the host as float32 (786 KB at 256 x 256), converted it in numpy and
// encoded it with PIL on one thread (utils/cv_utils.py: save_cv2_img).  Here the frames leave the device as the bytes of the file.
// The output is byte-identical to libjpeg(-turbo)'s baseline encoder with its default (not optimised) Huffman tables; the
// integer restatement in tests/jpeg_ref.py is the specification both are tested against.
//
// The algorithm (everything after step 1 is int32 arithmetic):
//   1. float -> uint8   u = trunc(((x + 1) / 2) * 255) in fp32, every operation rounded separately (save_cv2_img, normalize=True;
//                       the file is built without fp contraction), clamped to 0..255, NaN -> 0.  x is (N,3,H,W) NCHW in [-1,1].
//   2. RGB -> YCbCr     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//                       Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//                       Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
//   3. chroma           4:2:0: (sum of each 2 x 2 cell + bias) >> 2, bias 1, 2, 1, 2, ... along the output row from column 0;
//                       4:4:4: as it is.
//   4. level shift      - 128
//   5. 8 x 8 DCT        the 13-bit integer "slow-but-accurate" DCT (CONST_BITS 13, PASS1_BITS 2): rows first, results scaled by 4
//                       (terms 0 and 4 shifted left by 2, the others descaled by 11), then columns (terms 0 and 4 descaled by 2, the
//                       others by 15); DESCALE(x, n) = (x + (1 << (n - 1))) >> n; output scaled by 8.
//   6. quantisation     ITU-T T.81 Annex K.1 tables, scale = q < 50 ? 5000 / q : 200 - 2 q, entry = clip((base * scale + 50) / 100,
//                       1, 255); with qv = 8 * entry: coef -> sign * ((|coef| + (qv >> 1)) / qv).
//   7. entropy coding   Annex K.3 Huffman tables, zigzag order, DC differences per component across the frame from predictor 0,
//                       ZRL (0xF0) for every 16 zeros of a run, EOB only if the block ends in zeros, a negative amplitude v coded as
//                       v - 1 in `size` bits, bits MSB first, the last byte padded with 1-bits, 0x00 after every 0xFF byte.
//                       MCUs in raster order: 4:2:0 Y00 Y01 Y10 Y11 Cb Cr per 16 x 16 pixels, 4:4:4 Y Cb Cr per 8 x 8.
//   8. header           623 bytes: SOI, APP0 "JFIF" 1.01 (units 0, density 1 x 1), two DQT, SOF0, four DHT (DC0 AC0 DC1 AC1), SOS;
//                       EOI after the scan data.
// H and W are multiples of 16 (whole MCUs for both subsamplings).
//
// Passes (one stream, no host synchronisation, no host-to-device copy: the call can be captured in a graph):
//   blocks   one workgroup per 16 x 16 pixels: steps 1-6 through LDS -> int16 coefficients, 64 per block in zigzag order, blocks
//            in MCU order;
//   measure  one wave64 per block, lane z = coefficient z: __ballot of the non-zero lanes gives each lane its zero run, hence its
//            symbol (ZRL codes + Huffman code + amplitude, at most 59 bits) -> the block's bit count;
//   scan     one workgroup per frame: exclusive scan of the bit counts -> every block's bit offset, the frame's total;
//   emit     one wave64 per block: the lanes' symbols again, OR-ed into 64 dwords of LDS at their prefix-summed positions, then
//            shifted to the block's bit offset in the zeroed frame buffer with integer atomicOr (neighbours share dwords);
//   count    0xFF bytes per 1 KiB chunk of the (padded) scan data;
//   write    header, the chunk's bytes at offset + number of 0xFF bytes in front of it, a 0x00 after every 0xFF, EOI, the length.
// Capacity: a block emits at most 20 (DC: 9-bit code + 11 bits) + 63 * 26 (AC: 16-bit code + 10 bits) = 1658 bits, so a frame's
// stream is at most 623 + 2 * ceil(nblocks * 1658 / 8) + 2 bytes (every byte stuffed): rows of the output have that stride and
// nothing can overflow.  The only atomics are integer OR; the result does not depend on their order.
#include "common.h"

namespace lwg {
namespace {

constexpr int kHeaderBytes = 623;
constexpr int kMaxBlockBits = 20 + 63 * 26;
constexpr int kChunkBytes = 1024;      // bytes of scan data per workgroup of the count / write passes (256 lanes x one dword)

// ------------------------------------------------------------------------------------------------ constant tables
struct HuffSpec { unsigned char bits[16]; int nvals; unsigned char vals[162]; };   // Annex K.3: BITS, HUFFVAL

constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, {
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
    0xf9, 0xfa}};
constexpr HuffSpec kAcChroma = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, {
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
    0xf9, 0xfa}};

// symbol -> code | length << 16 (Annex C), 0 for a symbol the table does not hold
struct HuffLut { unsigned int e[256]; };

constexpr HuffLut make_lut(const HuffSpec &s)
{
    HuffLut lut = {};
    unsigned int code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) lut.e[s.vals[k++]] = code++ | (unsigned int)len << 16;
        code <<= 1;
    }
    return lut;
}

// the header with the quality- and size-dependent bytes left 0: they are filled in by header_byte()
struct Header { unsigned char b[kHeaderBytes]; };
constexpr int kDqtLuma = 25, kDqtChroma = 94, kSofSize = 163, kSofSampling = 169;   // offsets of the patched fields

constexpr Header make_header()
{
    Header h = {};
    int n = 0;
    const unsigned char app0[] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (unsigned char c : app0) h.b[n++] = c;
    for (int t = 0; t < 2; ++t) {
        const unsigned char dqt[] = {0xff, 0xdb, 0, 67, (unsigned char)t};
        for (unsigned char c : dqt) h.b[n++] = c;
        n += 64;
    }
    const unsigned char sof[] = {0xff, 0xc0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (unsigned char c : sof) h.b[n++] = c;
    const HuffSpec *specs[4] = {&kDcLuma, &kAcLuma, &kDcChroma, &kAcChroma};
    const unsigned char ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        const unsigned char dht[] = {0xff, 0xc4, 0, (unsigned char)(19 + specs[t]->nvals), ids[t]};
        for (unsigned char c : dht) h.b[n++] = c;
        for (int i = 0; i < 16; ++i) h.b[n++] = specs[t]->bits[i];
        for (int i = 0; i < specs[t]->nvals; ++i) h.b[n++] = specs[t]->vals[i];
    }
    const unsigned char sos[] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (unsigned char c : sos) h.b[n++] = c;
    if (n != kHeaderBytes) h.b[0] = 0;   // caught by the static_assert below
    return h;
}
static_assert(make_header().b[0] == 0xff && make_header().b[kHeaderBytes - 1] == 0, "the JFIF header is 623 bytes");

__device__ const HuffLut kLut[4] = {make_lut(kDcLuma), make_lut(kAcLuma), make_lut(kDcChroma), make_lut(kAcChroma)};
__device__ const Header kHeader = make_header();

// Annex K.1 in natural (row-major) order: luminance, chrominance
__device__ const unsigned char kBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99}};
// natural index of the k-th coefficient in zigzag order
__device__ const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ int quant_entry(int table, int natural, int scale)
{
    const int v = (kBaseQ[table][natural] * scale + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// ------------------------------------------------------------------------------------------------ pass 1: blocks
__device__ __forceinline__ int to_u8(float x)
{
    const float a = x + 1.f;
    const float h = a / 2.f;
    const float s = h * 255.f;
    return (int)fminf(fmaxf(s, 0.f), 255.f);   // fmaxf(NaN, 0) = 0
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of the DCT over eight values `stride` ints apart
template <bool kFirst>
__device__ __forceinline__ void dct_pass(int *d, int stride)
{
    constexpr int n = kFirst ? 11 : 15;
    const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride],
              d6 = d[6 * stride], d7 = d[7 * stride];
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = kFirst ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d[4 * stride] = kFirst ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2 * stride] = descale(z1 + t13 * 6270, n);
    d[6 * stride] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446;
    t5 *= 16819;
    t6 *= 25172;
    t7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * stride] = descale(t4 + z1 + z3, n);
    d[5 * stride] = descale(t5 + z2 + z4, n);
    d[3 * stride] = descale(t6 + z2 + z3, n);
    d[stride] = descale(t7 + z1 + z4, n);
}

// grid (W/16, H/16, N), 256 lanes: lane = pixel of the 16 x 16 region.  k444: the region is 4 MCUs of 3 blocks, else 1 MCU of 6.
template <bool k444>
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const float *__restrict__ x, int H, int W, int scale,
                                                          short *__restrict__ coef, int nblocks)
{
    constexpr int kBlocks = k444 ? 12 : 6;
    __shared__ int s[kBlocks][64];
    __shared__ int chroma[2][256];
    const int tid = threadIdx.x, py = tid >> 4, px = tid & 15, n = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const float *p = x + (size_t)n * 3 * plane + (size_t)(blockIdx.y * 16 + py) * W + blockIdx.x * 16 + px;
    const int r = to_u8(p[0]), g = to_u8(p[plane]), b = to_u8(p[2 * plane]);
    const int y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    const int cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    const int cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
    const int quad = (py >> 3) * 2 + (px >> 3), pos = (py & 7) * 8 + (px & 7);
    if (k444) {
        s[quad * 3][pos] = y - 128;
        s[quad * 3 + 1][pos] = cb - 128;
        s[quad * 3 + 2][pos] = cr - 128;
    } else {
        s[quad][pos] = y - 128;
        chroma[0][tid] = cb;
        chroma[1][tid] = cr;
        __syncthreads();
        if (tid < 128) {
            const int c = tid >> 6, k = tid & 63, oy = k >> 3, ox = k & 7;
            const int *q = &chroma[c][oy * 32 + ox * 2];
            // the region starts at an even output column, so the bias 1, 2, 1, 2, ... follows ox
            s[4 + c][k] = ((q[0] + q[1] + q[16] + q[17] + 1 + (ox & 1)) >> 2) - 128;
        }
    }
    __syncthreads();
    if (tid < kBlocks * 8) dct_pass<true>(&s[tid >> 3][(tid & 7) * 8], 1);
    __syncthreads();
    if (tid < kBlocks * 8) dct_pass<false>(&s[tid >> 3][tid & 7], 8);
    __syncthreads();
    short *out = coef + (size_t)n * nblocks * 64;
    for (int e = tid; e < kBlocks * 64; e += 256) {
        const int blk = e >> 6, z = e & 63, nat = kZigzag[z];
        int gblk, table;
        if (k444) {
            const int mcu = blk / 3, comp = blk - mcu * 3;
            gblk = ((blockIdx.y * 2 + (mcu >> 1)) * (W >> 3) + blockIdx.x * 2 + (mcu & 1)) * 3 + comp;
            table = comp != 0;
        } else {
            gblk = (blockIdx.y * gridDim.x + blockIdx.x) * 6 + blk;
            table = blk >= 4;
        }
        const int qv = quant_entry(table, nat, scale) * 8, v = s[blk][nat];
        const int a = ((v < 0 ? -v : v) + (qv >> 1)) / qv;
        out[(size_t)gblk * 64 + z] = (short)(v < 0 ? -a : a);
    }
}

// ------------------------------------------------------------------------------------------------ passes 2 and 4: symbols
struct Symbol { unsigned long long bits; int len; };   // right-aligned, at most 59 bits

// What lane `lane` of a block's wave contributes to the stream.  v: the lane's coefficient (lane 0: the DC difference).
__device__ __forceinline__ Symbol lane_symbol(int v, int lane, bool chroma)
{
    const unsigned int *dc = kLut[chroma ? 2 : 0].e, *ac = kLut[chroma ? 3 : 1].e;
    const unsigned long long present = __ballot(v != 0) | 1ull;   // the DC symbol is always coded
    const int a = v < 0 ? -v : v;
    const int size = a ? 32 - __clz(a) : 0;
    const unsigned long long amp = (unsigned int)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    Symbol sym = {0ull, 0};
    if (lane == 0) {
        const unsigned int e = dc[size];
        sym.bits = ((unsigned long long)(e & 0xffffu) << size) | amp;
        sym.len = (int)(e >> 16) + size;
    } else if (v != 0) {
        const int prev = 63 - __clzll((long long)(present & ((1ull << lane) - 1ull)));   // bit 0 is set: never empty
        const int run = lane - prev - 1;
        const unsigned int zrl = ac[0xf0], e = ac[((run & 15) << 4) | size];
        for (int i = 0; i < (run >> 4); ++i) {      // at most 3 x (11 or 10) bits
            sym.bits = (sym.bits << (zrl >> 16)) | (zrl & 0xffffu);
            sym.len += (int)(zrl >> 16);
        }
        sym.bits = (((sym.bits << (e >> 16)) | (e & 0xffffu)) << size) | amp;
        sym.len += (int)(e >> 16) + size;
    } else if (lane == 63) {                        // the block ends in zeros: EOB
        sym.bits = ac[0] & 0xffffu;
        sym.len = (int)(ac[0] >> 16);
    }
    return sym;
}

// the lane's coefficient of block `i` of a frame, lane 0 minus the DC of the previous block of the same component
template <bool k444>
__device__ __forceinline__ int load_lane(const short *__restrict__ frame_coef, int i, int lane, bool &chroma)
{
    int v = frame_coef[(size_t)i * 64 + lane];
    int prev;
    if (k444) {
        chroma = i % 3 != 0;
        prev = i - 3;
    } else {
        const int b = i % 6;
        chroma = b >= 4;
        prev = (b >= 1 && b <= 3) ? i - 1 : (b == 0 ? i - 3 : i - 6);
    }
    if (lane == 0 && prev >= 0) v -= frame_coef[(size_t)prev * 64];
    return v;
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// one wave64 per block, 4 per workgroup
template <bool k444>
__global__ __launch_bounds__(256) void jpeg_measure_kernel(const short *__restrict__ coef, int nblocks, long total_blocks,
                                                           unsigned int *__restrict__ nbits)
{
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= total_blocks) return;   // wave-uniform
    const long n = g / nblocks;
    const int i = (int)(g - n * nblocks);
    bool chroma;
    const int v = load_lane<k444>(coef + (size_t)n * nblocks * 64, i, lane, chroma);
    const int sum = wave_inclusive_scan(lane_symbol(v, lane, chroma).len, lane);
    if (lane == 63) nbits[g] = (unsigned int)sum;
}

// grid N, 1024 lanes: bitoff[n][i] = bits of the frame's blocks in front of block i (in place over the counts), total[n] = all
__global__ __launch_bounds__(1024) void jpeg_scan_kernel(unsigned int *__restrict__ nbits, int nblocks, unsigned int *__restrict__ total)
{
    __shared__ int wave_sum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int *f = nbits + (size_t)blockIdx.x * nblocks;
    int carry = 0;
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + tid;
        const int v = i < nblocks ? (int)f[i] : 0;
        const int incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int sw = wave_sum[w];
            before += w < wave ? sw : 0;
            all += sw;
        }
        if (i < nblocks) f[i] = (unsigned int)(carry + before + incl - v);
        carry += all;
        __syncthreads();
    }
    if (tid == 0) total[blockIdx.x] = (unsigned int)carry;
}

template <bool k444>
__global__ __launch_bounds__(256) void jpeg_emit_kernel(const short *__restrict__ coef, int nblocks, long total_blocks,
                                                        const unsigned int *__restrict__ bitoff, unsigned int *__restrict__ frame_bits,
                                                        size_t frame_dwords)
{
    __shared__ unsigned int staged[4][64];   // a block's bits, MSB first: at most 1658 of the 2048
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long g = (long)blockIdx.x * 4 + wave;
    const bool active = g < total_blocks;   // wave-uniform; every wave reaches the barriers
    unsigned int *st = staged[wave];
    st[lane] = 0u;
    __syncthreads();
    long n = 0;
    if (active) {
        n = g / nblocks;
        const int i = (int)(g - n * nblocks);
        bool chroma;
        const int v = load_lane<k444>(coef + (size_t)n * nblocks * 64, i, lane, chroma);
        const Symbol sym = lane_symbol(v, lane, chroma);
        const int at = wave_inclusive_scan(sym.len, lane) - sym.len;
        if (sym.len) {
            const unsigned long long left = sym.bits << (64 - sym.len);   // left-aligned
            const unsigned int hi = (unsigned int)(left >> 32), lo = (unsigned int)left;
            const int d = at >> 5, sh = at & 31;                          // at + len <= 1658: d + 2 <= 53
            const unsigned int w0 = hi >> sh, w1 = (sh ? hi << (32 - sh) : 0u) | (lo >> sh), w2 = sh ? lo << (32 - sh) : 0u;
            if (w0) atomicOr(&st[d], w0);
            if (w1) atomicOr(&st[d + 1], w1);
            if (w2) atomicOr(&st[d + 2], w2);
        }
    }
    __syncthreads();
    if (!active) return;
    // dword `lane` of the block's bits shifted to its place: set bits lie inside the block's own span of the frame buffer
    const unsigned int off = bitoff[g];
    const int sh = (int)(off & 31u);
    const unsigned int cur = st[lane], before = lane ? st[lane - 1] : 0u;
    const unsigned int word = (cur >> sh) | (sh ? before << (32 - sh) : 0u);
    if (word) atomicOr(frame_bits + (size_t)n * frame_dwords + (off >> 5) + lane, word);
}

// ------------------------------------------------------------------------------------------------ passes 5 and 6: bytes
// dword `di` of a frame's scan data with the last byte padded with 1-bits
__device__ __forceinline__ unsigned int padded_dword(const unsigned int *__restrict__ bits, unsigned int di, unsigned int total_bits,
                                                     unsigned int nbytes)
{
    unsigned int w = bits[di];
    if (di == (nbytes - 1) >> 2) w |= ((1u << (8u * nbytes - total_bits)) - 1u) << (24u - 8u * ((nbytes - 1u) & 3u));
    return w;
}

__device__ __forceinline__ int count_ff(unsigned int w, unsigned int first_byte, unsigned int nbytes)
{
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += first_byte + k < nbytes && ((w >> (24 - 8 * k)) & 0xffu) == 0xffu;
    return c;
}

// sum over the 256 lanes of a workgroup, returned to every lane; `incl` (optional): the inclusive prefix sum
__device__ __forceinline__ int block_sum_256(int v, int *scratch4, int *incl)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = wave_inclusive_scan(v, lane);
    __syncthreads();   // scratch4 may still be read from a previous call
    if (lane == 63) scratch4[wave] = s;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        before += w < wave ? scratch4[w] : 0;
        all += scratch4[w];
    }
    if (incl) *incl = before + s;
    return all;
}

// grid (chunks, N), 256 lanes
__global__ __launch_bounds__(256) void jpeg_count_kernel(const unsigned int *__restrict__ frame_bits, size_t frame_dwords,
                                                         const unsigned int *__restrict__ total, int nchunks,
                                                         unsigned int *__restrict__ ff_count)
{
    __shared__ int scratch[4];
    const int n = blockIdx.y;
    const unsigned int total_bits = total[n], nbytes = (total_bits + 7u) >> 3, di = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x * (unsigned int)kChunkBytes >= nbytes) return;   // workgroup-uniform; chunks past the data are never read
    const unsigned int w = padded_dword(frame_bits + (size_t)n * frame_dwords, di, total_bits, nbytes);
    const int all = block_sum_256(count_ff(w, di * 4u, nbytes), scratch, nullptr);
    if (threadIdx.x == 0) ff_count[(size_t)n * nchunks + blockIdx.x] = (unsigned int)all;
}

__device__ __forceinline__ unsigned char header_byte(int i, int H, int W, int scale, bool k444)
{
    if (i >= kDqtLuma && i < kDqtLuma + 64) return (unsigned char)quant_entry(0, kZigzag[i - kDqtLuma], scale);
    if (i >= kDqtChroma && i < kDqtChroma + 64) return (unsigned char)quant_entry(1, kZigzag[i - kDqtChroma], scale);
    if (i == kSofSize) return (unsigned char)(H >> 8);
    if (i == kSofSize + 1) return (unsigned char)H;
    if (i == kSofSize + 2) return (unsigned char)(W >> 8);
    if (i == kSofSize + 3) return (unsigned char)W;
    if (i == kSofSampling) return k444 ? 0x11 : 0x22;
    return kHeader.b[i];
}

// grid (chunks, N), 256 lanes
__global__ __launch_bounds__(256) void jpeg_write_kernel(const unsigned int *__restrict__ frame_bits, size_t frame_dwords,
                                                         const unsigned int *__restrict__ total, int nchunks,
                                                         const unsigned int *__restrict__ ff_count, int H, int W, int scale, int k444,
                                                         unsigned char *__restrict__ out, size_t row_stride, int *__restrict__ lengths)
{
    __shared__ int scratch[4];
    const int n = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const unsigned int total_bits = total[n], nbytes = (total_bits + 7u) >> 3, di = chunk * 256u + tid;
    if (chunk * (unsigned int)kChunkBytes >= nbytes) return;   // workgroup-uniform
    unsigned char *row = out + (size_t)n * row_stride;
    if (chunk == 0)
        for (int i = tid; i < kHeaderBytes; i += 256) row[i] = header_byte(i, H, W, scale, k444 != 0);
    // 0xFF bytes in the chunks in front of this one
    int mine = 0;
    for (int c = tid; c < chunk; c += 256) mine += (int)ff_count[(size_t)n * nchunks + c];
    const int in_front = block_sum_256(mine, scratch, nullptr);
    const unsigned int w = padded_dword(frame_bits + (size_t)n * frame_dwords, di, total_bits, nbytes);
    const int ff = count_ff(w, di * 4u, nbytes);
    int incl;
    block_sum_256(ff, scratch, &incl);
    size_t at = (size_t)kHeaderBytes + (size_t)di * 4u + (size_t)in_front + (size_t)(incl - ff);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned int byte_index = di * 4u + k;
        if (byte_index < nbytes) {
            const unsigned char b = (unsigned char)(w >> (24 - 8 * k));
            row[at++] = b;
            if (b == 0xff) row[at++] = 0;
            if (byte_index == nbytes - 1) {
                row[at++] = 0xff;
                row[at++] = 0xd9;
                lengths[n] = (int)at;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct Plan {
    long nblocks;          // 8 x 8 blocks per frame, all components
    size_t scan_bytes;     // capacity of a frame's scan data before stuffing
    int nchunks;           // 1 KiB chunks covering it
    size_t frame_dwords;   // dwords of a frame's bit buffer (whole chunks)
    size_t stream_bytes;   // capacity of a frame's finished stream
    // workspace layout
    size_t coef_off, nbits_off, total_off, ff_off, bits_off, bytes;
};

bool known_subsampling(int s) { return s == 420 || s == 444; }

// sizes only; false when they do not fit the kernels' 32-bit bit offsets
bool make_plan(int N, int H, int W, int subsampling, Plan &p)
{
    p.nblocks = subsampling == 444 ? (long)(H / 8) * (W / 8) * 3 : (long)(H / 16) * (W / 16) * 6;
    if (p.nblocks * kMaxBlockBits >= (1l << 31) || p.nblocks * (long)N >= (1l << 31) || N > 65535) return false;
    p.scan_bytes = (size_t)(p.nblocks * kMaxBlockBits + 7) / 8;
    p.nchunks = (int)((p.scan_bytes + kChunkBytes - 1) / kChunkBytes);
    p.frame_dwords = (size_t)p.nchunks * (kChunkBytes / 4);
    p.stream_bytes = kHeaderBytes + 2 * p.scan_bytes + 2;
    size_t at = 0;
    p.coef_off = at, at = align_up(at + (size_t)N * p.nblocks * 64 * sizeof(short), 256);
    p.nbits_off = at, at = align_up(at + (size_t)N * p.nblocks * sizeof(unsigned int), 256);
    p.total_off = at, at = align_up(at + (size_t)N * sizeof(unsigned int), 256);
    p.ff_off = at, at = align_up(at + (size_t)N * p.nchunks * sizeof(unsigned int), 256);
    p.bits_off = at, at = align_up(at + (size_t)N * p.frame_dwords * sizeof(unsigned int), 256);
    p.bytes = at;
    return true;
}

int quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

}  // namespace
}  // namespace lwg

using namespace lwg;

extern "C" {

size_t lwg_jpeg_stream_bytes(int H, int W, int subsampling)
{
    Plan p;
    if (H <= 0 || W <= 0 || H % 16 || W % 16 || !known_subsampling(subsampling) || !make_plan(1, H, W, subsampling, p)) return 0;
    return p.stream_bytes;
}

size_t lwg_jpeg_workspace_bytes(int N, int H, int W, int subsampling)
{
    Plan p;
    if (N <= 0 || H <= 0 || W <= 0 || H % 16 || W % 16 || !known_subsampling(subsampling) || !make_plan(N, H, W, subsampling, p))
        return 0;
    return p.bytes;
}

int lwg_jpeg_encode(const float *x, int N, int H, int W, int quality, int subsampling, uint8_t *out, size_t row_stride,
                    int32_t *lengths, void *workspace, size_t workspace_bytes, lwg_stream_t stream)
{
    LWG_REQUIRE(x && out && lengths && workspace, "jpeg_encode: NULL argument");
    LWG_REQUIRE(N > 0 && H > 0 && W > 0, "jpeg_encode: sizes must be positive (N=%d H=%d W=%d)", N, H, W);
    LWG_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode: quality %d is not in 1..100", quality);
    LWG_REQUIRE(known_subsampling(subsampling), "jpeg_encode: subsampling %d is neither 420 nor 444", subsampling);
    LWG_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)lengths % 4 == 0 && (uintptr_t)workspace % 16 == 0,
                "jpeg_encode: x and lengths must be 4-byte aligned, the workspace 16-byte aligned");
    if (H % 16 || W % 16 || H > 65535 || W > 65535)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "jpeg_encode: %d x %d: sides must be multiples of 16 (whole MCUs) below 65536", H, W);
    Plan p;
    if (!make_plan(N, H, W, subsampling, p)) LWG_FAIL(LWG_ERR_UNSUPPORTED, "jpeg_encode: %d frames of %d x %d are too many for one call", N, H, W);
    if (workspace_bytes < p.bytes) LWG_FAIL(LWG_ERR_WORKSPACE, "jpeg_encode: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    if (row_stride < p.stream_bytes)
        LWG_FAIL(LWG_ERR_WORKSPACE, "jpeg_encode: row stride of %zu bytes, a stream may take %zu", row_stride, p.stream_bytes);

    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    short *coef = reinterpret_cast<short *>(ws + p.coef_off);
    unsigned int *nbits = reinterpret_cast<unsigned int *>(ws + p.nbits_off), *total = reinterpret_cast<unsigned int *>(ws + p.total_off),
                 *ff = reinterpret_cast<unsigned int *>(ws + p.ff_off), *bits = reinterpret_cast<unsigned int *>(ws + p.bits_off);
    const bool k444 = subsampling == 444;
    const int scale = quality_scale(quality), nblocks = (int)p.nblocks;
    const long total_blocks = p.nblocks * N;
    const dim3 regions(W / 16, H / 16, N), chunks(p.nchunks, N);
    const int waves4 = ceil_div(total_blocks, 4);

    LWG_HIP(hipMemsetAsync(bits, 0, (size_t)N * p.frame_dwords * sizeof(unsigned int), st));
    if (k444) {
        jpeg_blocks_kernel<true><<<regions, 256, 0, st>>>(x, H, W, scale, coef, nblocks);
        jpeg_measure_kernel<true><<<waves4, 256, 0, st>>>(coef, nblocks, total_blocks, nbits);
    } else {
        jpeg_blocks_kernel<false><<<regions, 256, 0, st>>>(x, H, W, scale, coef, nblocks);
        jpeg_measure_kernel<false><<<waves4, 256, 0, st>>>(coef, nblocks, total_blocks, nbits);
    }
    LWG_LAUNCH_CHECK("jpeg_blocks_kernel / jpeg_measure_kernel");
    jpeg_scan_kernel<<<N, 1024, 0, st>>>(nbits, nblocks, total);
    LWG_LAUNCH_CHECK("jpeg_scan_kernel");
    if (k444)
        jpeg_emit_kernel<true><<<waves4, 256, 0, st>>>(coef, nblocks, total_blocks, nbits, bits, p.frame_dwords);
    else
        jpeg_emit_kernel<false><<<waves4, 256, 0, st>>>(coef, nblocks, total_blocks, nbits, bits, p.frame_dwords);
    LWG_LAUNCH_CHECK("jpeg_emit_kernel");
    jpeg_count_kernel<<<chunks, 256, 0, st>>>(bits, p.frame_dwords, total, p.nchunks, ff);
    LWG_LAUNCH_CHECK("jpeg_count_kernel");
    jpeg_write_kernel<<<chunks, 256, 0, st>>>(bits, p.frame_dwords, total, p.nchunks, ff, H, W, scale, (int)k444, out, row_stride,
                                              lengths);
    LWG_LAUNCH_CHECK("jpeg_write_kernel");
    return LWG_OK;
}

}  // extern "C"
