// inception.hip -- torchvision's inception_v3 cut at the final average pool (the reference's InceptionV3(output_blocks=[3],
// resize_input=False, normalize_input=False): thirdparty/his_evaluators/.../metrics/metrics.py:16-158, 197-205) for the set
// metrics FID and Inception Score (metrics.py:634-781): frames in, 2048 fp32 features per frame out.
//
// 94 x (Conv2d(bias=False) + BatchNorm2d(eps=1e-3, eval) + ReLU), two MaxPool(3,2), nine avg_pool2d(3,1,1), a global average pool.
//
//   igemm32::conv_kernel<InceptionFrames> / <InceptionNhwc>: the exact-fp32 implicit GEMM of igemm32.h on v_mfma_f32_32x32x2_f32,
//   shared with hmr.hip and lpips.hip; this file states what is Inception's own, as the policy struct InceptionConv.  kh, kw,
//   stride, ph and pw are independent; Cout is predicated (48, 80, 320, 448 occur); the output goes to a channel offset with a
//   channel pitch, so the branches of a Mixed block write their slices of the concatenated buffer themselves.  Epilogue:
//   fmaf(acc, scale, shift), the BatchNorm folded on the host in fp64 and rounded once to fp32, then ReLU.  The first convolution
//   reads the (n,3,H,W) NCHW frames through the evaluator's pixel modes (map_pixel of pixel.h).
//
//   maxpool3s2_kernel (maxpool.h) at floor-mode sizes: F.max_pool2d(3, 2), NHWC, into a channel slice.
//   inception_avgpool_kernel: F.avg_pool2d(3, 1, 1), count_include_pad=True: the nine taps added in (kh, kw) order, padded taps 0,
//   divided by 9.
//   inception_global_pool_kernel: the mean over the pixels, added in ascending pixel order in fp64, rounded once.
//   inception_prep_kernel: the pixel mode, then F.interpolate(bilinear, align_corners=False) to the network's input size.
//
// No atomics.  The reduction order of every number depends on nothing but its own indices: a frame's features are the same bits
// at any batch size and any position in the batch.  One stream, no host synchronisation and no allocation in forward: capturable
// as a single chain of launches.
#include <cstring>

#include "common.h"
#include "igemm32.h"
#include "maxpool.h"
#include "pixel.h"

namespace lwg {
namespace {

// Conv2d(bias=False) + BatchNorm + ReLU into a channel slice, as a policy of igemm32::conv_kernel; InceptionFrames and InceptionNhwc
// add the gather
struct InceptionConv {
    igemm32::Geom g;
    const float *x;          // NHWC (N,H,W,Cin); InceptionFrames: (N,3,H,W) NCHW frames
    const float *scale;      // (Cout) or NULL
    const float *shift;      // (Cout) or NULL
    float *y;                // (N,Ho,Wo,y_pitch), this convolution's channels at y_off
    int relu, mode, y_pitch, y_off;
    static constexpr bool kCoutTail = true;   // 48, 80, 320, 448 occur

    struct Col {
        float scale, shift;
    };
    __device__ Col column(int co) const { return Col{scale ? scale[co] : 1.f, shift ? shift[co] : 0.f}; }
    __device__ void write(long m, int co, const Col &c, float v) const
    {
        if (scale || shift) v = fmaf(v, c.scale, c.shift);   // one rounding
        if (relu) v = fmaxf(v, 0.f);
        y[(size_t)m * y_pitch + y_off + co] = v;
    }
};

// Cin == 3, NCHW frames through map_pixel
struct InceptionFrames : InceptionConv {
    __device__ float4 gather(const igemm32::Row &r, int kg) const
    {
        const float *base = x + (size_t)r.n * g.H * g.W * g.Cin;
        return igemm32::gather_each(g, r, kg, 3, [&](int c, int ih, int iw) {
            return map_pixel(base[((size_t)c * g.H + ih) * g.W + iw], mode);
        });
    }
};

// Cin % 4 == 0, four consecutive reduction indices are one 16-byte load inside one tap
struct InceptionNhwc : InceptionConv {
    __device__ float4 gather(const igemm32::Row &r, int kg) const { return igemm32::gather_nhwc4(g, x, r, kg); }
};

// avg_pool2d(kernel 3, stride 1, padding 1), count_include_pad=True, NHWC, C % 4 == 0: the taps inside the image added in
// (kh, kw) order (a padded tap is a zero, which changes no sum), then a true division by 9
__global__ __launch_bounds__(256) void inception_avgpool_kernel(const float *__restrict__ x, int H, int W, int C4, long total,
                                                               float *__restrict__ y)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // over N*H*W*C4
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    long px = i / C4;
    const int ow = (int)(px % W);
    px /= W;
    const int oh = (int)(px % H);
    const long n = px / H;
    const float4 *xs = reinterpret_cast<const float4 *>(x);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = -1; kh <= 1; ++kh) {
#pragma unroll
        for (int kw = -1; kw <= 1; ++kw) {
            const int ih = oh + kh, iw = ow + kw;
            if ((unsigned)ih >= (unsigned)H || (unsigned)iw >= (unsigned)W) continue;
            const float4 v = xs[((n * H + ih) * W + iw) * C4 + c4];
            s.x += v.x;
            s.y += v.y;
            s.z += v.z;
            s.w += v.w;
        }
    }
    reinterpret_cast<float4 *>(y)[i] = make_float4(s.x / 9.f, s.y / 9.f, s.z / 9.f, s.w / 9.f);
}

// x (N,P,C) NHWC -> y (N,C): the P pixels added in ascending order in fp64, divided by P in fp64, rounded once to fp32
__global__ __launch_bounds__(256) void inception_global_pool_kernel(const float *__restrict__ x, int P, int C, long total,
                                                                   float *__restrict__ y)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // over N*C
    if (i >= total) return;
    const int c = (int)(i % C);
    const long n = i / C;
    const float *q = x + (size_t)n * P * C + c;
    double s = 0.0;
    for (int px = 0; px < P; ++px) s += (double)q[(size_t)px * C];
    y[i] = (float)(s / (double)P);
}

// frames (N,3,H,W) -> (N,3,Ho,Wo): the pixel mode first (the reference's `out *= 2; out -= 1`), then the resize
__global__ __launch_bounds__(256) void inception_prep_kernel(const float *__restrict__ x, int H, int W, int Ho, int Wo, int mode,
                                                            long total, float *__restrict__ y)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const long plane = i / ((long)Wo * Ho);
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    linear_taps(sy, yo, H, y0, y1, wy0, wy1);
    linear_taps(sx, xo, W, x0, x1, wx0, wx1);
    const float *r0 = x + (size_t)plane * H * W + (size_t)y0 * W;
    const float *r1 = x + (size_t)plane * H * W + (size_t)y1 * W;
    const float top = map_pixel(r0[x0], mode) * wx0 + map_pixel(r0[x1], mode) * wx1;
    const float bot = map_pixel(r1[x0], mode) * wx0 + map_pixel(r1[x1], mode) * wx1;
    y[i] = top * wy0 + bot * wy1;
}

// ------------------------------------------------------------------------------------------------ host side
using igemm32::aligned16;
using igemm32::conv_out;

int launch_conv(const InceptionConv &p, bool image, hipStream_t st)
{
    if (image) return igemm32::launch(InceptionFrames{p}, "igemm32::conv_kernel<InceptionFrames>", st);
    return igemm32::launch(InceptionNhwc{p}, "igemm32::conv_kernel<InceptionNhwc>", st);
}

// F.max_pool2d(3, 2), floor mode, into a channel slice
int launch_floor_maxpool(const float *x, int N, int H, int W, int C, float *y, int pitch, int off, hipStream_t st)
{
    return launch_maxpool(x, N, H, W, C, pool_out(H), pool_out(W), y, pitch, off, st);
}

int launch_avgpool(const float *x, int N, int H, int W, int C, float *y, hipStream_t st)
{
    const long total = (long)N * H * W * (C / 4);
    inception_avgpool_kernel<<<ceil_div(total, 256), 256, 0, st>>>(x, H, W, C / 4, total, y);
    LWG_LAUNCH_CHECK("inception_avgpool_kernel");
    return LWG_OK;
}

int launch_global_pool(const float *x, int N, int P, int C, float *y, hipStream_t st)
{
    const long total = (long)N * C;
    inception_global_pool_kernel<<<ceil_div(total, 256), 256, 0, st>>>(x, P, C, total, y);
    LWG_LAUNCH_CHECK("inception_global_pool_kernel");
    return LWG_OK;
}

// ---- the network as a list of launches.  The same walk sizes the buffers (create, at the largest input) and drives a forward.
constexpr int kConvs = 94, kMaxOps = 128, kStages = 18, kNetSize = 299;
enum { OP_CONV = 0, OP_MAXPOOL = 1, OP_AVGPOOL = 2 };
// IN: the frames (or the resized frames); A / B: a block's input and output, alternating; T0 / T1: what the inner convolutions of a
// branch hand on; P: the block input after avg_pool2d
enum { BUF_IN = -1, BUF_A = 0, BUF_B = 1, BUF_T0 = 2, BUF_T1 = 3, BUF_P = 4, NBUF = 5 };

struct ConvDef {
    int cin, cout, kh, kw, stride, ph, pw;
    long w_off;              // blob offset in floats: w (kh*kw*cin*cout) | scale (cout) | shift (cout)
};
struct Op {
    int kind, src, dst, H, W, C, Ho, Wo, off, pitch, conv;
};
struct Stage {
    int buf, H, W, C, end_op;    // complete once ops[0 .. end_op - 1] have run
};
struct Plan {
    ConvDef convs[kConvs];
    Op ops[kMaxOps];
    Stage stages[kStages];
    int nconv = 0, nops = 0, nstages = 0;
    size_t need[NBUF] = {0};     // floats per image
    long blob_floats = 0;
    bool ok = true;              // false: some stage has no pixel at this input size
};

struct Walker {
    Plan &p;
    explicit Walker(Plan &plan) : p(plan) {}
    void grow(int buf, size_t floats)
    {
        if (buf >= 0 && floats > p.need[buf]) p.need[buf] = floats;
    }
    // a "conv" of the issue: Conv2d(bias=False) + BatchNorm + ReLU, its channels written at `off` of a `pitch`-channel buffer
    void conv(int src, int H, int W, int cin, int cout, int kh, int kw, int stride, int ph, int pw, int dst, int off, int pitch)
    {
        ConvDef &d = p.convs[p.nconv];
        d = ConvDef{cin, cout, kh, kw, stride, ph, pw, p.blob_floats};
        p.blob_floats += (long)kh * kw * cin * cout + 2 * cout;
        Op &o = p.ops[p.nops++];
        o = Op{OP_CONV, src, dst, H, W, cin, conv_out(H, kh, stride, ph), conv_out(W, kw, stride, pw), off, pitch, p.nconv++};
        if (o.Ho < 1 || o.Wo < 1) p.ok = false;
        grow(dst, (size_t)o.Ho * o.Wo * pitch);
    }
    void k1(int src, int H, int W, int cin, int cout, int dst, int off, int pitch) { conv(src, H, W, cin, cout, 1, 1, 1, 0, 0, dst, off, pitch); }
    void maxpool(int src, int H, int W, int C, int dst, int off, int pitch)
    {
        Op &o = p.ops[p.nops++];
        o = Op{OP_MAXPOOL, src, dst, H, W, C, pool_out(H), pool_out(W), off, pitch, -1};
        if (o.Ho < 1 || o.Wo < 1) p.ok = false;
        grow(dst, (size_t)o.Ho * o.Wo * pitch);
    }
    void avgpool(int src, int H, int W, int C, int dst)
    {
        p.ops[p.nops++] = Op{OP_AVGPOOL, src, dst, H, W, C, H, W, 0, C, -1};
        grow(dst, (size_t)H * W * C);
    }
    void stage(int buf, int H, int W, int C) { p.stages[p.nstages++] = Stage{buf, H, W, C, p.nops}; }

    void inception_a(int in, int out, int H, int W, int C, int pf)
    {
        const int pitch = 224 + pf;
        k1(in, H, W, C, 64, out, 0, pitch);                                   // branch1x1
        k1(in, H, W, C, 48, BUF_T0, 0, 48);                                   // branch5x5_1
        conv(BUF_T0, H, W, 48, 64, 5, 5, 1, 2, 2, out, 64, pitch);            // branch5x5_2
        k1(in, H, W, C, 64, BUF_T0, 0, 64);                                   // branch3x3dbl_1
        conv(BUF_T0, H, W, 64, 96, 3, 3, 1, 1, 1, BUF_T1, 0, 96);             // branch3x3dbl_2
        conv(BUF_T1, H, W, 96, 96, 3, 3, 1, 1, 1, out, 128, pitch);           // branch3x3dbl_3
        avgpool(in, H, W, C, BUF_P);
        k1(BUF_P, H, W, C, pf, out, 224, pitch);                              // branch_pool
        stage(out, H, W, pitch);
    }
    void inception_b(int in, int out, int H, int W)                           // 288 -> 768, stride 2
    {
        conv(in, H, W, 288, 384, 3, 3, 2, 0, 0, out, 0, 768);                 // branch3x3
        k1(in, H, W, 288, 64, BUF_T0, 0, 64);                                 // branch3x3dbl_1
        conv(BUF_T0, H, W, 64, 96, 3, 3, 1, 1, 1, BUF_T1, 0, 96);             // branch3x3dbl_2
        conv(BUF_T1, H, W, 96, 96, 3, 3, 2, 0, 0, out, 384, 768);             // branch3x3dbl_3
        maxpool(in, H, W, 288, out, 480, 768);
        stage(out, pool_out(H), pool_out(W), 768);
    }
    void inception_c(int in, int out, int H, int W, int c7)
    {
        k1(in, H, W, 768, 192, out, 0, 768);                                  // branch1x1
        k1(in, H, W, 768, c7, BUF_T0, 0, c7);                                 // branch7x7_1
        conv(BUF_T0, H, W, c7, c7, 1, 7, 1, 0, 3, BUF_T1, 0, c7);             // branch7x7_2
        conv(BUF_T1, H, W, c7, 192, 7, 1, 1, 3, 0, out, 192, 768);            // branch7x7_3
        k1(in, H, W, 768, c7, BUF_T0, 0, c7);                                 // branch7x7dbl_1
        conv(BUF_T0, H, W, c7, c7, 7, 1, 1, 3, 0, BUF_T1, 0, c7);             // branch7x7dbl_2
        conv(BUF_T1, H, W, c7, c7, 1, 7, 1, 0, 3, BUF_T0, 0, c7);             // branch7x7dbl_3
        conv(BUF_T0, H, W, c7, c7, 7, 1, 1, 3, 0, BUF_T1, 0, c7);             // branch7x7dbl_4
        conv(BUF_T1, H, W, c7, 192, 1, 7, 1, 0, 3, out, 384, 768);            // branch7x7dbl_5
        avgpool(in, H, W, 768, BUF_P);
        k1(BUF_P, H, W, 768, 192, out, 576, 768);                             // branch_pool
        stage(out, H, W, 768);
    }
    void inception_d(int in, int out, int H, int W)                           // 768 -> 1280, stride 2
    {
        k1(in, H, W, 768, 192, BUF_T0, 0, 192);                               // branch3x3_1
        conv(BUF_T0, H, W, 192, 320, 3, 3, 2, 0, 0, out, 0, 1280);            // branch3x3_2
        k1(in, H, W, 768, 192, BUF_T0, 0, 192);                               // branch7x7x3_1
        conv(BUF_T0, H, W, 192, 192, 1, 7, 1, 0, 3, BUF_T1, 0, 192);          // branch7x7x3_2
        conv(BUF_T1, H, W, 192, 192, 7, 1, 1, 3, 0, BUF_T0, 0, 192);          // branch7x7x3_3
        conv(BUF_T0, H, W, 192, 192, 3, 3, 2, 0, 0, out, 320, 1280);          // branch7x7x3_4
        maxpool(in, H, W, 768, out, 512, 1280);
        stage(out, pool_out(H), pool_out(W), 1280);
    }
    void inception_e(int in, int out, int H, int W, int C)
    {
        k1(in, H, W, C, 320, out, 0, 2048);                                   // branch1x1
        k1(in, H, W, C, 384, BUF_T0, 0, 384);                                 // branch3x3_1
        conv(BUF_T0, H, W, 384, 384, 1, 3, 1, 0, 1, out, 320, 2048);          // branch3x3_2a
        conv(BUF_T0, H, W, 384, 384, 3, 1, 1, 1, 0, out, 704, 2048);          // branch3x3_2b
        k1(in, H, W, C, 448, BUF_T0, 0, 448);                                 // branch3x3dbl_1
        conv(BUF_T0, H, W, 448, 384, 3, 3, 1, 1, 1, BUF_T1, 0, 384);          // branch3x3dbl_2
        conv(BUF_T1, H, W, 384, 384, 1, 3, 1, 0, 1, out, 1088, 2048);         // branch3x3dbl_3a
        conv(BUF_T1, H, W, 384, 384, 3, 1, 1, 1, 0, out, 1472, 2048);         // branch3x3dbl_3b
        avgpool(in, H, W, C, BUF_P);
        k1(BUF_P, H, W, C, 192, out, 1856, 2048);                             // branch_pool
        stage(out, H, W, 2048);
    }

    // the whole network for an H x W input; the convolutions in torchvision's definition order, which is the blob's order
    void network(int H, int W)
    {
        auto co = [](int v, int k, int s, int pad) { return conv_out(v, k, s, pad); };
        conv(BUF_IN, H, W, 3, 32, 3, 3, 2, 0, 0, BUF_A, 0, 32);               // Conv2d_1a_3x3
        H = co(H, 3, 2, 0), W = co(W, 3, 2, 0);
        stage(BUF_A, H, W, 32);
        conv(BUF_A, H, W, 32, 32, 3, 3, 1, 0, 0, BUF_B, 0, 32);               // Conv2d_2a_3x3
        H = co(H, 3, 1, 0), W = co(W, 3, 1, 0);
        stage(BUF_B, H, W, 32);
        conv(BUF_B, H, W, 32, 64, 3, 3, 1, 1, 1, BUF_A, 0, 64);               // Conv2d_2b_3x3
        stage(BUF_A, H, W, 64);
        maxpool(BUF_A, H, W, 64, BUF_B, 0, 64);
        H = pool_out(H), W = pool_out(W);
        stage(BUF_B, H, W, 64);
        k1(BUF_B, H, W, 64, 80, BUF_A, 0, 80);                                // Conv2d_3b_1x1
        stage(BUF_A, H, W, 80);
        conv(BUF_A, H, W, 80, 192, 3, 3, 1, 0, 0, BUF_B, 0, 192);             // Conv2d_4a_3x3
        H = co(H, 3, 1, 0), W = co(W, 3, 1, 0);
        stage(BUF_B, H, W, 192);
        maxpool(BUF_B, H, W, 192, BUF_A, 0, 192);
        H = pool_out(H), W = pool_out(W);
        stage(BUF_A, H, W, 192);
        inception_a(BUF_A, BUF_B, H, W, 192, 32);                             // Mixed_5b
        inception_a(BUF_B, BUF_A, H, W, 256, 64);                             // Mixed_5c
        inception_a(BUF_A, BUF_B, H, W, 288, 64);                             // Mixed_5d
        inception_b(BUF_B, BUF_A, H, W);                                      // Mixed_6a
        H = pool_out(H), W = pool_out(W);
        inception_c(BUF_A, BUF_B, H, W, 128);                                 // Mixed_6b
        inception_c(BUF_B, BUF_A, H, W, 160);                                 // Mixed_6c
        inception_c(BUF_A, BUF_B, H, W, 160);                                 // Mixed_6d
        inception_c(BUF_B, BUF_A, H, W, 192);                                 // Mixed_6e
        inception_d(BUF_A, BUF_B, H, W);                                      // Mixed_7a
        H = pool_out(H), W = pool_out(W);
        inception_e(BUF_B, BUF_A, H, W, 1280);                                // Mixed_7b
        inception_e(BUF_A, BUF_B, H, W, 2048);                                // Mixed_7c
        if (H < 1 || W < 1) p.ok = false;
    }
};

constexpr int kMinSize = 75;   // 75 -> 37 -> 35 -> 17 -> 15 -> 7 -> 3 -> 1: the smallest input at which Mixed_7c still has a pixel

}  // namespace
}  // namespace lwg

using namespace lwg;

struct lwg_inception {
    int max_images = 0, max_h = 0, max_w = 0;
    Plan plan;                         // at the largest network input: the buffer sizes and the blob layout
    float *blob = nullptr;
    float *buf[NBUF] = {nullptr};
    float *resized = nullptr;          // (max_images, 3, 299, 299)
    bool ready = false;
};

extern "C" {

int lwg_inception_create(lwg_inception **out, int max_images, int max_h, int max_w)
{
    LWG_REQUIRE(out != nullptr, "lwg_inception_create: NULL output handle");
    *out = nullptr;
    LWG_REQUIRE(max_images >= 1 && max_images <= 4096, "lwg_inception_create: max_images %d outside 1..4096", max_images);
    LWG_REQUIRE(max_h >= 1 && max_w >= 1 && max_h <= 8192 && max_w <= 8192, "lwg_inception_create: max_h x max_w = %d x %d outside 1..8192",
                max_h, max_w);
    lwg_inception *h = new lwg_inception();
    h->max_images = max_images;
    h->max_h = max_h;
    h->max_w = max_w;
    // a frame is either resized to 299 x 299 or taken as it is: the network input is at most the larger of the two
    Walker(h->plan).network(max_h > kNetSize ? max_h : kNetSize, max_w > kNetSize ? max_w : kNetSize);
    hipError_t e = alloc_floats(&h->blob, (size_t)h->plan.blob_floats);
    for (int b = 0; b < NBUF && e == hipSuccess; ++b) e = alloc_floats(&h->buf[b], (size_t)max_images * h->plan.need[b]);
    if (e == hipSuccess) e = alloc_floats(&h->resized, (size_t)max_images * 3 * kNetSize * kNetSize);
    if (e != hipSuccess) {
        lwg_inception_destroy(h);
        LWG_FAIL(LWG_ERR_HIP, "lwg_inception_create: hipMalloc failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return LWG_OK;
}

void lwg_inception_destroy(lwg_inception *h)
{
    if (!h) return;
    free_device(h->blob);
    for (int b = 0; b < NBUF; ++b) free_device(h->buf[b]);
    free_device(h->resized);
    delete h;
}

size_t lwg_inception_weight_floats(void)
{
    Plan plan;
    Walker(plan).network(kNetSize, kNetSize);
    return (size_t)plan.blob_floats;
}

int lwg_inception_set_weights(lwg_inception *h, const float *blob_host, size_t n_floats)
{
    LWG_REQUIRE(h != nullptr, "lwg_inception_set_weights: NULL handle");
    LWG_REQUIRE(blob_host != nullptr, "lwg_inception_set_weights: NULL blob");
    LWG_REQUIRE(n_floats == (size_t)h->plan.blob_floats, "lwg_inception_set_weights: blob of %zu floats, this network takes %ld", n_floats,
                h->plan.blob_floats);
    return upload_blob(h->blob, blob_host, n_floats, h->ready);
}

int lwg_inception_forward(lwg_inception *h, const float *frames, int n, int H, int W, int mode, int out_h, int out_w, float *features,
                          int tap_stage, float *tap_out, lwg_stream_t stream)
{
    LWG_REQUIRE(h != nullptr, "lwg_inception_forward: NULL handle");
    LWG_REQUIRE(frames != nullptr && features != nullptr, "lwg_inception_forward: NULL frames or features");
    LWG_REQUIRE(n >= 1 && H >= 1 && W >= 1, "lwg_inception_forward: sizes must be positive (n=%d H=%d W=%d)", n, H, W);
    LWG_REQUIRE(mode >= 0 && mode <= 2, "lwg_inception_forward: mode %d is none of 0 (as is), 1 ([0,1] input), 2 (8-bit round trip)", mode);
    LWG_REQUIRE((out_h == 0 && out_w == 0) || (out_h == kNetSize && out_w == kNetSize),
                "lwg_inception_forward: the resize target %d x %d is neither 0 x 0 (no resize) nor %d x %d", out_h, out_w, kNetSize, kNetSize);
    LWG_REQUIRE(tap_stage >= -1 && tap_stage < kStages, "lwg_inception_forward: tap_stage %d outside -1..%d", tap_stage, kStages - 1);
    LWG_REQUIRE(tap_stage < 0 || tap_out != nullptr, "lwg_inception_forward: tap_stage %d without tap_out", tap_stage);
    LWG_REQUIRE(((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(features) | reinterpret_cast<uintptr_t>(tap_out)) & 3) == 0,
                "lwg_inception_forward: frames, features and tap_out must be 4-byte aligned");
    const int nh = out_h ? out_h : H, nw = out_w ? out_w : W;   // the network's input
    if (nh < kMinSize || nw < kMinSize)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_forward: a %d x %d network input is below %d x %d, the smallest at which Mixed_7c has a pixel",
                 nh, nw, kMinSize, kMinSize);
    if (n > h->max_images) LWG_FAIL(LWG_ERR_STATE, "lwg_inception_forward: n = %d above max_images = %d", n, h->max_images);
    if (H > h->max_h || W > h->max_w)
        LWG_FAIL(LWG_ERR_STATE, "lwg_inception_forward: %d x %d above max_h x max_w = %d x %d", H, W, h->max_h, h->max_w);
    if (!h->ready) LWG_FAIL(LWG_ERR_STATE, "lwg_inception_forward: no weights set");
    Plan plan;
    Walker(plan).network(nh, nw);
    if (!plan.ok) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_forward: a stage of the network has no pixel at %d x %d", nh, nw);
    for (int b = 0; b < NBUF; ++b)       // cannot happen (the handle is sized for the largest input); checked all the same
        if (plan.need[b] > h->plan.need[b]) LWG_FAIL(LWG_ERR_STATE, "lwg_inception_forward: buffer %d too small for %d x %d", b, nh, nw);
    hipStream_t st = as_stream(stream);
    const float *input = frames;
    int in_mode = mode;
    if (out_h) {
        const long total = (long)n * 3 * nh * nw;
        inception_prep_kernel<<<ceil_div(total, 256), 256, 0, st>>>(frames, H, W, nh, nw, mode, total, h->resized);
        LWG_LAUNCH_CHECK("inception_prep_kernel");
        input = h->resized;
        in_mode = 0;
    }
    auto src_of = [&](int b) -> const float * { return b == BUF_IN ? input : h->buf[b]; };
    for (int i = 0; i < plan.nops; ++i) {
        const Op &o = plan.ops[i];
        int rc = LWG_OK;
        if (o.kind == OP_CONV) {
            const ConvDef &d = plan.convs[o.conv];
            InceptionConv p;
            memset(&p, 0, sizeof(p));
            p.g = igemm32::geom(h->blob + d.w_off, n, o.H, o.W, d.cin, d.cout, d.kh, d.kw, d.stride, d.ph, d.pw);
            p.x = src_of(o.src);
            p.scale = p.g.w + (size_t)d.kh * d.kw * d.cin * d.cout;
            p.shift = p.scale + d.cout;
            p.y = h->buf[o.dst];
            p.relu = 1; p.mode = in_mode; p.y_pitch = o.pitch; p.y_off = o.off;
            rc = launch_conv(p, o.src == BUF_IN, st);
        } else if (o.kind == OP_MAXPOOL) {
            rc = launch_floor_maxpool(src_of(o.src), n, o.H, o.W, o.C, h->buf[o.dst], o.pitch, o.off, st);
        } else {
            rc = launch_avgpool(src_of(o.src), n, o.H, o.W, o.C, h->buf[o.dst], st);
        }
        if (rc != LWG_OK) return rc;
        if (tap_stage >= 0 && plan.stages[tap_stage].end_op == i + 1) {   // before A / B are written again
            const Stage &s = plan.stages[tap_stage];
            LWG_HIP(hipMemcpyAsync(tap_out, h->buf[s.buf], (size_t)n * s.H * s.W * s.C * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    const Stage &last = plan.stages[kStages - 1];
    return launch_global_pool(h->buf[last.buf], n, last.H * last.W, last.C, features, st);
}

int lwg_inception_conv(const float *x, int N, int H, int W, int Cin, const float *w, const float *scale, const float *shift, int Cout,
                       int kh, int kw, int stride, int ph, int pw, int relu, int input_mode, float *y, int y_pitch, int y_offset,
                       lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "lwg_inception_conv: NULL x, w or y");
    LWG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "lwg_inception_conv: non-positive size");
    LWG_REQUIRE(kh >= 1 && kw >= 1 && kh <= 11 && kw <= 11 && stride >= 1 && stride <= 4 && ph >= 0 && pw >= 0 && ph < kh && pw < kw,
                "lwg_inception_conv: (kh, kw, stride, ph, pw) = (%d, %d, %d, %d, %d) outside kh, kw 1..11, stride 1..4, 0 <= ph < kh, 0 <= pw < kw",
                kh, kw, stride, ph, pw);
    LWG_REQUIRE(relu == 0 || relu == 1, "lwg_inception_conv: relu = %d is neither 0 nor 1", relu);
    LWG_REQUIRE(input_mode <= 2, "lwg_inception_conv: input_mode %d is none of < 0 (NHWC), 0, 1, 2 (NCHW frames in that pixel mode)", input_mode);
    LWG_REQUIRE(input_mode < 0 || Cin == 3, "lwg_inception_conv: the frame prologue takes 3 channels, got Cin = %d", Cin);
    LWG_REQUIRE(y_pitch >= 1 && y_offset >= 0 && (long)y_offset + Cout <= y_pitch,
                "lwg_inception_conv: channels %d..%d do not fit a pitch of %d", y_offset, y_offset + Cout - 1, y_pitch);
    // 16-byte accesses: the weight rows always, the input when it is NHWC
    LWG_REQUIRE(aligned16(w), "lwg_inception_conv: w is not 16-byte aligned");
    LWG_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(scale) |
                  reinterpret_cast<uintptr_t>(shift)) & 3) == 0, "lwg_inception_conv: x / y / scale / shift are not 4-byte aligned");
    LWG_REQUIRE(input_mode >= 0 || aligned16(x), "lwg_inception_conv: x is not 16-byte aligned");
    if (input_mode < 0 && Cin % 4 != 0) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_conv: Cin = %d is neither 3 (frames) nor a multiple of 4", Cin);
    if (Cout % 4 != 0) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_conv: Cout = %d is no multiple of 4", Cout);
    const int Ho = conv_out(H, kh, stride, ph), Wo = conv_out(W, kw, stride, pw);
    LWG_REQUIRE(Ho >= 1 && Wo >= 1, "lwg_inception_conv: empty output");
    if (igemm32::too_large(N, H, W, Cin) || igemm32::too_large(N, Ho, Wo, y_pitch) || igemm32::grid_too_large(N, Ho, Wo, kh, kw, Cin))
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_conv: tensor too large");
    InceptionConv p;
    memset(&p, 0, sizeof(p));
    p.g = igemm32::geom(w, N, H, W, Cin, Cout, kh, kw, stride, ph, pw);
    p.x = x; p.scale = scale; p.shift = shift; p.y = y;
    p.relu = relu; p.mode = input_mode < 0 ? 0 : input_mode; p.y_pitch = y_pitch; p.y_off = y_offset;
    return launch_conv(p, input_mode >= 0, as_stream(stream));
}

int lwg_inception_maxpool(const float *x, int N, int H, int W, int C, float *y, int y_pitch, int y_offset, lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && y != nullptr, "lwg_inception_maxpool: NULL x or y");
    LWG_REQUIRE(N >= 1 && H >= 3 && W >= 3 && C >= 1, "lwg_inception_maxpool: needs N, C >= 1 and H, W >= 3");
    LWG_REQUIRE(y_pitch >= 1 && y_offset >= 0 && (long)y_offset + C <= y_pitch,
                "lwg_inception_maxpool: channels %d..%d do not fit a pitch of %d", y_offset, y_offset + C - 1, y_pitch);
    if (C % 4 != 0 || y_pitch % 4 != 0 || y_offset % 4 != 0)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_maxpool: C = %d, pitch %d, offset %d are not all multiples of 4", C, y_pitch, y_offset);
    LWG_REQUIRE(aligned16(x) && aligned16(y), "lwg_inception_maxpool: x / y are not 16-byte aligned");
    if ((long)N * H * W * (C / 4) > 256L * 0x7fffffffL || igemm32::too_large(N, pool_out(H), pool_out(W), y_pitch))
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_maxpool: tensor too large");
    return launch_floor_maxpool(x, N, H, W, C, y, y_pitch, y_offset, as_stream(stream));
}

int lwg_inception_avgpool(const float *x, int N, int H, int W, int C, float *y, lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && y != nullptr, "lwg_inception_avgpool: NULL x or y");
    LWG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, "lwg_inception_avgpool: non-positive size");
    if (C % 4 != 0) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_avgpool: C = %d is no multiple of 4", C);
    LWG_REQUIRE(aligned16(x) && aligned16(y), "lwg_inception_avgpool: x / y are not 16-byte aligned");
    if ((long)N * H * W * (C / 4) > 256L * 0x7fffffffL) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_avgpool: tensor too large");
    return launch_avgpool(x, N, H, W, C, y, as_stream(stream));
}

int lwg_inception_global_pool(const float *x, int N, int P, int C, float *y, lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && y != nullptr, "lwg_inception_global_pool: NULL x or y");
    LWG_REQUIRE(N >= 1 && P >= 1 && C >= 1, "lwg_inception_global_pool: sizes must be positive (N=%d P=%d C=%d)", N, P, C);
    LWG_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 3) == 0, "lwg_inception_global_pool: x / y are not 4-byte aligned");
    if ((long)N * C > 256L * 0x7fffffffL || (long)N * P * (long)C >= (1L << 40)) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_inception_global_pool: tensor too large");
    return launch_global_pool(x, N, P, C, y, as_stream(stream));
}

}  // extern "C"
