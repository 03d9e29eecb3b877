// hmr.hip -- the HMR image -> SMPL regressor (reference: networks/hmr.py:119-300) in eval mode, exact fp32:
// a pre-activation ResNet-50 (v2), a global average pool and the 3-iteration ThetaRegressor.
//
// Activations are NHWC fp32 and the output-pixel dimension M = N*Ho*Wo is FLATTENED ACROSS IMAGES and predicated at its
// tail (the maps are 112^2 ... 7^2: 49 pixels per image are no multiple of any tile).  Every convolution of the network
// -- 38 1x1 GEMMs, 16 3x3 (13 stride 1, 3 stride 2) and the 7x7 stride-2 stem -- runs on ONE kernel:
//
//   igemm32::conv_kernel<HmrVec> (Cin % 4 == 0) / <HmrScalar> (the stem): the implicit GEMM of igemm32.h on
//   v_mfma_f32_32x32x2_f32, shared with lpips.hip and inception.hip; this file states what is HMR's own, as the policy
//   struct HmrConv.  Optional PROLOGUE on the gathered input: per-input-channel max(x*scale + shift, 0)
//   (bn1 + ReLU in front of conv1 and of the shortcut conv; padding taps stay 0, as torch pads the activated tensor).
//   Optional EPILOGUE: + bias, per-output-channel max(v*scale + shift, 0) (bn2 / bn3 + ReLU), + residual read at
//   (oh*rs, ow*rs) of an NHWC tensor (conv3 + shortcut; rs = 2 is the reference's subsample = max_pool2d([1,1], stride 2)).
//
// The reduction order of an output element is (tap, input channel) ascending, whatever its position in M, the batch size
// or max_batch: rows of a batch are bit-identical to the same image run alone.
// One stream, no host synchronisation and no allocation in forward: capturable as a single chain.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "igemm32.h"
#include "maxpool.h"

namespace lwg {
namespace {

// every convolution of the network: NHWC in, NHWC out.  The prologue and the epilogue of the file header, as a policy of
// igemm32::conv_kernel; HmrVec and HmrScalar add the gather
struct HmrConv {
    igemm32::Geom g;
    const float *x;          // (N,H,W,Cin) NHWC
    const float *pre_scale, *pre_shift;     // (Cin) or NULL
    const float *bias;                      // (Cout) or NULL
    const float *post_scale, *post_shift;   // (Cout) or NULL
    const float *res;                       // (N,res_H,res_W,Cout) or NULL
    float *y;                // (N,Ho,Wo,Cout)
    int res_stride, res_H, res_W;
    static constexpr bool kCoutTail = false;

    struct Col {
        float bias, ps, pb;
    };
    __device__ Col column(int co) const
    {
        return Col{bias ? bias[co] : 0.f, post_scale ? post_scale[co] : 1.f, post_scale ? post_shift[co] : 0.f};
    }
    __device__ void write(long m, int co, const Col &c, float v) const
    {
        if (bias) v += c.bias;
        if (post_scale) v = fmaxf(fmaf(v, c.ps, c.pb), 0.f);
        if (res) {
            const int n = (int)(m / ((long)g.Ho * g.Wo));
            const int rem = (int)(m - (long)n * g.Ho * g.Wo);
            const int oh = rem / g.Wo, ow = rem - oh * g.Wo;
            v += res[(((size_t)n * res_H + (size_t)oh * res_stride) * res_W + (size_t)ow * res_stride) * g.Cout + co];
        }
        y[(size_t)m * g.Cout + co] = v;
    }
};

// Cin % 4 == 0, so four consecutive reduction indices are one 16-byte load inside one tap
struct HmrVec : HmrConv {
    __device__ float4 gather(const igemm32::Row &r, int kg) const
    {
        return igemm32::gather_nhwc4(g, x, r, kg, [&](float4 val, int c) {
            if (pre_scale) {
                const float4 s = *reinterpret_cast<const float4 *>(pre_scale + c);
                const float4 b = *reinterpret_cast<const float4 *>(pre_shift + c);
                val.x = fmaxf(fmaf(val.x, s.x, b.x), 0.f);
                val.y = fmaxf(fmaf(val.y, s.y, b.y), 0.f);
                val.z = fmaxf(fmaf(val.z, s.z, b.z), 0.f);
                val.w = fmaxf(fmaf(val.w, s.w, b.w), 0.f);
            }
            return val;
        });
    }
};

// any Cin (the 3-channel stem): one input value at a time, activated
struct HmrScalar : HmrConv {
    __device__ float4 gather(const igemm32::Row &r, int kg) const
    {
        return igemm32::gather_each(g, r, kg, g.Cin, [&](int c, int ih, int iw) {
            float val = *igemm32::nhwc_at(g, x, r, c, ih, iw);
            if (pre_scale) val = fmaxf(fmaf(val, pre_scale[c], pre_shift[c]), 0.f);
            return val;
        });
    }
};

// (N,C,H,W) -> (N,H,W,C), C small (the 3-channel image in front of the stem)
__global__ __launch_bounds__(256) void hmr_nhwc_kernel(const float *__restrict__ x, int C, long HW, long total, float *__restrict__ y)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // over N*HW*C, output order
    if (i >= total) return;
    const int c = (int)(i % C);
    const long px = i / C;
    const long n = px / HW, hw = px - n * HW;
    y[i] = x[(n * C + c) * HW + hw];
}

// relu(post_bn(x)) -> average over the HW pixels of an image: x (N,HW,C) -> out (N,C); pixels summed in ascending order
__global__ __launch_bounds__(256) void hmr_pool_kernel(const float *__restrict__ x, int HW, int C, long total,
                                                      const float *__restrict__ scale, const float *__restrict__ shift,
                                                      float *__restrict__ out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // over N*C
    if (i >= total) return;
    const int c = (int)(i % C);
    const long n = i / C;
    const float s = scale[c], b = shift[c];
    const float *px = x + n * HW * C + c;
    float sum = 0.f;
    for (int q = 0; q < HW; ++q) sum += fmaxf(fmaf(px[(size_t)q * C], s, b), 0.f);
    out[i] = sum / (float)HW;
}

__global__ __launch_bounds__(256) void hmr_theta_init_kernel(const float *__restrict__ mean, int D, int total, float *__restrict__ theta)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) theta[i] = mean[i % D];
}

// Linear layer for up to 8 rows at once, one wave per output: out[n][j] = act(b[j] + sum_k W[j][k] * [x0[n], x1[n]][k]) (+ add[n][j]).
// Each lane sums k = lane, lane + 64, ... in ascending order, then a fixed butterfly: the same arithmetic for every row count.
constexpr int FC_ROWS = 8;
__global__ __launch_bounds__(256) void hmr_fc_kernel(const float *__restrict__ Wt, const float *__restrict__ b,
                                                    const float *__restrict__ x0, int K0, const float *__restrict__ x1, int K1,
                                                    int rows, int out_dim, int relu, const float *add, float *out)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= out_dim) return;
    const int K = K0 + K1;
    const float *wr = Wt + (size_t)j * K;
    float acc[FC_ROWS];
#pragma unroll
    for (int n = 0; n < FC_ROWS; ++n) acc[n] = 0.f;
    for (int k = lane; k < K0; k += 64) {
        const float w = wr[k];
#pragma unroll
        for (int n = 0; n < FC_ROWS; ++n)
            if (n < rows) acc[n] = fmaf(w, x0[(size_t)n * K0 + k], acc[n]);
    }
    for (int k = lane; k < K1; k += 64) {
        const float w = wr[K0 + k];
#pragma unroll
        for (int n = 0; n < FC_ROWS; ++n)
            if (n < rows) acc[n] = fmaf(w, x1[(size_t)n * K1 + k], acc[n]);
    }
#pragma unroll
    for (int n = 0; n < FC_ROWS; ++n) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[n] += __shfl_xor(acc[n], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < FC_ROWS; ++n) {
            if (n >= rows) continue;
            float v = acc[n] + b[j];
            if (relu) v = fmaxf(v, 0.f);
            if (add) v += add[(size_t)n * out_dim + j];
            out[(size_t)n * out_dim + j] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool conv_geometry_ok(int k, int stride, int pad)
{
    return (k == 1 && stride == 1 && pad == 0) || (k == 3 && stride == 1 && pad == 1) || (k == 3 && stride == 2 && pad == 1) ||
           (k == 7 && stride == 2 && pad == 3);
}

int launch_conv(const HmrConv &p, hipStream_t st)
{
    if (p.g.Cin % 4 == 0) return igemm32::launch(HmrVec{p}, "igemm32::conv_kernel<HmrVec>", st);
    return igemm32::launch(HmrScalar{p}, "igemm32::conv_kernel<HmrScalar>", st);
}

// max_pool2d(3, 2, ceil_mode=True): taps outside the input are ignored
int launch_ceil_maxpool(const float *x, int N, int H, int W, int C, float *y, hipStream_t st)
{
    return launch_maxpool(x, N, H, W, C, pool_out_ceil(H), pool_out_ceil(W), y, C, 0, st);
}

int launch_pool(const float *x, int N, int HW, int C, const float *scale, const float *shift, float *out, hipStream_t st)
{
    const long total = (long)N * C;
    hmr_pool_kernel<<<ceil_div(total, 256), 256, 0, st>>>(x, HW, C, total, scale, shift, out);
    LWG_LAUNCH_CHECK("hmr_pool_kernel");
    return LWG_OK;
}

struct FcWeights {
    const float *mean_theta, *w1, *b1, *w2, *b2, *w3, *b3;
};

// ThetaRegressor.forward (hmr.py:239-252), dropout = identity: rows <= FC_ROWS.  h1, h2: (rows, hidden) scratch.
int launch_regress(const float *feat, int rows, int feat_dim, int theta_dim, int hidden, int iterations, const FcWeights &f,
                   float *h1, float *h2, float *theta, hipStream_t st)
{
    hmr_theta_init_kernel<<<ceil_div(rows * theta_dim, 256), 256, 0, st>>>(f.mean_theta, theta_dim, rows * theta_dim, theta);
    LWG_LAUNCH_CHECK("hmr_theta_init_kernel");
    for (int it = 0; it < iterations; ++it) {
        hmr_fc_kernel<<<ceil_div(hidden, 4), 256, 0, st>>>(f.w1, f.b1, feat, feat_dim, theta, theta_dim, rows, hidden, 1, nullptr, h1);
        hmr_fc_kernel<<<ceil_div(hidden, 4), 256, 0, st>>>(f.w2, f.b2, h1, hidden, nullptr, 0, rows, hidden, 1, nullptr, h2);
        // theta += fc3(h2): every element is read and written by the one lane that owns it
        hmr_fc_kernel<<<ceil_div(theta_dim, 4), 256, 0, st>>>(f.w3, f.b3, h2, hidden, nullptr, 0, rows, theta_dim, 0, theta, theta);
        LWG_LAUNCH_CHECK("hmr_fc_kernel");
    }
    return LWG_OK;
}

constexpr int kImage = 224, kFeat = 2048, kTheta = 85, kHidden = 1024, kIterations = 3;

struct ConvOp {
    int src, dst, res;            // buffer roles; res = -1: none
    int H, W, Cin, Cout, ks, stride, pad, res_stride, res_H, res_W;
    long w, pre, bias, post;      // blob offsets in floats (-1: absent); pre / post: scale, the shift follows it
};

}  // namespace
}  // namespace lwg

using namespace lwg;

// buffer roles of the forward pass
enum { HB_IMG = 0, HB_STEM, HB_X0, HB_X1, HB_SC, HB_T1, HB_T2, HB_COUNT };

struct lwg_hmr {
    int max_batch = 0, num_blocks[4] = {0, 0, 0, 0};
    std::vector<ConvOp> ops;          // stem first, then the blocks' convs in launch order
    long post_bn = 0, fc = 0;         // blob offsets
    size_t blob_floats = 0;
    size_t buf_floats[HB_COUNT] = {0};   // per image
    float *blob = nullptr, *buf[HB_COUNT] = {nullptr};
    float *feat = nullptr, *h1 = nullptr, *h2 = nullptr, *theta = nullptr;
    int final_buf = HB_X0, final_hw = 0;
    bool ready = false;
};

namespace {

// The blob layout -- what impersonator_amd/networks/hmr.py::pack_weights writes, in this order:
//   stem w (7*7*3, 64) | stem bias
//   per block: bn1 scale, shift (Cin) | conv1 w (Cin, p) | bn2 scale, shift (p) | conv2 w (9*p, p) | bn3 scale, shift (p)
//              | conv3 w (p, 4p) | conv3 bias | [shortcut w (Cin, 4p) | shortcut bias]
//   post_bn scale, shift (2048) | mean_theta (85) | fc1 w (1024, 2133), b | fc2 w (1024, 1024), b | fc3 w (85, 1024), b
void build_plan(lwg_hmr *h)
{
    long off = 0;
    auto take = [&](long n) { const long o = off; off += n; return o; };
    auto need = [&](int role, size_t n) { if (h->buf_floats[role] < n) h->buf_floats[role] = n; };
    need(HB_IMG, (size_t)3 * kImage * kImage);
    ConvOp stem = {HB_IMG, HB_STEM, -1, kImage, kImage, 3, 64, 7, 2, 3, 0, 0, 0, -1, -1, -1, -1};
    stem.w = take(49 * 3 * 64);
    stem.bias = take(64);
    h->ops.push_back(stem);
    int H = kImage / 2;                                   // 112
    need(HB_STEM, (size_t)H * H * 64);
    H = pool_out_ceil(H);                                 // 56
    need(HB_X0, (size_t)H * H * 64);
    int cur = HB_X0, Cin = 64;
    const int planes[4] = {64, 128, 256, 512}, layer_stride[4] = {2, 2, 2, 1};
    for (int L = 0; L < 4; ++L) {
        const int p = planes[L];
        for (int i = 0; i < h->num_blocks[L]; ++i) {
            const int s = (i > 0 && i == h->num_blocks[L] - 1) ? layer_stride[L] : 1;   // hmr.py:140-147
            const int Ho = igemm32::conv_out(H, 3, s, 1);
            const bool shortcut = Cin != 4 * p;
            const int nxt = cur == HB_X0 ? HB_X1 : HB_X0;
            const long bn1 = take(2L * Cin);
            ConvOp c1 = {cur, HB_T1, -1, H, H, Cin, p, 1, 1, 0, 0, 0, 0, take((long)Cin * p), bn1, -1, -1};
            c1.post = take(2L * p);
            ConvOp c2 = {HB_T1, HB_T2, -1, H, H, p, p, 3, s, 1, 0, 0, 0, take(9L * p * p), -1, -1, -1};
            c2.post = take(2L * p);
            ConvOp c3 = {HB_T2, nxt, shortcut ? HB_SC : cur, Ho, Ho, p, 4 * p, 1, 1, 0, shortcut ? 1 : s, shortcut ? Ho : H,
                         shortcut ? Ho : H, take((long)p * 4 * p), -1, -1, -1};
            c3.bias = take(4L * p);
            if (shortcut) {
                ConvOp sc = {cur, HB_SC, -1, H, H, Cin, 4 * p, 1, 1, 0, 0, 0, 0, take((long)Cin * 4 * p), bn1, -1, -1};
                sc.bias = take(4L * p);
                h->ops.push_back(sc);
                need(HB_SC, (size_t)H * H * 4 * p);
            }
            h->ops.push_back(c1);
            h->ops.push_back(c2);
            h->ops.push_back(c3);
            need(HB_T1, (size_t)H * H * p);
            need(HB_T2, (size_t)Ho * Ho * p);
            need(nxt, (size_t)Ho * Ho * 4 * p);
            cur = nxt;
            H = Ho;
            Cin = 4 * p;
        }
    }
    h->final_buf = cur;
    h->final_hw = H * H;
    h->post_bn = take(2L * kFeat);
    h->fc = take(kTheta + (long)kHidden * (kFeat + kTheta) + kHidden + (long)kHidden * kHidden + kHidden + (long)kTheta * kHidden + kTheta);
    h->blob_floats = (size_t)off;
}

FcWeights fc_weights(const float *base)
{
    FcWeights f;
    f.mean_theta = base;
    f.w1 = f.mean_theta + kTheta;
    f.b1 = f.w1 + (size_t)kHidden * (kFeat + kTheta);
    f.w2 = f.b1 + kHidden;
    f.b2 = f.w2 + (size_t)kHidden * kHidden;
    f.w3 = f.b2 + kHidden;
    f.b3 = f.w3 + (size_t)kTheta * kHidden;
    return f;
}

}  // namespace

extern "C" {

int lwg_hmr_create(lwg_hmr **out, int max_batch, const int *num_blocks)
{
    LWG_REQUIRE(out != nullptr, "lwg_hmr_create: NULL output handle");
    *out = nullptr;
    LWG_REQUIRE(max_batch >= 1 && max_batch <= 1024, "lwg_hmr_create: max_batch %d outside 1..1024", max_batch);
    static const int kDefault[4] = {3, 4, 6, 3};
    const int *nb = num_blocks ? num_blocks : kDefault;
    for (int i = 0; i < 4; ++i) LWG_REQUIRE(nb[i] >= 1 && nb[i] <= 64, "lwg_hmr_create: num_blocks[%d] = %d outside 1..64", i, nb[i]);
    lwg_hmr *h = new lwg_hmr();
    h->max_batch = max_batch;
    for (int i = 0; i < 4; ++i) h->num_blocks[i] = nb[i];
    build_plan(h);
    hipError_t e = alloc_floats(&h->blob, h->blob_floats);
    for (int r = 0; r < HB_COUNT && e == hipSuccess; ++r) e = alloc_floats(&h->buf[r], h->buf_floats[r] * max_batch);
    if (e == hipSuccess) e = alloc_floats(&h->feat, (size_t)max_batch * kFeat);
    if (e == hipSuccess) e = alloc_floats(&h->h1, (size_t)max_batch * kHidden);
    if (e == hipSuccess) e = alloc_floats(&h->h2, (size_t)max_batch * kHidden);
    if (e == hipSuccess) e = alloc_floats(&h->theta, (size_t)max_batch * kTheta);
    if (e != hipSuccess) {
        lwg_hmr_destroy(h);
        LWG_FAIL(LWG_ERR_HIP, "lwg_hmr_create: hipMalloc failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return LWG_OK;
}

void lwg_hmr_destroy(lwg_hmr *h)
{
    if (!h) return;
    free_device(h->blob);
    for (int r = 0; r < HB_COUNT; ++r) free_device(h->buf[r]);
    free_device(h->feat); free_device(h->h1); free_device(h->h2); free_device(h->theta);
    delete h;
}

size_t lwg_hmr_weight_floats(const lwg_hmr *h) { return h ? h->blob_floats : 0; }

int lwg_hmr_set_weights(lwg_hmr *h, const float *blob_host, size_t n_floats)
{
    LWG_REQUIRE(h != nullptr, "lwg_hmr_set_weights: NULL handle");
    LWG_REQUIRE(blob_host != nullptr, "lwg_hmr_set_weights: NULL blob");
    LWG_REQUIRE(n_floats == h->blob_floats, "lwg_hmr_set_weights: blob of %zu floats, this network takes %zu", n_floats, h->blob_floats);
    return upload_blob(h->blob, blob_host, n_floats, h->ready);
}

int lwg_hmr_forward(lwg_hmr *h, const float *images, int n, int height, int width, float *theta_out, float *features_out,
                    lwg_stream_t stream)
{
    LWG_REQUIRE(h != nullptr, "lwg_hmr_forward: NULL handle");
    LWG_REQUIRE(images != nullptr && theta_out != nullptr, "lwg_hmr_forward: NULL images or theta_out");
    LWG_REQUIRE(n >= 1, "lwg_hmr_forward: n = %d", n);
    if (height != kImage || width != kImage)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_forward: images are %d x %d, the regressor takes %d x %d", height, width, kImage, kImage);
    if (n > h->max_batch) LWG_FAIL(LWG_ERR_STATE, "lwg_hmr_forward: n = %d above max_batch = %d", n, h->max_batch);
    if (!h->ready) LWG_FAIL(LWG_ERR_STATE, "lwg_hmr_forward: no weights set");
    hipStream_t st = as_stream(stream);
    const long total = (long)n * 3 * kImage * kImage;
    hmr_nhwc_kernel<<<ceil_div(total, 256), 256, 0, st>>>(images, 3, (long)kImage * kImage, total, h->buf[HB_IMG]);
    LWG_LAUNCH_CHECK("hmr_nhwc_kernel");
    for (size_t i = 0; i < h->ops.size(); ++i) {
        const ConvOp &o = h->ops[i];
        HmrConv p;
        memset(&p, 0, sizeof(p));
        p.g = igemm32::geom(h->blob + o.w, n, o.H, o.W, o.Cin, o.Cout, o.ks, o.ks, o.stride, o.pad, o.pad);
        p.x = h->buf[o.src];
        p.y = h->buf[o.dst];
        if (o.pre >= 0) { p.pre_scale = h->blob + o.pre; p.pre_shift = p.pre_scale + o.Cin; }
        if (o.bias >= 0) p.bias = h->blob + o.bias;
        if (o.post >= 0) { p.post_scale = h->blob + o.post; p.post_shift = p.post_scale + o.Cout; }
        if (o.res >= 0) { p.res = h->buf[o.res]; p.res_stride = o.res_stride; p.res_H = o.res_H; p.res_W = o.res_W; }
        const int rc = launch_conv(p, st);
        if (rc != LWG_OK) return rc;
        if (i == 0) {
            const int rc2 = launch_ceil_maxpool(h->buf[HB_STEM], n, kImage / 2, kImage / 2, 64, h->buf[HB_X0], st);
            if (rc2 != LWG_OK) return rc2;
        }
    }
    float *feat = features_out ? features_out : h->feat;
    int rc = launch_pool(h->buf[h->final_buf], n, h->final_hw, kFeat, h->blob + h->post_bn, h->blob + h->post_bn + kFeat, feat, st);
    if (rc != LWG_OK) return rc;
    const FcWeights f = fc_weights(h->blob + h->fc);
    for (int r0 = 0; r0 < n; r0 += FC_ROWS) {
        const int rows = n - r0 < FC_ROWS ? n - r0 : FC_ROWS;
        rc = launch_regress(feat + (size_t)r0 * kFeat, rows, kFeat, kTheta, kHidden, kIterations, f, h->h1 + (size_t)r0 * kHidden,
                            h->h2 + (size_t)r0 * kHidden, theta_out + (size_t)r0 * kTheta, st);
        if (rc != LWG_OK) return rc;
    }
    return LWG_OK;
}

int lwg_hmr_conv(const float *x, int N, int H, int W, int Cin, const float *w, int Cout, int k, int stride, int pad,
                 const float *pre_scale, const float *pre_shift, const float *bias, const float *post_scale,
                 const float *post_shift, const float *residual, int res_stride, int res_H, int res_W, float *y,
                 lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "lwg_hmr_conv: NULL x, w or y");
    LWG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "lwg_hmr_conv: non-positive size");
    // 16-byte accesses: the weight rows always, the input and the prologue vectors when Cin is a multiple of 4
    LWG_REQUIRE(igemm32::aligned16(w), "lwg_hmr_conv: w is not 16-byte aligned");
    LWG_REQUIRE(Cin % 4 != 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pre_scale) |
                                  reinterpret_cast<uintptr_t>(pre_shift)) & 15) == 0,
                "lwg_hmr_conv: x / pre_scale / pre_shift are not 16-byte aligned");
    LWG_REQUIRE((pre_scale == nullptr) == (pre_shift == nullptr), "lwg_hmr_conv: the prologue needs both scale and shift (one is NULL)");
    LWG_REQUIRE((post_scale == nullptr) == (post_shift == nullptr), "lwg_hmr_conv: the epilogue needs both scale and shift (one is NULL)");
    if (!conv_geometry_ok(k, stride, pad))
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_conv: (k, stride, pad) = (%d, %d, %d) is none of (1,1,0) (3,1,1) (3,2,1) (7,2,3)", k, stride, pad);
    if (Cout % igemm32::BN != 0) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_conv: Cout = %d is no multiple of %d", Cout, igemm32::BN);
    if (igemm32::too_large(N, H, W, Cin > Cout ? Cin : Cout)) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_conv: tensor too large");
    const int Ho = igemm32::conv_out(H, k, stride, pad), Wo = igemm32::conv_out(W, k, stride, pad);
    LWG_REQUIRE(Ho >= 1 && Wo >= 1, "lwg_hmr_conv: empty output");
    if (residual) {
        LWG_REQUIRE(res_stride >= 1 && res_H >= 1 && res_W >= 1, "lwg_hmr_conv: residual stride / size not positive");
        LWG_REQUIRE((long)(Ho - 1) * res_stride < res_H && (long)(Wo - 1) * res_stride < res_W,
                    "lwg_hmr_conv: a %d x %d residual read with stride %d does not cover the %d x %d output", res_H, res_W, res_stride, Ho, Wo);
    }
    HmrConv p;
    memset(&p, 0, sizeof(p));
    p.g = igemm32::geom(w, N, H, W, Cin, Cout, k, k, stride, pad, pad);
    p.x = x; p.y = y;
    p.pre_scale = pre_scale; p.pre_shift = pre_shift; p.bias = bias; p.post_scale = post_scale; p.post_shift = post_shift;
    p.res = residual; p.res_stride = res_stride; p.res_H = res_H; p.res_W = res_W;
    return launch_conv(p, as_stream(stream));
}

int lwg_hmr_maxpool(const float *x, int N, int H, int W, int C, float *y, lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && y != nullptr, "lwg_hmr_maxpool: NULL x or y");
    LWG_REQUIRE(N >= 1 && H >= 3 && W >= 3 && C >= 1, "lwg_hmr_maxpool: needs N, C >= 1 and H, W >= 3");
    if (C % 4 != 0) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_maxpool: C = %d is no multiple of 4", C);
    LWG_REQUIRE(igemm32::aligned16(x) && igemm32::aligned16(y), "lwg_hmr_maxpool: x / y are not 16-byte aligned");
    return launch_ceil_maxpool(x, N, H, W, C, y, as_stream(stream));
}

int lwg_hmr_pool_features(const float *x, int N, int HW, int C, const float *scale, const float *shift, float *out,
                          lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && scale != nullptr && shift != nullptr && out != nullptr, "lwg_hmr_pool_features: NULL pointer");
    LWG_REQUIRE(N >= 1 && HW >= 1 && C >= 1, "lwg_hmr_pool_features: non-positive size");
    return launch_pool(x, N, HW, C, scale, shift, out, as_stream(stream));
}

size_t lwg_hmr_regress_workspace_bytes(int N) { return N >= 1 ? (size_t)N * 2 * kHidden * sizeof(float) : 0; }

int lwg_hmr_regress(const float *features, int N, const float *mean_theta, const float *fc1_w, const float *fc1_b,
                    const float *fc2_w, const float *fc2_b, const float *fc3_w, const float *fc3_b, float *theta_out,
                    void *workspace, size_t workspace_bytes, lwg_stream_t stream)
{
    LWG_REQUIRE(features != nullptr && theta_out != nullptr, "lwg_hmr_regress: NULL features or theta_out");
    LWG_REQUIRE(mean_theta && fc1_w && fc1_b && fc2_w && fc2_b && fc3_w && fc3_b, "lwg_hmr_regress: NULL weight pointer");
    LWG_REQUIRE(N >= 1, "lwg_hmr_regress: N = %d", N);
    LWG_REQUIRE(workspace != nullptr, "lwg_hmr_regress: NULL workspace");
    if (workspace_bytes < lwg_hmr_regress_workspace_bytes(N) || (reinterpret_cast<uintptr_t>(workspace) & 3))
        LWG_FAIL(LWG_ERR_WORKSPACE, "lwg_hmr_regress: workspace of %zu bytes, needs %zu (4-byte aligned)", workspace_bytes,
                 lwg_hmr_regress_workspace_bytes(N));
    FcWeights f = {mean_theta, fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b};
    float *h1 = static_cast<float *>(workspace), *h2 = h1 + (size_t)N * kHidden;
    for (int r0 = 0; r0 < N; r0 += FC_ROWS) {
        const int rows = N - r0 < FC_ROWS ? N - r0 : FC_ROWS;
        const int rc = launch_regress(features + (size_t)r0 * kFeat, rows, kFeat, kTheta, kHidden, kIterations, f,
                                      h1 + (size_t)r0 * kHidden, h2 + (size_t)r0 * kHidden, theta_out + (size_t)r0 * kTheta,
                                      as_stream(stream));
        if (rc != LWG_OK) return rc;
    }
    return LWG_OK;
}

}  // extern "C"
