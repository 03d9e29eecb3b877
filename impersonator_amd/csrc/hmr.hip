// hmr.hip -- the HMR image -> SMPL regressor (reference: networks/hmr.py:119-300) in eval mode, exact fp32:
// a pre-activation ResNet-50 (v2), a global average pool and the 3-iteration ThetaRegressor.
//
// Activations are NHWC fp32 and the output-pixel dimension M = N*Ho*Wo is FLATTENED ACROSS IMAGES and predicated at its
// tail (the maps are 112^2 ... 7^2: 49 pixels per image are no multiple of any tile).  Every convolution of the network
// -- 38 1x1 GEMMs, 16 3x3 (13 stride 1, 3 stride 2) and the 7x7 stride-2 stem -- runs on ONE kernel:
//
//   hmr_conv_kernel: implicit GEMM on v_mfma_f32_32x32x2_f32 (bit-for-bit a k-ordered fmaf chain).  Workgroup = 64
//   pixels x 64 output channels, four waves of one 32x32 tile, K = taps x Cin walked 32 at a time through a
//   double-buffered LDS stage.  Optional PROLOGUE on the gathered input: per-input-channel max(x*scale + shift, 0)
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

namespace lwg {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 32;
constexpr int A_PITCH = BK + 1;   // odd pitch: the 32 rows a fragment read touches fall into 32 banks
constexpr int B_PITCH = BN;

struct ConvP {
    const float *x;          // (N,H,W,Cin) NHWC
    const float *w;          // (k*k*Cin, Cout): [tap][ci][co]
    const float *pre_scale, *pre_shift;     // (Cin) or NULL
    const float *bias;                      // (Cout) or NULL
    const float *post_scale, *post_shift;   // (Cout) or NULL
    const float *res;                       // (N,res_H,res_W,Cout) or NULL
    float *y;                // (N,Ho,Wo,Cout)
    int N, H, W, Cin, Cout, ks, stride, pad, Ho, Wo;
    int res_stride, res_H, res_W;
    long M;                  // N*Ho*Wo
    int K;                   // ks*ks*Cin
};

// VEC: Cin % 4 == 0, so four consecutive reduction indices are one 16-byte load inside one tap
template <bool VEC>
__global__ __launch_bounds__(256) void hmr_conv_kernel(const ConvP p)
{
    __shared__ __attribute__((aligned(16))) float sA[2][BM * A_PITCH];
    __shared__ __attribute__((aligned(16))) float sB[2][BK * B_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long m0 = (long)blockIdx.x * BM;
    const int co0 = blockIdx.y * BN;

    // A loader: rows (tid >> 3) and (tid >> 3) + 32, reduction indices (tid & 7) * 4 .. + 3 of the stage
    const int a_col = (tid & 7) * 4;
    int a_n[2], a_ih0[2], a_iw0[2];
    bool a_ok[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const long m = m0 + (tid >> 3) + 32 * v;
        a_ok[v] = m < p.M;
        const long mm = a_ok[v] ? m : 0;
        const int n = (int)(mm / ((long)p.Ho * p.Wo));
        const int rem = (int)(mm - (long)n * p.Ho * p.Wo);
        const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
        a_n[v] = n;
        a_ih0[v] = oh * p.stride - p.pad;
        a_iw0[v] = ow * p.stride - p.pad;
    }
    // B loader: reduction rows (tid >> 4) and (tid >> 4) + 16, output channels (tid & 15) * 4 .. + 3
    const int b_col = (tid & 15) * 4;

    float4 ra[2], rb[2];
    auto gather1 = [&](int v, int kg) -> float {   // one input value, activated; 0 outside the image, past K or past M
        if (!a_ok[v] || kg >= p.K) return 0.f;
        const int tap = kg / p.Cin, c = kg - tap * p.Cin;
        const int kh = tap / p.ks, kw = tap - kh * p.ks;
        const int ih = a_ih0[v] + kh, iw = a_iw0[v] + kw;
        if ((unsigned)ih >= (unsigned)p.H || (unsigned)iw >= (unsigned)p.W) return 0.f;
        float val = p.x[(((size_t)a_n[v] * p.H + ih) * p.W + iw) * p.Cin + c];
        if (p.pre_scale) val = fmaxf(fmaf(val, p.pre_scale[c], p.pre_shift[c]), 0.f);
        return val;
    };
    auto load = [&](int k0) {
        const int kg = k0 + a_col;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (VEC) {
                ra[v] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (a_ok[v] && kg < p.K) {
                    const int tap = kg / p.Cin, c = kg - tap * p.Cin;
                    const int kh = tap / p.ks, kw = tap - kh * p.ks;
                    const int ih = a_ih0[v] + kh, iw = a_iw0[v] + kw;
                    if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) {
                        float4 val = *reinterpret_cast<const float4 *>(p.x + (((size_t)a_n[v] * p.H + ih) * p.W + iw) * p.Cin + c);
                        if (p.pre_scale) {
                            const float4 s = *reinterpret_cast<const float4 *>(p.pre_scale + c);
                            const float4 b = *reinterpret_cast<const float4 *>(p.pre_shift + c);
                            val.x = fmaxf(fmaf(val.x, s.x, b.x), 0.f);
                            val.y = fmaxf(fmaf(val.y, s.y, b.y), 0.f);
                            val.z = fmaxf(fmaf(val.z, s.z, b.z), 0.f);
                            val.w = fmaxf(fmaf(val.w, s.w, b.w), 0.f);
                        }
                        ra[v] = val;
                    }
                }
            } else {
                ra[v] = make_float4(gather1(v, kg), gather1(v, kg + 1), gather1(v, kg + 2), gather1(v, kg + 3));
            }
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int kr = k0 + (tid >> 4) + 16 * v;
            rb[v] = kr < p.K ? *reinterpret_cast<const float4 *>(p.w + (size_t)kr * p.Cout + co0 + b_col)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            float *d = &sA[buf][((tid >> 3) + 32 * v) * A_PITCH + a_col];
            d[0] = ra[v].x;
            d[1] = ra[v].y;
            d[2] = ra[v].z;
            d[3] = ra[v].w;
            *reinterpret_cast<float4 *>(&sB[buf][((tid >> 4) + 16 * v) * B_PITCH + b_col]) = rb[v];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    int buf = 0;
    load(0);
    store(0);
    __syncthreads();
    for (int k0 = 0; k0 < p.K; k0 += BK) {
        const bool more = k0 + BK < p.K;
        if (more) load(k0 + BK);
        // A: lane -> pixel row (lane & 31), k = lane >> 5;  B: lane -> output channel (lane & 31), k = lane >> 5
        const float *ar = &sA[buf][(wm * 32 + (lane & 31)) * A_PITCH + (lane >> 5)];
        const float *br = &sB[buf][(lane >> 5) * B_PITCH + wn * 32 + (lane & 31)];
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[2 * kk], br[2 * kk * B_PITCH], acc, 0, 0, 0);
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // C/D layout: col = lane & 31 -> output channel, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) -> pixel
    const int co = co0 + wn * 32 + (lane & 31);
    const float bias = p.bias ? p.bias[co] : 0.f;
    const float ps = p.post_scale ? p.post_scale[co] : 1.f, pb = p.post_scale ? p.post_shift[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= p.M) continue;
        float v = acc[r];
        if (p.bias) v += bias;
        if (p.post_scale) v = fmaxf(fmaf(v, ps, pb), 0.f);
        if (p.res) {
            const int n = (int)(m / ((long)p.Ho * p.Wo));
            const int rem = (int)(m - (long)n * p.Ho * p.Wo);
            const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
            v += p.res[(((size_t)n * p.res_H + (size_t)oh * p.res_stride) * p.res_W + (size_t)ow * p.res_stride) * p.Cout + co];
        }
        p.y[(size_t)m * p.Cout + co] = v;
    }
}

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

// max_pool2d(kernel 3, stride 2, ceil_mode=True, no padding), NHWC, C % 4 == 0: taps outside the input are ignored
__global__ __launch_bounds__(256) void hmr_maxpool_kernel(const float *__restrict__ x, int H, int W, int C4, int Ho, int Wo,
                                                         long total, float *__restrict__ y)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // over N*Ho*Wo*C4
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    long px = i / C4;
    const int ow = (int)(px % Wo);
    px /= Wo;
    const int oh = (int)(px % Ho);
    const long n = px / Ho;
    const float4 *xs = reinterpret_cast<const float4 *>(x);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh * 2 + kh;
        if (ih >= H) break;
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = ow * 2 + kw;
            if (iw >= W) break;
            const float4 v = xs[((n * H + ih) * W + iw) * C4 + c4];
            m.x = fmaxf(m.x, v.x);
            m.y = fmaxf(m.y, v.y);
            m.z = fmaxf(m.z, v.z);
            m.w = fmaxf(m.w, v.w);
        }
    }
    reinterpret_cast<float4 *>(y)[i] = m;
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

int launch_conv(ConvP p, hipStream_t st)
{
    p.Ho = (p.H + 2 * p.pad - p.ks) / p.stride + 1;
    p.Wo = (p.W + 2 * p.pad - p.ks) / p.stride + 1;
    p.M = (long)p.N * p.Ho * p.Wo;
    p.K = p.ks * p.ks * p.Cin;
    const dim3 grid((unsigned)ceil_div(p.M, BM), (unsigned)(p.Cout / BN));
    if (p.Cin % 4 == 0) hmr_conv_kernel<true><<<grid, 256, 0, st>>>(p);
    else hmr_conv_kernel<false><<<grid, 256, 0, st>>>(p);
    LWG_LAUNCH_CHECK("hmr_conv_kernel");
    return LWG_OK;
}

int launch_maxpool(const float *x, int N, int H, int W, int C, float *y, hipStream_t st)
{
    const int Ho = ceil_div(H - 3, 2) + 1, Wo = ceil_div(W - 3, 2) + 1;
    const long total = (long)N * Ho * Wo * (C / 4);
    hmr_maxpool_kernel<<<ceil_div(total, 256), 256, 0, st>>>(x, H, W, C / 4, Ho, Wo, total, y);
    LWG_LAUNCH_CHECK("hmr_maxpool_kernel");
    return LWG_OK;
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
    H = ceil_div(H - 3, 2) + 1;                           // 56
    need(HB_X0, (size_t)H * H * 64);
    int cur = HB_X0, Cin = 64;
    const int planes[4] = {64, 128, 256, 512}, layer_stride[4] = {2, 2, 2, 1};
    for (int L = 0; L < 4; ++L) {
        const int p = planes[L];
        for (int i = 0; i < h->num_blocks[L]; ++i) {
            const int s = (i > 0 && i == h->num_blocks[L] - 1) ? layer_stride[L] : 1;   // hmr.py:140-147
            const int Ho = (H + 2 - 3) / s + 1;
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
    auto alloc = [&](float **p, size_t n) { return hipMalloc(reinterpret_cast<void **>(p), n * sizeof(float)); };
    hipError_t e = alloc(&h->blob, h->blob_floats);
    for (int r = 0; r < HB_COUNT && e == hipSuccess; ++r) e = alloc(&h->buf[r], h->buf_floats[r] * max_batch);
    if (e == hipSuccess) e = alloc(&h->feat, (size_t)max_batch * kFeat);
    if (e == hipSuccess) e = alloc(&h->h1, (size_t)max_batch * kHidden);
    if (e == hipSuccess) e = alloc(&h->h2, (size_t)max_batch * kHidden);
    if (e == hipSuccess) e = alloc(&h->theta, (size_t)max_batch * kTheta);
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
    auto fr = [](void *p) { if (p) (void)hipFree(p); };
    fr(h->blob);
    for (int r = 0; r < HB_COUNT; ++r) fr(h->buf[r]);
    fr(h->feat); fr(h->h1); fr(h->h2); fr(h->theta);
    delete h;
}

size_t lwg_hmr_weight_floats(const lwg_hmr *h) { return h ? h->blob_floats : 0; }

int lwg_hmr_set_weights(lwg_hmr *h, const float *blob_host, size_t n_floats)
{
    LWG_REQUIRE(h != nullptr, "lwg_hmr_set_weights: NULL handle");
    LWG_REQUIRE(blob_host != nullptr, "lwg_hmr_set_weights: NULL blob");
    LWG_REQUIRE(n_floats == h->blob_floats, "lwg_hmr_set_weights: blob of %zu floats, this network takes %zu", n_floats, h->blob_floats);
    h->ready = false;
    // synchronous: the caller's host buffer may go away after the call, and no forward may overlap the replacement
    LWG_HIP(hipDeviceSynchronize());
    LWG_HIP(hipMemcpy(h->blob, blob_host, n_floats * sizeof(float), hipMemcpyHostToDevice));
    h->ready = true;
    return LWG_OK;
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
        ConvP p;
        memset(&p, 0, sizeof(p));
        p.x = h->buf[o.src];
        p.y = h->buf[o.dst];
        p.w = h->blob + o.w;
        if (o.pre >= 0) { p.pre_scale = h->blob + o.pre; p.pre_shift = p.pre_scale + o.Cin; }
        if (o.bias >= 0) p.bias = h->blob + o.bias;
        if (o.post >= 0) { p.post_scale = h->blob + o.post; p.post_shift = p.post_scale + o.Cout; }
        if (o.res >= 0) { p.res = h->buf[o.res]; p.res_stride = o.res_stride; p.res_H = o.res_H; p.res_W = o.res_W; }
        p.N = n; p.H = o.H; p.W = o.W; p.Cin = o.Cin; p.Cout = o.Cout; p.ks = o.ks; p.stride = o.stride; p.pad = o.pad;
        const int rc = launch_conv(p, st);
        if (rc != LWG_OK) return rc;
        if (i == 0) {
            const int rc2 = launch_maxpool(h->buf[HB_STEM], n, kImage / 2, kImage / 2, 64, h->buf[HB_X0], st);
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
    LWG_REQUIRE((reinterpret_cast<uintptr_t>(w) & 15) == 0, "lwg_hmr_conv: w is not 16-byte aligned");
    LWG_REQUIRE(Cin % 4 != 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pre_scale) |
                                  reinterpret_cast<uintptr_t>(pre_shift)) & 15) == 0,
                "lwg_hmr_conv: x / pre_scale / pre_shift are not 16-byte aligned");
    LWG_REQUIRE((pre_scale == nullptr) == (pre_shift == nullptr), "lwg_hmr_conv: the prologue needs both scale and shift (one is NULL)");
    LWG_REQUIRE((post_scale == nullptr) == (post_shift == nullptr), "lwg_hmr_conv: the epilogue needs both scale and shift (one is NULL)");
    if (!conv_geometry_ok(k, stride, pad))
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_conv: (k, stride, pad) = (%d, %d, %d) is none of (1,1,0) (3,1,1) (3,2,1) (7,2,3)", k, stride, pad);
    if (Cout % lwg::BN != 0) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_conv: Cout = %d is no multiple of %d", Cout, lwg::BN);
    if ((long)N * H * W * (long)(Cin > Cout ? Cin : Cout) >= (1L << 40))
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_conv: tensor too large");
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    LWG_REQUIRE(Ho >= 1 && Wo >= 1, "lwg_hmr_conv: empty output");
    if (residual) {
        LWG_REQUIRE(res_stride >= 1 && res_H >= 1 && res_W >= 1, "lwg_hmr_conv: residual stride / size not positive");
        LWG_REQUIRE((long)(Ho - 1) * res_stride < res_H && (long)(Wo - 1) * res_stride < res_W,
                    "lwg_hmr_conv: a %d x %d residual read with stride %d does not cover the %d x %d output", res_H, res_W, res_stride, Ho, Wo);
    }
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.w = w; p.y = y;
    p.pre_scale = pre_scale; p.pre_shift = pre_shift; p.bias = bias; p.post_scale = post_scale; p.post_shift = post_shift;
    p.res = residual; p.res_stride = res_stride; p.res_H = res_H; p.res_W = res_W;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.ks = k; p.stride = stride; p.pad = pad;
    return launch_conv(p, as_stream(stream));
}

int lwg_hmr_maxpool(const float *x, int N, int H, int W, int C, float *y, lwg_stream_t stream)
{
    LWG_REQUIRE(x != nullptr && y != nullptr, "lwg_hmr_maxpool: NULL x or y");
    LWG_REQUIRE(N >= 1 && H >= 3 && W >= 3 && C >= 1, "lwg_hmr_maxpool: needs N, C >= 1 and H, W >= 3");
    if (C % 4 != 0) LWG_FAIL(LWG_ERR_UNSUPPORTED, "lwg_hmr_maxpool: C = %d is no multiple of 4", C);
    LWG_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0, "lwg_hmr_maxpool: x / y are not 16-byte aligned");
    return launch_maxpool(x, N, H, W, C, y, as_stream(stream));
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
