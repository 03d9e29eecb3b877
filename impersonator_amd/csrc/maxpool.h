// maxpool.h -- max_pool2d(kernel 3, stride 2, no padding) on NHWC fp32, C % 4 == 0, for hmr.hip, lpips.hip and inception.hip.
// One kernel for both rounding modes of the output size: a window is clipped to the input, so with floor-mode sizes (pool_out)
// every tap is inside and with ceil-mode sizes (pool_out_ceil) the taps past the last row and column are ignored, as torch does.
// A maximum is exact and order-free: the result is the same bits either way.
#pragma once
#include "common.h"

namespace lwg {

inline int pool_out(int in) { return in >= 3 ? (in - 3) / 2 + 1 : 0; }
inline int pool_out_ceil(int in) { return in >= 3 ? ceil_div(in - 3, 2) + 1 : 0; }

// pitch4 / off4: the output's channel pitch and offset in float4 units (a branch of a Mixed block writes its slice itself)
static __global__ __launch_bounds__(256) void maxpool3s2_kernel(const float *__restrict__ x, int H, int W, int C4, int Ho, int Wo,
                                                               long total, float *__restrict__ y, int pitch4, int off4)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // over N*Ho*Wo*C4
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const long opx = i / C4;
    long px = opx;
    const int ow = (int)(px % Wo);
    px /= Wo;
    const int oh = (int)(px % Ho);
    const long n = px / Ho;
    const float4 *xs = reinterpret_cast<const float4 *>(x);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ih = oh * 2 + kh, iw = ow * 2 + kw;
            if (ih >= H || iw >= W) continue;
            const float4 v = xs[((n * H + ih) * W + iw) * C4 + c4];
            m.x = fmaxf(m.x, v.x);
            m.y = fmaxf(m.y, v.y);
            m.z = fmaxf(m.z, v.z);
            m.w = fmaxf(m.w, v.w);
        }
    }
    reinterpret_cast<float4 *>(y)[opx * pitch4 + off4 + c4] = m;
}

// x (N,H,W,C) -> channels off .. off + C - 1 of y (N,Ho,Wo,pitch); Ho, Wo from pool_out or pool_out_ceil
static inline int launch_maxpool(const float *x, int N, int H, int W, int C, int Ho, int Wo, float *y, int pitch, int off,
                                 hipStream_t st)
{
    const long total = (long)N * Ho * Wo * (C / 4);
    maxpool3s2_kernel<<<ceil_div(total, 256), 256, 0, st>>>(x, H, W, C / 4, Ho, Wo, total, y, pitch / 4, off / 4);
    LWG_LAUNCH_CHECK("maxpool3s2_kernel");
    return LWG_OK;
}

}  // namespace lwg
