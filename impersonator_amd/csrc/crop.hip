// crop.hip -- box crop + bilinear resize back to full size, and its adjoint (gfx950).
//
// Replaces GlobalLocalDiscriminator.crop_body (networks/discriminator.py:80-96 of the reference):
//   x[i, :, min_y:max_y, min_x:max_x]  ->  F.interpolate(size=(S,S), mode='bilinear', align_corners=True)
// with the boxes read on the device, so that nothing about a batch's boxes is baked into the launch (no host read, no
// synchronisation, no allocation: the calls can be captured in a graph and replayed with other boxes).
//
// Per axis, PyTorch's align-corners arithmetic: scale = (in-1)/(S-1) (0 when in == 1), src = scale*dst, i0 = floor(src),
// lambda = src - i0, i1 = i0 + (i0 < in-1).  Built without fp contraction: the forward keeps torch's expression order.
#include "common.h"

namespace lwg {
namespace {

struct Box { int x0, y0, w, h; };   // clamped to the image; w <= 0 or h <= 0: empty

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// boxes: (n,4) int64 (min_x, max_x, min_y, max_y), exclusive ends; every coordinate is clamped to [0,S] before use
__device__ __forceinline__ Box load_box(const long long *__restrict__ boxes, int b, int S)
{
    const long long *p = boxes + (size_t)b * 4;
    const int x0 = clampi(p[0], 0, S), x1 = clampi(p[1], 0, S), y0 = clampi(p[2], 0, S), y1 = clampi(p[3], 0, S);
    return Box{x0, y0, x1 - x0, y1 - y0};
}

__device__ __forceinline__ float axis_scale(int in, int S) { return S > 1 ? (float)(in - 1) / (float)(S - 1) : 0.f; }

// the two taps of output coordinate `dst` on an axis of `in` source pixels: i0, i1 in [0, in), weights (1-l, l)
__device__ __forceinline__ void axis_taps(float scale, int dst, int in, int &i0, int &i1, float &l)
{
    const float src = scale * (float)dst;
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

// forward: one lane per V consecutive outputs of a row (V = 4: one 16-byte store; V = 1: any S)
template <int V>
__global__ __launch_bounds__(256) void crop_resize_kernel(const float *__restrict__ x, int C, int S,
                                                          const long long *__restrict__ boxes, long total,
                                                          float *__restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int SV = S / V;
    const int xq = (int)(i % SV), y = (int)((i / SV) % S);
    const long plane = i / ((long)SV * S);
    const Box bx = load_box(boxes, (int)(plane / C), S);
    float r[V];
    if (bx.w <= 0 || bx.h <= 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] = 0.f;
    } else {
        int y0, y1;
        float ly;
        axis_taps(axis_scale(bx.h, S), y, bx.h, y0, y1, ly);
        const float *r0 = x + plane * S * S + (size_t)(bx.y0 + y0) * S + bx.x0;
        const float *r1 = x + plane * S * S + (size_t)(bx.y0 + y1) * S + bx.x0;
        const float sx = axis_scale(bx.w, S), hy = 1.f - ly;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            int x0, x1;
            float lx;
            axis_taps(sx, xq * V + k, bx.w, x0, x1, lx);
            const float hx = 1.f - lx;
            r[k] = hy * (hx * r0[x0] + lx * r0[x1]) + ly * (hx * r1[x0] + lx * r1[x1]);
        }
    }
    float *o = out + plane * S * S + (size_t)y * S + (size_t)xq * V;
    if (V == 4) {
        *reinterpret_cast<float4 *>(o) = make_float4(r[0], r[1 % V], r[2 % V], r[3 % V]);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = r[k];
    }
}

// The outputs whose footprint can contain source pixel j: src in (j-1, j+1), widened by one on each side against the
// rounding of the division; every candidate is then tested with axis_taps itself, so the weights are the forward's.
__device__ __forceinline__ void axis_range(float scale, int j, int S, int &lo, int &hi)
{
    lo = 0;
    hi = S - 1;
    if (scale > 0.f) {
        lo = max(0, (int)floorf((float)(j - 1) / scale) - 1);
        hi = min(S - 1, (int)ceilf((float)(j + 1) / scale) + 1);
    }
}

constexpr int kCropTX = 16;   // source columns per workgroup

// backward: the exact adjoint, as two gathers with a fixed summation order (no atomics: bit-reproducible).  One workgroup owns
// kCropTX image columns of one (sample, channel) plane, all S rows:
//   pass 1 (resize along x, per output row):  tmp[y][sx]  = sum_x  wx(x, sx) * dy[y][x]      -> LDS, S x kCropTX floats
//   pass 2 (resize along y):                  dx[sy][sx]  = sum_y  wy(y, sy) * tmp[y][sx]
// each a loop over only the outputs that reach the source pixel (about 2/scale of them), so the cost per plane stays at a few
// S^2 multiply-adds whatever the box: a 2x2 box has one busy workgroup summing S terms per pass.  Pixels outside the box are
// written as 0.0 by the workgroup that owns their column strip, so dx needs no clearing.
__global__ __launch_bounds__(256) void crop_resize_backward_kernel(const float *__restrict__ dy, int C, int S,
                                                                   const long long *__restrict__ boxes,
                                                                   float *__restrict__ dx)
{
    extern __shared__ float tmp[];   // [S][kCropTX]
    const int plane = blockIdx.y, c0 = blockIdx.x * kCropTX;
    const Box bx = load_box(boxes, plane / C, S);
    const float *g = dy + (size_t)plane * S * S;
    float *o = dx + (size_t)plane * S * S;
    const int items = S * kCropTX;
    // block-uniform: does this strip meet the box at all?
    const bool live = bx.w > 0 && bx.h > 0 && c0 < bx.x0 + bx.w && c0 + kCropTX > bx.x0;
    if (live) {
        const float sx = axis_scale(bx.w, S);
        for (int it = threadIdx.x; it < items; it += 256) {
            const int tj = it % kCropTX, y = it / kCropTX, j = c0 + tj - bx.x0;
            float acc = 0.f;
            if (j >= 0 && j < bx.w) {
                int lo, hi;
                axis_range(sx, j, S, lo, hi);
                const float *row = g + (size_t)y * S;
                for (int xo = lo; xo <= hi; ++xo) {
                    int i0, i1;
                    float l;
                    axis_taps(sx, xo, bx.w, i0, i1, l);
                    const float v = row[xo];
                    if (i0 == j) acc += (1.f - l) * v;
                    if (i1 == j) acc += l * v;
                }
            }
            tmp[it] = acc;
        }
        __syncthreads();
    }
    const float sy = axis_scale(bx.h, S);
    for (int it = threadIdx.x; it < items; it += 256) {
        const int tj = it % kCropTX, r = it / kCropTX, col = c0 + tj;
        if (col >= S) continue;
        const int j = r - bx.y0;
        float acc = 0.f;
        if (live && j >= 0 && j < bx.h && col >= bx.x0 && col < bx.x0 + bx.w) {
            int lo, hi;
            axis_range(sy, j, S, lo, hi);
            for (int yo = lo; yo <= hi; ++yo) {
                int i0, i1;
                float l;
                axis_taps(sy, yo, bx.h, i0, i1, l);
                const float v = tmp[yo * kCropTX + tj];
                if (i0 == j) acc += (1.f - l) * v;
                if (i1 == j) acc += l * v;
            }
        }
        o[(size_t)r * S + col] = acc;
    }
}

int crop_check(const char *what, const void *a, int n, int C, int S, const void *boxes, const void *b)
{
    LWG_REQUIRE(a && boxes && b, "%s: NULL argument", what);
    LWG_REQUIRE(n > 0 && C > 0 && S > 0, "%s: sizes must be positive (n=%d C=%d S=%d)", what, n, C, S);
    LWG_REQUIRE((long)n * C <= 65535, "%s: n*C = %ld planes exceed 65535", what, (long)n * C);
    LWG_REQUIRE(S <= 1024, "%s: S=%d exceeds 1024", what, S);
    LWG_REQUIRE((uintptr_t)boxes % 8 == 0, "%s: boxes must be 8-byte aligned (int64)", what);
    return LWG_OK;
}

}  // namespace
}  // namespace lwg

using namespace lwg;

extern "C" {

int lwg_crop_resize(const float *x, int n, int C, int S, const int64_t *boxes, float *out, lwg_stream_t stream)
{
    const int rc = crop_check("crop_resize", x, n, C, S, boxes, out);
    if (rc != LWG_OK) return rc;
    const long long *bx = reinterpret_cast<const long long *>(boxes);
    if (S % 4 == 0 && (uintptr_t)out % 16 == 0) {
        const long total = (long)n * C * S * (S / 4);
        crop_resize_kernel<4><<<ceil_div(total, 256), 256, 0, as_stream(stream)>>>(x, C, S, bx, total, out);
    } else {
        const long total = (long)n * C * S * S;
        crop_resize_kernel<1><<<ceil_div(total, 256), 256, 0, as_stream(stream)>>>(x, C, S, bx, total, out);
    }
    LWG_LAUNCH_CHECK("crop_resize_kernel");
    return LWG_OK;
}

int lwg_crop_resize_backward(const float *dy, int n, int C, int S, const int64_t *boxes, float *dx, lwg_stream_t stream)
{
    const int rc = crop_check("crop_resize_backward", dy, n, C, S, boxes, dx);
    if (rc != LWG_OK) return rc;
    const dim3 grid(ceil_div(S, kCropTX), n * C);
    crop_resize_backward_kernel<<<grid, 256, (size_t)S * kCropTX * sizeof(float), as_stream(stream)>>>(
        dy, C, S, reinterpret_cast<const long long *>(boxes), dx);
    LWG_LAUNCH_CHECK("crop_resize_backward_kernel");
    return LWG_OK;
}

}  // extern "C"
