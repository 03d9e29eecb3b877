// pixel.h -- what the evaluator's kernels (eval.hip, lpips.hip, inception.hip) do to a stored pixel before they score it, and the
// source taps of its bilinear resize.  Device code, float32, one rounding per step.
#pragma once
#include <hip/hip_runtime.h>

namespace lwg {

// how a stored value becomes the value that is scored; every step a separately rounded float32 operation (the pragma says so
// whatever the flags of the file that includes this)
//   0: as it is   1: [0,1] -> [-1,1], 2*x - 1   2: [-1,1] through the writer's 8 bits and the loader's way back
__device__ __forceinline__ float map_pixel(float x, int mode)
{
#pragma clang fp contract(off)
    if (mode == 1) {
        const float t = 2.f * x;
        return t - 1.f;
    }
    if (mode == 2) {
        const float a = x + 1.f;
        const float b = a / 2.f;
        const float c = b * 255.f;
        float u = truncf(c);
        u = u > 0.f ? u : 0.f;         // NaN -> 0 as well
        u = u < 255.f ? u : 255.f;
        const float d = u / 255.f;
        const float e = d * 2.f;
        return e - 1.f;
    }
    return x;
}

// ATen's source index of F.interpolate(mode='bilinear', align_corners=False), float32.  scale*(dst+0.5)-0.5 is ONE fused
// multiply-add, stated as such: torch's CPU binaries contract it (measured: with two roundings the result is up to 5.7e-7 from
// F.interpolate on [-1,1] noise, with the fused form 1.2e-7), and so do its device builds.  Everything else rounds per step.
__device__ __forceinline__ void linear_taps(float scale, int dst, int in, int &i0, int &i1, float &w0, float &w1)
{
    const float c = (float)dst + 0.5f;
    float src = fmaf(scale, c, -0.5f);
    src = src > 0.f ? src : 0.f;
    i0 = min((int)src, in - 1);
    i1 = min(i0 + 1, in - 1);
    w1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    w0 = 1.f - w1;
}

}  // namespace lwg
