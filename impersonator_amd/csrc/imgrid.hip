// imgrid.hip -- a batch of images as ONE uint8 picture: torchvision.utils.make_grid + save_image's conversion (gfx950).
//
// The reference's run_view.py:76-85 writes its 16 novel views with `save_image((preds + 1) / 2.0, path)`:
//   make_grid : xmaps = min(nrow, n), ymaps = ceil(n / xmaps); a (H+padding)*ymaps+padding by (W+padding)*xmaps+padding canvas
//               filled with pad_value; image k at row (k / xmaps)*(H+padding)+padding, column (k % xmaps)*(W+padding)+padding;
//               one image alone is returned as it is (no padding);
//   save_image: grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)  -- rounding by +0.5 and truncation.
// Every step is a separately rounded fp32 operation, so the file is built without fp contraction (a fused v*255+0.5 moves
// values that sit on a rounding boundary).  One lane per canvas pixel, three byte stores: a bandwidth kernel of ~1 M pixels.
#include "common.h"

namespace lwg {
namespace {

struct GridShape { int xmaps, ymaps, gh, gw; };

// false: the canvas does not fit 32-bit coordinates
bool grid_shape(int n, int H, int W, int nrow, int padding, GridShape &g)
{
    g.xmaps = nrow < n ? nrow : n;
    g.ymaps = (n + g.xmaps - 1) / g.xmaps;
    long gh = (long)(H + (long)padding) * g.ymaps + padding, gw = (long)(W + (long)padding) * g.xmaps + padding;
    if (n == 1) gh = H, gw = W;   // make_grid returns a single image unchanged
    if (gh > INT32_MAX || gw > INT32_MAX) return false;
    g.gh = (int)gh;
    g.gw = (int)gw;
    return true;
}

__device__ __forceinline__ unsigned char to_u8(float v)
{
    const float s = v * 255.f;
    const float r = s + 0.5f;
    return (unsigned char)fminf(fmaxf(r, 0.f), 255.f);
}

__global__ __launch_bounds__(256) void image_grid_u8_kernel(const float *__restrict__ x, int n, int H, int W, int xmaps, int padding,
                                                            int gw, long total, float pad_value, int normalize,
                                                            unsigned char *__restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int gy = (int)(i / gw), gx = (int)(i - (long)gy * gw);
    int k = 0, iy = gy, ix = gx;
    bool inside = true;
    if (n > 1) {
        const int cy = gy - padding, cx = gx - padding, ph = H + padding, pw = W + padding;
        inside = cy >= 0 && cx >= 0;
        if (inside) {
            const int r = cy / ph, c = cx / pw;
            iy = cy - r * ph;
            ix = cx - c * pw;
            k = r * xmaps + c;
            inside = iy < H && ix < W && c < xmaps && k < n;
        }
    }
    unsigned char *o = out + (size_t)i * 3;
    if (!inside) {
        o[0] = o[1] = o[2] = to_u8(pad_value);
        return;
    }
    const size_t plane = (size_t)H * W;
    const float *p = x + (size_t)k * 3 * plane + (size_t)iy * W + ix;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = p[c * plane];
        if (normalize) v = (v + 1.f) / 2.f;
        o[c] = to_u8(v);
    }
}

int grid_check(const char *what, int n, int H, int W, int nrow, int padding)
{
    LWG_REQUIRE(n > 0 && H > 0 && W > 0 && nrow > 0, "%s: sizes must be positive (n=%d H=%d W=%d nrow=%d)", what, n, H, W, nrow);
    LWG_REQUIRE(padding >= 0, "%s: negative padding %d", what, padding);
    return LWG_OK;
}

}  // namespace
}  // namespace lwg

using namespace lwg;

extern "C" {

int lwg_image_grid_shape(int n, int H, int W, int nrow, int padding, int *grid_h, int *grid_w)
{
    LWG_REQUIRE(grid_h && grid_w, "image_grid_shape: NULL argument");
    const int rc = grid_check("image_grid_shape", n, H, W, nrow, padding);
    if (rc != LWG_OK) return rc;
    GridShape g;
    if (!grid_shape(n, H, W, nrow, padding, g)) LWG_FAIL(LWG_ERR_UNSUPPORTED, "image_grid_shape: the grid exceeds 2^31 pixels a side");
    *grid_h = g.gh;
    *grid_w = g.gw;
    return LWG_OK;
}

int lwg_image_grid_u8(const float *x, int n, int H, int W, int nrow, int padding, float pad_value, int normalize,
                      unsigned char *out, lwg_stream_t stream)
{
    LWG_REQUIRE(x && out, "image_grid_u8: NULL argument");
    const int rc = grid_check("image_grid_u8", n, H, W, nrow, padding);
    if (rc != LWG_OK) return rc;
    GridShape g;
    if (!grid_shape(n, H, W, nrow, padding, g) || (long)g.gh * g.gw > (long)INT32_MAX * 128)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "image_grid_u8: the grid is too large for one launch");
    const long total = (long)g.gh * g.gw;
    image_grid_u8_kernel<<<ceil_div(total, 256), 256, 0, as_stream(stream)>>>(x, n, H, W, g.xmaps, padding, g.gw, total, pad_value,
                                                                              normalize, out);
    LWG_LAUNCH_CHECK("image_grid_u8_kernel");
    return LWG_OK;
}

}  // extern "C"
