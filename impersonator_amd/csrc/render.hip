// render.hip -- shading on top of the tile rasteriser: textured SMPL mesh images, silhouettes, per-face texture
// extraction (gfx950).
//
// Serves the textured half of the reference's SMPLRenderer (utils/nmr.py:192-244,295-310,354-388):
//   neural_renderer/lighting.py:33-53                       per-face light              face_light_kernel
//   rasterize_cuda_kernel.cu:188-260 (texture sampling),
//   rasterize.py:190-197 (background), :343 (2x2 average)   shading of a rastered frame  shade_resolve_kernel
//   rasterize.py:184-187, :345                              alpha                        silhouette_resolve_kernel
//   utils/nmr.py:382-388,435-470                            per-face sampling grid       face_sampler_kernel
//   utils/nmr.py:364-380                                    F.grid_sample -> texture cube extract_tex_kernel
// The face-index / weight / depth maps come from raster.hip unchanged (lwg_project_faces, lwg_rasterize_fim_wim at the
// super-sampled size); nothing here writes them.
//
// shade_resolve is a gather: one lane per OUTPUT pixel reads its 1 or 2x2 sub-pixels of fim / wim / depth (20 B each),
// the winning face's three depths, eight texels and light, and writes three floats.  The reference multiplies the whole
// texture tensor by the light first (in place, on a clone); the blend is linear in the texels, so the light multiplies
// the blended colour here and no lit copy of the textures exists.  The maps arrive vertically flipped; sampling is per
// pixel, so the flip of rasterize.py:324 needs no further work, and pooling pairs rows 2y, 2y+1 of the flipped map as
// F.avg_pool2d does after the flip.
//
// Compiled with -ffp-contract=off: extract_tex must give the bits of lwg_grid_sample (same tap code, csrc/sample.h, same
// multiply-then-add per tap), and the sampling keeps the .cu file's expression order.
#include <cstdlib>

#include "common.h"
#include "sample.h"

namespace lwg {
namespace {

struct Light {
    float int_amb, int_dir;
    float amb[3], dir_color[3], direction[3];
};

// one lane per (frame, face); verts are the RAW posed vertices (nmr.py:218 runs before the projection)
__global__ __launch_bounds__(256) void face_light_kernel(const float *__restrict__ verts,
                                                         const int32_t *__restrict__ faces_idx, int bs, int nv, int nf,
                                                         Light L, float *__restrict__ light)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bs * nf) return;
    const int b = i / nf, f = i - b * nf;
    float out[3] = {0.f, 0.f, 0.f};
    if (L.int_amb != 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] += L.int_amb * L.amb[c];
    }
    if (L.int_dir != 0.f) {
        float v[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int vi = faces_idx[f * 3 + k];
            vi = min(max(vi, 0), nv - 1);
            const float *p = verts + ((size_t)b * nv + vi) * 3;
            v[k][0] = p[0];
            v[k][1] = p[1];
            v[k][2] = p[2];
        }
        const float ax = v[0][0] - v[1][0], ay = v[0][1] - v[1][1], az = v[0][2] - v[1][2];   // v10
        const float bx = v[2][0] - v[1][0], by = v[2][1] - v[1][1], bz = v[2][2] - v[1][2];   // v12
        const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const float len = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-5f);                 // F.normalize(eps=1e-5)
        const float cs = fmaxf(((nx / len) * L.direction[0] + (ny / len) * L.direction[1]) + (nz / len) * L.direction[2], 0.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] += L.int_dir * (L.dir_color[c] * cs);
    }
    float *o = light + (size_t)i * 3;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
}

// rasterize_cuda_kernel.cu:227-258 for one covered sub-pixel, times the face's light
__device__ __forceinline__ void sample_texture(const float *__restrict__ face, const float *__restrict__ tex,
                                               const float *__restrict__ lit, const float w[3], float depth, int ts,
                                               float eps, float rgb[3])
{
    float frac[3];
    int cell[3];
    const float hi = (float)(ts - 1) - eps;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float tif = w[k] * (float)(ts - 1) * (depth / face[3 * k + 2]);
        tif = fmaxf(tif, 0.f);
        tif = fminf(tif, hi);
        int c = (int)tif;
        c = min(max(c, 0), ts - 2);   // no-op for finite tif (0 <= tif < ts - 1); keeps the upper texel inside the cube
        cell[k] = c;
        frac[k] = tif - (float)c;
    }
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int pn = 0; pn < 8; ++pn) {
        float wt = 1.f;
        int idx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (((pn >> k) & 1) == 0) {
                wt *= 1.f - frac[k];
                idx[k] = cell[k];
            } else {
                wt *= frac[k];
                idx[k] = cell[k] + 1;
            }
        }
        const int isc = idx[0] * ts * ts + idx[1] * ts + idx[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wt * tex[isc * 3 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = acc[c] * lit[c];
}

// one lane per output pixel; AA = 1: the maps are (2 is)^2 and the 2x2 sub-pixels are averaged
template <int AA>
__global__ __launch_bounds__(256) void shade_resolve_kernel(const float *__restrict__ f2verts,
                                                            const int32_t *__restrict__ fim,
                                                            const float *__restrict__ wim,
                                                            const float *__restrict__ depth,
                                                            const float *__restrict__ textures, int tex_bs,
                                                            const float *__restrict__ light,
                                                            const float *__restrict__ background, int bg_bs, int bs,
                                                            int nf, int is, int ts, float eps, float *__restrict__ rgb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int npix = is * is;
    if (i >= bs * npix) return;
    const int b = i / npix, pn = i - b * npix;
    const int y = pn / is, x = pn - y * is;
    constexpr int kSub = AA ? 2 : 1;
    const int S = is * kSub;
    const size_t cube = (size_t)ts * ts * ts * 3;
    const float *bg = background + (bg_bs > 1 ? b : 0) * 3;
    const float bgc[3] = {bg[0], bg[1], bg[2]};
    float sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < kSub; ++dy) {
#pragma unroll
        for (int dx = 0; dx < kSub; ++dx) {
            const size_t m = ((size_t)b * S + (y * kSub + dy)) * S + (x * kSub + dx);
            const int fn = fim[m];
            float px[3] = {bgc[0], bgc[1], bgc[2]};
            if (fn >= 0 && fn < nf) {
                const float w[3] = {wim[m * 3 + 0], wim[m * 3 + 1], wim[m * 3 + 2]};
                const size_t bf = (size_t)b * nf + fn;
                sample_texture(f2verts + bf * 9, textures + ((size_t)(tex_bs > 1 ? b : 0) * nf + fn) * cube, light + bf * 3, w,
                               depth[m], ts, eps, px);
            }
            sum[0] += px[0];
            sum[1] += px[1];
            sum[2] += px[2];
        }
    }
    float *o = rgb + (size_t)b * 3 * npix + pn;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * npix] = AA ? sum[c] * 0.25f : sum[c];
}

#ifdef LWG_EXPERIMENTS   // measurement only (tools/bench_render.py, profiles/render.md): never in the shipped library
// The other thread mapping of the anti-aliased case: four lanes per output pixel, one sub-pixel each, summed across the quad.
// Selected with LWG_SHADE=quad.  The sum is (s00 + s01) + (s10 + s11): last bits may differ from the one-lane kernel's.
__global__ __launch_bounds__(256) void shade_resolve_quad_kernel(const float *__restrict__ f2verts,
                                                                 const int32_t *__restrict__ fim,
                                                                 const float *__restrict__ wim,
                                                                 const float *__restrict__ depth,
                                                                 const float *__restrict__ textures, int tex_bs,
                                                                 const float *__restrict__ light,
                                                                 const float *__restrict__ background, int bg_bs, int bs,
                                                                 int nf, int is, int ts, float eps, float *__restrict__ rgb)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int npix = is * is;
    const bool live = (t >> 2) < (long)bs * npix;       // dead quads compute pixel 0 again and store nothing
    const int i = live ? (int)(t >> 2) : 0;
    const int sub = (int)(t & 3);
    const int b = i / npix, pn = i - b * npix;
    const int y = pn / is, x = pn - y * is;
    const int S = is * 2;
    const size_t cube = (size_t)ts * ts * ts * 3;
    const float *bg = background + (bg_bs > 1 ? b : 0) * 3;
    const size_t m = ((size_t)b * S + (y * 2 + (sub >> 1))) * S + (x * 2 + (sub & 1));
    const int fn = fim[m];
    float px[3] = {bg[0], bg[1], bg[2]};
    if (fn >= 0 && fn < nf) {
        const float w[3] = {wim[m * 3 + 0], wim[m * 3 + 1], wim[m * 3 + 2]};
        const size_t bf = (size_t)b * nf + fn;
        sample_texture(f2verts + bf * 9, textures + ((size_t)(tex_bs > 1 ? b : 0) * nf + fn) * cube, light + bf * 3, w, depth[m],
                       ts, eps, px);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        px[c] += __shfl_xor(px[c], 1);
        px[c] += __shfl_xor(px[c], 2);
    }
    if (live && sub == 0) {
        float *o = rgb + (size_t)b * 3 * npix + pn;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * npix] = px[c] * 0.25f;
    }
}
#endif

__global__ __launch_bounds__(256) void silhouette_resolve_kernel(const int32_t *__restrict__ fim, int bs, int is, int aa,
                                                                 float *__restrict__ alpha)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int npix = is * is;
    if (i >= bs * npix) return;
    if (!aa) {
        alpha[i] = fim[i] >= 0 ? 1.f : 0.f;
        return;
    }
    const int b = i / npix, pn = i - b * npix;
    const int y = pn / is, x = pn - y * is;
    const int S = 2 * is;
    const int32_t *r0 = fim + ((size_t)b * S + 2 * y) * S + 2 * x;
    const int n = (r0[0] >= 0) + (r0[1] >= 0) + (r0[S] >= 0) + (r0[S + 1] >= 0);
    alpha[i] = (float)n * 0.25f;
}

// one lane per (frame, face, texel row/column pair): the face's three projected points, then the affine combination
__global__ __launch_bounds__(256) void face_sampler_kernel(const float *__restrict__ cam, const float *__restrict__ verts,
                                                           const int32_t *__restrict__ faces_idx,
                                                           const float *__restrict__ coords, int bs, int nv, int nf, int tt,
                                                           float *__restrict__ sampler)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)bs * nf * tt) return;
    const int t = (int)(i % tt);
    const long bf = i / tt;
    const int f = (int)(bf % nf), b = (int)(bf / nf);
    const float s = cam[b * 3 + 0], tx = cam[b * 3 + 1], ty = cam[b * 3 + 2];
    float p[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int vi = faces_idx[f * 3 + k];
        vi = min(max(vi, 0), nv - 1);
        const float *v = verts + ((size_t)b * nv + vi) * 3;
        p[k][0] = s * (v[0] + tx);   // batch_orth_proj_idrot: no y flip
        p[k][1] = s * (v[1] + ty);
    }
    const float c0 = coords[t], c1 = coords[tt + t];
    float o[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float r = ((p[0][d] - p[2][d]) * c0 + (p[1][d] - p[2][d]) * c1) + p[2][d];
        o[d] = fminf(fmaxf(r, -1.f), 1.f);
    }
    *reinterpret_cast<float2 *>(sampler + (size_t)i * 2) = make_float2(o[0], o[1]);
}

// one lane per (frame, face, i, j): the four taps of grid_sample_nchw_kernel (warp.hip), the value repeated along k
__global__ __launch_bounds__(256) void extract_tex_kernel(const float *__restrict__ img, int img_bs, int H, int W,
                                                          const float *__restrict__ sampler, int bs, int nf, int T,
                                                          int align_corners, float *__restrict__ tex)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int tt = T * T;
    if (i >= (long)bs * nf * tt) return;
    const int b = (int)(i / ((long)nf * tt));
    const float2 g = *reinterpret_cast<const float2 *>(sampler + (size_t)i * 2);
    const GridTaps t = grid_taps(g.x, g.y, W, H, align_corners);
    const float *xb = img + (size_t)(img_bs > 1 ? b : 0) * 3 * H * W;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *pl = xb + (size_t)c * H * W;
        float acc = 0.f;
        if (t.vnw) acc += pl[t.y0 * W + t.x0] * t.wnw;
        if (t.vne) acc += pl[t.y0 * W + t.x0 + 1] * t.wne;
        if (t.vsw) acc += pl[(t.y0 + 1) * W + t.x0] * t.wsw;
        if (t.vse) acc += pl[(t.y0 + 1) * W + t.x0 + 1] * t.wse;
        v[c] = acc;
    }
    float *o = tex + (size_t)i * T * 3;   // (b, f, i, j) -> T texels along k
    for (int k = 0; k < T; ++k) {
        o[k * 3 + 0] = v[0];
        o[k * 3 + 1] = v[1];
        o[k * 3 + 2] = v[2];
    }
}

constexpr long kMaxElems = 1l << 30;   // every flat index of these kernels stays below 2^31 floats

}  // namespace
}  // namespace lwg

using namespace lwg;

extern "C" {

int lwg_face_light(const float *verts, const int32_t *faces_idx, int bs, int nv, int nf, float intensity_ambient,
                   float intensity_directional, const float *color_ambient_host, const float *color_directional_host,
                   const float *direction_host, float *light, lwg_stream_t stream)
{
    LWG_REQUIRE(verts && faces_idx && light, "face_light: NULL argument");
    LWG_REQUIRE(color_ambient_host && color_directional_host && direction_host, "face_light: NULL light colour / direction");
    LWG_REQUIRE(bs > 0 && nv > 0 && nf > 0, "face_light: bs/nv/nf must be positive");
    if ((long)bs * nf > kMaxElems / 3 || (long)bs * nv > kMaxElems / 3)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "face_light: problem too large (bs=%d nv=%d nf=%d)", bs, nv, nf);
    Light L;
    L.int_amb = intensity_ambient;
    L.int_dir = intensity_directional;
    for (int c = 0; c < 3; ++c) {
        L.amb[c] = color_ambient_host[c];
        L.dir_color[c] = color_directional_host[c];
        L.direction[c] = direction_host[c];
    }
    face_light_kernel<<<ceil_div((long)bs * nf, 256), 256, 0, as_stream(stream)>>>(verts, faces_idx, bs, nv, nf, L, light);
    LWG_LAUNCH_CHECK("face_light_kernel");
    return LWG_OK;
}

int lwg_shade_resolve(const float *f2verts, const int32_t *fim, const float *wim, const float *depth, const float *textures,
                      int tex_bs, const float *light, const float *background, int bg_bs, int bs, int nf, int image_size,
                      int anti_aliasing, int tex_size, float eps, float *rgb, lwg_stream_t stream)
{
    LWG_REQUIRE(f2verts && fim && wim && depth && textures && light && background && rgb, "shade_resolve: NULL argument");
    LWG_REQUIRE(bs > 0 && nf > 0 && image_size > 0, "shade_resolve: bs/nf/image_size must be positive");
    LWG_REQUIRE(tex_size >= 2, "shade_resolve: tex_size must be at least 2 (got %d): a one-texel cube has no upper cell", tex_size);
    LWG_REQUIRE(tex_bs == 1 || tex_bs == bs, "shade_resolve: texture batch must be 1 or %d (got %d)", bs, tex_bs);
    LWG_REQUIRE(bg_bs == 1 || bg_bs == bs, "shade_resolve: background batch must be 1 or %d (got %d)", bs, bg_bs);
    LWG_REQUIRE(eps >= 0.f && eps < 1.f, "shade_resolve: eps must lie in [0, 1)");
    const long S = (long)image_size * (anti_aliasing ? 2 : 1);
    if (S > 8192 || tex_size > 64 || (long)bs * S * S > kMaxElems / 3 ||
        (long)bs * nf * tex_size * tex_size * tex_size > kMaxElems / 3)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "shade_resolve: problem too large (bs=%d nf=%d is=%d ts=%d)", bs, nf, image_size, tex_size);
    const int blocks = ceil_div((long)bs * image_size * image_size, 256);
#ifdef LWG_EXPERIMENTS
    static const char *shade_env = getenv("LWG_SHADE");   // "quad": four lanes per pixel (A/B switch of the measurement build)
    if (anti_aliasing && shade_env && shade_env[0] == 'q') {
        shade_resolve_quad_kernel<<<ceil_div((long)bs * image_size * image_size * 4, 256), 256, 0, as_stream(stream)>>>(
            f2verts, fim, wim, depth, textures, tex_bs, light, background, bg_bs, bs, nf, image_size, tex_size, eps, rgb);
        LWG_LAUNCH_CHECK("shade_resolve_quad_kernel");
        return LWG_OK;
    }
#endif
    if (anti_aliasing)
        shade_resolve_kernel<1><<<blocks, 256, 0, as_stream(stream)>>>(f2verts, fim, wim, depth, textures, tex_bs, light,
                                                                        background, bg_bs, bs, nf, image_size, tex_size, eps, rgb);
    else
        shade_resolve_kernel<0><<<blocks, 256, 0, as_stream(stream)>>>(f2verts, fim, wim, depth, textures, tex_bs, light,
                                                                        background, bg_bs, bs, nf, image_size, tex_size, eps, rgb);
    LWG_LAUNCH_CHECK("shade_resolve_kernel");
    return LWG_OK;
}

int lwg_silhouette_resolve(const int32_t *fim, int bs, int image_size, int anti_aliasing, float *alpha, lwg_stream_t stream)
{
    LWG_REQUIRE(fim && alpha, "silhouette_resolve: NULL argument");
    LWG_REQUIRE(bs > 0 && image_size > 0, "silhouette_resolve: bs/image_size must be positive");
    const long S = (long)image_size * (anti_aliasing ? 2 : 1);
    if (S > 8192 || (long)bs * S * S > kMaxElems)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "silhouette_resolve: problem too large (bs=%d is=%d)", bs, image_size);
    silhouette_resolve_kernel<<<ceil_div((long)bs * image_size * image_size, 256), 256, 0, as_stream(stream)>>>(
        fim, bs, image_size, anti_aliasing ? 1 : 0, alpha);
    LWG_LAUNCH_CHECK("silhouette_resolve_kernel");
    return LWG_OK;
}

int lwg_face_sampler(const float *cam, const float *verts, const int32_t *faces_idx, const float *coords, int bs, int nv,
                     int nf, int tex_points, float *sampler, lwg_stream_t stream)
{
    LWG_REQUIRE(cam && verts && faces_idx && coords && sampler, "face_sampler: NULL argument");
    LWG_REQUIRE(bs > 0 && nv > 0 && nf > 0 && tex_points > 0, "face_sampler: bs/nv/nf/tex_points must be positive");
    if ((long)bs * nf * tex_points > kMaxElems / 2 || (long)bs * nv > kMaxElems / 3)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "face_sampler: problem too large (bs=%d nf=%d points=%d)", bs, nf, tex_points);
    face_sampler_kernel<<<ceil_div((long)bs * nf * tex_points, 256), 256, 0, as_stream(stream)>>>(cam, verts, faces_idx, coords,
                                                                                                   bs, nv, nf, tex_points, sampler);
    LWG_LAUNCH_CHECK("face_sampler_kernel");
    return LWG_OK;
}

int lwg_extract_tex(const float *uv_img, int img_bs, int H, int W, const float *sampler, int bs, int nf, int tex_size,
                    int align_corners, float *tex, lwg_stream_t stream)
{
    LWG_REQUIRE(uv_img && sampler && tex, "extract_tex: NULL argument");
    LWG_REQUIRE(H > 0 && W > 0 && bs > 0 && nf > 0 && tex_size > 0, "extract_tex: sizes must be positive");
    LWG_REQUIRE(img_bs == 1 || img_bs == bs, "extract_tex: image batch must be 1 or %d (got %d)", bs, img_bs);
    if (tex_size > 64 || (long)H * W > kMaxElems / 3 || (long)img_bs * H * W > kMaxElems / 3 ||
        (long)bs * nf * tex_size * tex_size * tex_size > kMaxElems / 3)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "extract_tex: problem too large (bs=%d nf=%d ts=%d image %dx%d)", bs, nf, tex_size, H, W);
    extract_tex_kernel<<<ceil_div((long)bs * nf * tex_size * tex_size, 256), 256, 0, as_stream(stream)>>>(
        uv_img, img_bs, H, W, sampler, bs, nf, tex_size, align_corners, tex);
    LWG_LAUNCH_CHECK("extract_tex_kernel");
    return LWG_OK;
}

}  // extern "C"
