// animate.hip -- the per-frame geometry of Animator (appearance transfer driven by a motion sequence) as ONE launch (gfx950).
//
// Given the driven pose's raster maps (fim, wim: lwg_project_faces + lwg_rasterize_fim_wim) and two personalised subjects, a pixel of
// the generator's input is
//     cond      = map_fn[fim]
//     T_ref     = clamp(barycentric flow through the reference's face vertices, -2, 2)     (its kept-part faces sent to -2)
//     T_src     = clamp(barycentric flow through the source's face vertices, -2, 2)        (every other face sent to -2)
//     tsf_img   = grid_sample(ref_img, T_ref) * part_mask + grid_sample(src_img, T_src) * left_mask
//     tsf_inputs= cat(tsf_img, cond)
// which the existing entries compute as encode_fim x2, the two masks, cal_bc_transform x2, clamp x2, grid_sample x2, compose and pack:
// eleven launches and six intermediate tensors per batch.  Here one lane owns one pixel and does all of it from registers.
//
// Exactness: every output is bit-identical to that chain.  The flow is bc_transform_kernel's expression (p0*w0 + p2*w1) + p4*w2, the
// clamp is clamp_kernel's fminf(fmaxf(x, lo), hi), the taps are sample.h's grid_taps accumulated in grid_sample_nchw_kernel's order from
// 0.f, and the composite is swap_compose_kernel's two separately rounded products and their sum; the file is built with
// -ffp-contract=off like those kernels.  part_mask / left_mask are not summed per pixel: part = part_fn[fim], so "the selected (kept)
// channels of the pixel's row sum to non-zero" is a property of the row, and the host hands it over as two bits per row.
//
// A bandwidth kernel: per pixel 16 B of fim/wim in, 16 B of flows, 4 * nc B of cond and 12 B of tsf_img out, the generator's input in
// either layout, two 24-byte face gathers and up to eight image taps per channel from tables and images that stay in L2.  No LDS, no
// atomics, no matrix instructions.
#include "common.h"
#include "sample.h"

namespace lwg {
namespace {

struct AnimateArgs {
    const int32_t *fim;            // (bs, npix)
    const float *wim;              // (bs, npix, 3)
    const float *map_fn;           // (nf + 1, nc)
    const unsigned char *side;     // (nf + 1): bit 0 the row's selected channels sum to non-zero, bit 1 its kept channels do
    const float *src_f2p, *ref_f2p;   // (nf, 3, 2), shared by the batch
    const float *src_img, *ref_img;   // (3, is, is)
    float *T_src, *T_ref;          // (bs, npix, 2)
    float *cond;                   // (bs, nc, npix) or NULL
    float *tsf_img;                // (bs, 3, npix) or NULL
    float *x_nchw;                 // (bs, 3 + nc, npix) or NULL
    float *x_nhwc8;                // (bs, npix, 8) or NULL (nc == 3)
    int bs, nf, is, nc, align_corners;
};

// bc_transform_kernel's expression through one face's (3,2) vertices, then clamp_kernel's clamp
__device__ __forceinline__ float2 clamped_flow(const float *__restrict__ f2p, int fn, float w0, float w1, float w2)
{
    const float2 *p = reinterpret_cast<const float2 *>(f2p + (size_t)fn * 6);
    const float2 a = p[0], b = p[1], c = p[2];
    const float tx = (a.x * w0 + b.x * w1) + c.x * w2;
    const float ty = (a.y * w0 + b.y * w1) + c.y * w2;
    return make_float2(fminf(fmaxf(tx, -2.f), 2.f), fminf(fmaxf(ty, -2.f), 2.f));
}

// grid_sample_nchw_kernel's accumulation on one channel plane
__device__ __forceinline__ float sample_plane(const float *__restrict__ pl, const GridTaps &t, int W)
{
    float acc = 0.f;
    if (t.vnw) acc += pl[t.y0 * W + t.x0] * t.wnw;
    if (t.vne) acc += pl[t.y0 * W + t.x0 + 1] * t.wne;
    if (t.vsw) acc += pl[(t.y0 + 1) * W + t.x0] * t.wsw;
    if (t.vse) acc += pl[(t.y0 + 1) * W + t.x0 + 1] * t.wse;
    return acc;
}

__global__ __launch_bounds__(256) void animate_inputs_kernel(const AnimateArgs a)
{
    const int npix = a.is * a.is;
    const long total = (long)a.bs * npix;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // one pixel of one frame
    if (i >= total) return;
    const int b = (int)(i / npix), pn = (int)(i - (long)b * npix);

    // a rasteriser output is -1 .. nf-1; anything else reads the background row instead of memory it does not own
    const int fn = a.fim[i];
    const bool covered = (unsigned)fn < (unsigned)a.nf;
    const int row = covered ? fn : a.nf;
    const unsigned side = a.side[row];

    float2 ts = make_float2(-2.f, -2.f), tr = ts;   // utils/nmr.py:626; clamp(-2) = -2
    if (covered) {
        const float w0 = a.wim[(size_t)i * 3], w1 = a.wim[(size_t)i * 3 + 1], w2 = a.wim[(size_t)i * 3 + 2];
        ts = clamped_flow(a.src_f2p, fn, w0, w1, w2);
        tr = clamped_flow(a.ref_f2p, fn, w0, w1, w2);
    }
    *reinterpret_cast<float2 *>(a.T_src + (size_t)i * 2) = ts;
    *reinterpret_cast<float2 *>(a.T_ref + (size_t)i * 2) = tr;

    float cnd[3] = {0.f, 0.f, 0.f};
    if (a.cond || a.x_nchw || a.x_nhwc8) {
        for (int c = 0; c < a.nc; ++c) {
            const float m = a.map_fn[(size_t)row * a.nc + c];
            if (c < 3) cnd[c] = m;
            if (a.cond) a.cond[((size_t)b * a.nc + c) * npix + pn] = m;
            if (a.x_nchw) a.x_nchw[((size_t)b * (3 + a.nc) + 3 + c) * npix + pn] = m;
        }
    }
    if (!(a.tsf_img || a.x_nchw || a.x_nhwc8)) return;

    const float part_mask = (side & 1u) ? 1.f : 0.f, left_mask = (side & 2u) ? 1.f : 0.f;
    const GridTaps gr = grid_taps(tr.x, tr.y, a.is, a.is, a.align_corners);
    const GridTaps gs = grid_taps(ts.x, ts.y, a.is, a.is, a.align_corners);
    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float from_ref = sample_plane(a.ref_img + (size_t)c * npix, gr, a.is) * part_mask;
        const float from_src = sample_plane(a.src_img + (size_t)c * npix, gs, a.is) * left_mask;
        rgb[c] = from_ref + from_src;   // two roundings, then the sum (swap_compose_kernel)
        if (a.tsf_img) a.tsf_img[((size_t)b * 3 + c) * npix + pn] = rgb[c];
        if (a.x_nchw) a.x_nchw[((size_t)b * (3 + a.nc) + c) * npix + pn] = rgb[c];
    }
    if (a.x_nhwc8) {
        // [tsf_img(3), cond(3), 0, 0]: the pixel's 32 bytes as two 16-byte stores
        float4 *dst = reinterpret_cast<float4 *>(a.x_nhwc8 + (size_t)i * 8);
        dst[0] = make_float4(rgb[0], rgb[1], rgb[2], cnd[0]);
        dst[1] = make_float4(cnd[1], cnd[2], 0.f, 0.f);
    }
}

}  // namespace
}  // namespace lwg

using namespace lwg;

extern "C" {

int lwg_animate_inputs(const int32_t *fim, const float *wim, int bs, int nf, int image_size, const float *map_fn, int nc,
                       const unsigned char *side, const float *src_f2p, const float *ref_f2p, const float *src_img,
                       const float *ref_img, int align_corners, float *T_src, float *T_ref, float *cond, float *tsf_img,
                       float *tsf_inputs, float *tsf_inputs_nhwc8, lwg_stream_t stream)
{
    LWG_REQUIRE(fim && wim && map_fn && side && src_f2p && ref_f2p && src_img && ref_img, "animate_inputs: NULL input");
    LWG_REQUIRE(T_src && T_ref, "animate_inputs: NULL flow output (T_src and T_ref are always written)");
    LWG_REQUIRE(bs > 0 && nf > 0 && image_size > 0 && nc > 0, "animate_inputs: bs/nf/image_size/nc must be positive");
    if (tsf_inputs_nhwc8 && nc != 3)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "animate_inputs: the NHWC8 generator input needs nc == 3 (got %d)", nc);
    if (image_size > 8192 || (long)bs * image_size * image_size > (1l << 30))
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "animate_inputs: problem too large (bs=%d is=%d)", bs, image_size);
    LWG_REQUIRE(!((reinterpret_cast<uintptr_t>(src_f2p) | reinterpret_cast<uintptr_t>(ref_f2p) | reinterpret_cast<uintptr_t>(T_src) |
                   reinterpret_cast<uintptr_t>(T_ref)) & 7),
                "animate_inputs: face tables and flows must be 8-byte aligned");
    LWG_REQUIRE(!(reinterpret_cast<uintptr_t>(tsf_inputs_nhwc8) & 15), "animate_inputs: the NHWC8 output must be 16-byte aligned");
    AnimateArgs a;
    a.fim = fim;
    a.wim = wim;
    a.map_fn = map_fn;
    a.side = side;
    a.src_f2p = src_f2p;
    a.ref_f2p = ref_f2p;
    a.src_img = src_img;
    a.ref_img = ref_img;
    a.T_src = T_src;
    a.T_ref = T_ref;
    a.cond = cond;
    a.tsf_img = tsf_img;
    a.x_nchw = tsf_inputs;
    a.x_nhwc8 = tsf_inputs_nhwc8;
    a.bs = bs;
    a.nf = nf;
    a.is = image_size;
    a.nc = nc;
    a.align_corners = align_corners;
    const long total = (long)bs * image_size * image_size;
    animate_inputs_kernel<<<ceil_div(total, 256), 256, 0, as_stream(stream)>>>(a);
    LWG_LAUNCH_CHECK("animate_inputs_kernel");
    return LWG_OK;
}

}  // extern "C"
