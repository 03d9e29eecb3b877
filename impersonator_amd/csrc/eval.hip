// eval.hip -- paired evaluation of generated frames on the device (gfx950): windowed SSIM statistics + MSE + range of the
// reference image, F.interpolate's bilinear resize (align_corners=False) and the reduction of the scale-shape-pose error.
//
// Restates thirdparty/his_evaluators/.../metrics/metrics.py (SSIMMetric, PSNRMetric, ScaleShapePoseError) of the reference:
//   SSIM : scikit-image 0.16.2 structural_similarity(pred, ref, multichannel=True) on float32 images -- 7x7 uniform window,
//          data_range 2 (the float dtype range), K1 = 0.01, K2 = 0.03, sample covariance (cov_norm = 49/48), the mean of S over
//          the window positions that lie inside the image, per channel, then the mean of the three channels.
//   PSNR : 10 log10(data_range^2 / mse); the kernel gives mse, min(ref) and max(ref), the host picks data_range as
//          scikit-image does and takes the logarithm.
//   SSPE : |d[0]|, sum |d[75:85]|, sum |d[0:75]| of d = pred_theta - ref_theta, per frame.
//
// Arithmetic.  A pixel is loaded and mapped in float32 (the three modes of pixel.h's map_pixel, one rounding per step);
// everything after that is fp64: the products of two float32 values are exact there, so the window moments lose nothing before
// the subtraction uxx - ux*ux that a float32 statement gets wrong on flat regions.
//
// Tiling.  One workgroup of 256 lanes owns a 16x16 tile of one (frame, channel) plane: its pixels for the squared-difference sum
// and min/max (every pixel belongs to exactly one tile), and the window positions whose top-left pixel lies in it for S.  It
// loads the 22x22 patch those windows cover, sums 7 taps along x into LDS (22 rows x 16 columns x 5 moments, fp64), then 7 rows
// along y, and reduces its 256 values with a fixed LDS tree.  The four partials go to workspace[plane][tile]; a second kernel,
// one workgroup per frame, adds each channel's tiles in index order per lane and the lanes with the same tree.  No atomics, no
// dependence on N or on the frame's position in the batch: a frame's four numbers are the same bits wherever it is scored.
#include "common.h"
#include "pixel.h"

namespace lwg {
namespace {

constexpr int kTile = 16;             // tile edge: 256 lanes, one window position and one owned pixel each
constexpr int kWin = 7;               // scikit-image's default win_size
constexpr int kPatch = kTile + kWin - 1;
constexpr int kStatsPerTile = 4;      // sum S, sum (pred-ref)^2, min ref, max ref

// fixed-order reductions over the 256 lanes of a workgroup; the result is valid in lane 0
template <class Op>
__device__ __forceinline__ double block_reduce(double v, double *scratch, Op op)
{
    const int t = threadIdx.x;
    __syncthreads();                   // the previous use of scratch is over
    scratch[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) scratch[t] = op(scratch[t], scratch[t + s]);
        __syncthreads();
    }
    return scratch[0];
}

struct OpAdd { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMin { __device__ double operator()(double a, double b) const { return b < a ? b : a; } };
struct OpMax { __device__ double operator()(double a, double b) const { return b > a ? b : a; } };

__global__ __launch_bounds__(256) void pair_stats_tiles_kernel(const float *__restrict__ pred, const float *__restrict__ ref,
                                                               int H, int W, int tiles_x, int mode,
                                                               double *__restrict__ partial)
{
    __shared__ float sp[kPatch][kPatch + 1];
    __shared__ float sr[kPatch][kPatch + 1];
    __shared__ double hs[5][kPatch][kTile];
    __shared__ double scratch[256];

    const int tile = blockIdx.x, plane = blockIdx.y;
    const int y0 = (tile / tiles_x) * kTile, x0 = (tile % tiles_x) * kTile;
    const float *p = pred + (size_t)plane * H * W;
    const float *r = ref + (size_t)plane * H * W;
    const int t = threadIdx.x;

    // the patch under this tile's windows; outside the image 0, which no valid window reads
    for (int i = t; i < kPatch * kPatch; i += 256) {
        const int py = i / kPatch, px = i % kPatch;
        const int y = y0 + py, x = x0 + px;
        float a = 0.f, b = 0.f;
        if (y < H && x < W) {
            a = map_pixel(p[(size_t)y * W + x], mode);
            b = map_pixel(r[(size_t)y * W + x], mode);
        }
        sp[py][px] = a;
        sr[py][px] = b;
    }
    __syncthreads();

    // 7 taps along x: sums of x, y, xx, yy, xy for the window columns that start in this tile
    for (int i = t; i < kPatch * kTile; i += 256) {
        const int py = i / kTile, lx = i % kTile;
        double sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const double a = (double)sp[py][lx + k], b = (double)sr[py][lx + k];
            sa += a;
            sb += b;
            saa += a * a;
            sbb += b * b;
            sab += a * b;
        }
        hs[0][py][lx] = sa;
        hs[1][py][lx] = sb;
        hs[2][py][lx] = saa;
        hs[3][py][lx] = sbb;
        hs[4][py][lx] = sab;
    }
    __syncthreads();

    const int ly = t / kTile, lx = t % kTile;
    const int y = y0 + ly, x = x0 + lx;

    // 7 rows along y, then S at the window position (y, x)
    double S = 0.0;
    if (y + kWin <= H && x + kWin <= W) {
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < kWin; ++k) s += hs[q][ly + k][lx];
            m[q] = s / 49.0;
        }
        const double cov_norm = 49.0 / 48.0;
        const double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);
        const double ux = m[0], uy = m[1];
        const double vx = cov_norm * (m[2] - ux * ux);
        const double vy = cov_norm * (m[3] - uy * uy);
        const double vxy = cov_norm * (m[4] - ux * uy);
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
        const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        S = (A1 * A2) / (B1 * B2);
    }

    // the pixel this lane owns
    double sq = 0.0, lo = __builtin_huge_val(), hi = -__builtin_huge_val();
    if (y < H && x < W) {
        const double a = (double)sp[ly][lx], b = (double)sr[ly][lx];
        const double d = a - b;
        sq = d * d;
        lo = hi = b;
    }

    const double sumS = block_reduce(S, scratch, OpAdd());
    const double sumQ = block_reduce(sq, scratch, OpAdd());
    const double mn = block_reduce(lo, scratch, OpMin());
    const double mx = block_reduce(hi, scratch, OpMax());
    if (t == 0) {
        double *o = partial + ((size_t)plane * gridDim.x + tile) * kStatsPerTile;
        o[0] = sumS;
        o[1] = sumQ;
        o[2] = mn;
        o[3] = mx;
    }
}

// one workgroup per frame: channel by channel, lane t adds tiles t, t+256, ... in that order, then the lanes are added by the
// tree of block_reduce.  stats[n] = [mean over channels of mean S, mean squared difference, min ref, max ref]
__global__ __launch_bounds__(256) void pair_stats_finalize_kernel(const double *__restrict__ partial, int tiles, int H, int W,
                                                                  double *__restrict__ stats)
{
    __shared__ double scratch[256];
    const int n = blockIdx.x, t = threadIdx.x;
    const double positions = (double)(H - kWin + 1) * (double)(W - kWin + 1);
    double mssim = 0.0, sq = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (int c = 0; c < 3; ++c) {
        const double *q = partial + ((size_t)n * 3 + c) * tiles * kStatsPerTile;
        double s = 0.0, e = 0.0, lo = __builtin_huge_val(), hi = -__builtin_huge_val();
        for (int i = t; i < tiles; i += 256) {
            s += q[(size_t)i * kStatsPerTile + 0];
            e += q[(size_t)i * kStatsPerTile + 1];
            const double a = q[(size_t)i * kStatsPerTile + 2], b = q[(size_t)i * kStatsPerTile + 3];
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        s = block_reduce(s, scratch, OpAdd());
        e = block_reduce(e, scratch, OpAdd());
        lo = block_reduce(lo, scratch, OpMin());
        hi = block_reduce(hi, scratch, OpMax());
        mssim += s / positions;
        sq += e;
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
    }
    if (t == 0) {
        double *o = stats + (size_t)n * 4;
        o[0] = mssim / 3.0;
        o[1] = sq / (3.0 * (double)H * (double)W);
        o[2] = mn;
        o[3] = mx;
    }
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float *__restrict__ x, int H, int W, int Ho, int Wo,
                                                              long total, float *__restrict__ y)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
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
    const float top = r0[x0] * wx0 + r0[x1] * wx1;
    const float bot = r1[x0] * wx0 + r1[x1] * wx1;
    y[i] = top * wy0 + bot * wy1;
}

constexpr int kTheta = 85, kShape = 10;

// one lane per frame: 85 differences, added in index order
__global__ __launch_bounds__(64) void sspe_terms_kernel(const float *__restrict__ a, const float *__restrict__ b, int N,
                                                        double *__restrict__ terms)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float *pa = a + (size_t)n * kTheta, *pb = b + (size_t)n * kTheta;
    double pose = 0.0, shape = 0.0;
    for (int k = 0; k < kTheta - kShape; ++k) pose += fabs((double)pa[k] - (double)pb[k]);
    for (int k = kTheta - kShape; k < kTheta; ++k) shape += fabs((double)pa[k] - (double)pb[k]);
    double *o = terms + (size_t)n * 3;
    o[0] = fabs((double)pa[0] - (double)pb[0]);
    o[1] = shape;
    o[2] = pose;
}

inline long tiles_of(int H, int W) { return (long)ceil_div(H, kTile) * ceil_div(W, kTile); }

}  // namespace
}  // namespace lwg

using namespace lwg;

extern "C" {

size_t lwg_eval_workspace_bytes(int N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)N * 3 * (size_t)tiles_of(H, W) * kStatsPerTile * sizeof(double);
}

int lwg_eval_pair_stats(const float *pred, const float *ref, int N, int H, int W, int mode, double *stats, void *workspace,
                        size_t workspace_bytes, lwg_stream_t stream)
{
    LWG_REQUIRE(pred && ref && stats && workspace, "eval_pair_stats: NULL argument");
    LWG_REQUIRE(N > 0 && H > 0 && W > 0, "eval_pair_stats: sizes must be positive (N=%d H=%d W=%d)", N, H, W);
    LWG_REQUIRE(mode >= 0 && mode <= 2, "eval_pair_stats: mode %d is none of 0 (as is), 1 ([0,1] input), 2 (8-bit round trip)", mode);
    LWG_REQUIRE((uintptr_t)pred % 4 == 0 && (uintptr_t)ref % 4 == 0, "eval_pair_stats: images must be 4-byte aligned");
    LWG_REQUIRE((uintptr_t)stats % 8 == 0 && (uintptr_t)workspace % 8 == 0, "eval_pair_stats: stats and workspace must be 8-byte aligned (fp64)");
    if (H < kWin || W < kWin)
        LWG_FAIL(LWG_ERR_UNSUPPORTED, "eval_pair_stats: %dx%d is smaller than the 7x7 window", H, W);
    if ((long)N * 3 > 65535) LWG_FAIL(LWG_ERR_UNSUPPORTED, "eval_pair_stats: N=%d exceeds 21845 frames per call", N);
    const long tiles = tiles_of(H, W);
    if (tiles > 0x7fffffffL) LWG_FAIL(LWG_ERR_UNSUPPORTED, "eval_pair_stats: %dx%d has too many tiles", H, W);
    const size_t need = lwg_eval_workspace_bytes(N, H, W);
    if (workspace_bytes < need)
        LWG_FAIL(LWG_ERR_WORKSPACE, "eval_pair_stats: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    double *partial = static_cast<double *>(workspace);
    pair_stats_tiles_kernel<<<dim3((unsigned)tiles, (unsigned)(N * 3)), 256, 0, as_stream(stream)>>>(
        pred, ref, H, W, ceil_div(W, kTile), mode, partial);
    LWG_LAUNCH_CHECK("pair_stats_tiles_kernel");
    pair_stats_finalize_kernel<<<N, 256, 0, as_stream(stream)>>>(partial, (int)tiles, H, W, stats);
    LWG_LAUNCH_CHECK("pair_stats_finalize_kernel");
    return LWG_OK;
}

int lwg_resize_bilinear(const float *x, int N, int C, int H, int W, int Ho, int Wo, float *y, lwg_stream_t stream)
{
    LWG_REQUIRE(x && y, "resize_bilinear: NULL argument");
    LWG_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0,
                "resize_bilinear: sizes must be positive (N=%d C=%d %dx%d -> %dx%d)", N, C, H, W, Ho, Wo);
    LWG_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0, "resize_bilinear: tensors must be 4-byte aligned");
    const long total = (long)N * C * Ho * Wo;
    if (total > 256L * 0x7fffffffL) LWG_FAIL(LWG_ERR_UNSUPPORTED, "resize_bilinear: %ld outputs exceed one launch", total);
    resize_bilinear_kernel<<<ceil_div(total, 256), 256, 0, as_stream(stream)>>>(x, H, W, Ho, Wo, total, y);
    LWG_LAUNCH_CHECK("resize_bilinear_kernel");
    return LWG_OK;
}

int lwg_eval_sspe_terms(const float *pred_theta, const float *ref_theta, int N, double *terms, lwg_stream_t stream)
{
    LWG_REQUIRE(pred_theta && ref_theta && terms, "eval_sspe_terms: NULL argument");
    LWG_REQUIRE(N > 0, "eval_sspe_terms: N must be positive (N=%d)", N);
    LWG_REQUIRE((uintptr_t)pred_theta % 4 == 0 && (uintptr_t)ref_theta % 4 == 0 && (uintptr_t)terms % 8 == 0,
                "eval_sspe_terms: thetas must be 4-byte and terms 8-byte aligned");
    sspe_terms_kernel<<<ceil_div(N, 64), 64, 0, as_stream(stream)>>>(pred_theta, ref_theta, N, terms);
    LWG_LAUNCH_CHECK("sspe_terms_kernel");
    return LWG_OK;
}

}  // extern "C"
