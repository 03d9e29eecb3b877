// igemm32.h -- the exact-fp32 implicit-GEMM convolution that the HMR regressor (hmr.hip), LPIPS/AlexNet (lpips.hip) and InceptionV3
// (inception.hip) run on, stated once.
//
//   igemm32::conv_kernel<P>: implicit GEMM on v_mfma_f32_32x32x2_f32 (bit-for-bit a k-ordered fmaf chain).  Workgroup = 64 pixels x
//   64 output channels, four waves of one 32x32 tile, K = taps x Cin walked 32 at a time through a double-buffered LDS stage.
//   Activations are NHWC; the pixel dimension M = N*Ho*Wo is FLATTENED ACROSS IMAGES and predicated at its tail, the K tail is
//   zero-filled.  The reduction order of an output element is (tap, input channel) ascending, whatever its position in M or the
//   batch size.
//
// The kernel owns the row decode, the loaders' lane mapping, the LDS staging, the K loop, the MFMA walk and the mapping of an
// accumulator register to (m, co).  What differs between the networks is a policy struct P that each of them defines in its own
// file, and that is the kernel's one argument:
//
//   igemm32::Geom g;                             the geometry and the weights
//   static constexpr bool kCoutTail;             true: Cout is any multiple of 4, the B loads and the stores past it are masked;
//                                                false: Cout % 64 == 0
//   float4 gather(const Row &r, int kg) const;   the A values of reduction indices kg .. kg + 3 of one row, activated; the two
//                                                generic forms are gather_nhwc4 and gather_each below
//   Col column(int co) const;                    what the epilogue needs of one output channel, read once per lane
//   void write(long m, int co, const Col &c, float acc) const;   the epilogue of one output element
//
// This header holds NO floating-point arithmetic but the MFMA and zero-fills: hmr.hip is built with fp contraction allowed,
// lpips.hip and inception.hip without, so every float operation of a prologue or an epilogue stays in the policy, in the file
// whose flags it was written for.
#pragma once
#include "common.h"

namespace lwg {
namespace igemm32 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 32;
constexpr int A_PITCH = BK + 1;   // odd pitch: the 32 rows a fragment read touches fall into 32 banks
constexpr int B_PITCH = BN;

struct Geom {
    const float *w;          // (kh*kw*Cin, Cout): [kh][kw][ci][co]
    int N, H, W, Cin, Cout, kh, kw, stride, ph, pw, Ho, Wo;   // a square kernel has kh == kw, ph == pw
    long M;                  // N*Ho*Wo
    int K;                   // kh*kw*Cin
};

// one row of A, an output pixel: ok = inside M; its image and the input pixel of tap (0, 0)
struct Row {
    bool ok;
    int n, ih0, iw0;
};

// where reduction index kg of a row reads: input channel c of pixel (ih, iw).  false -- the value is 0 -- outside the image
// (padding).  cin: g.Cin, or the constant a policy knows it to be
__device__ __forceinline__ bool locate(const Geom &g, const Row &r, int kg, int cin, int &c, int &ih, int &iw)
{
    const int tap = kg / cin;
    c = kg - tap * cin;
    const int kh = tap / g.kw, kw = tap - kh * g.kw;
    ih = r.ih0 + kh;
    iw = r.iw0 + kw;
    return (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
}

// channel c of pixel (ih, iw) of the row's image in an (N,H,W,Cin) NHWC tensor
__device__ __forceinline__ const float *nhwc_at(const Geom &g, const float *x, const Row &r, int c, int ih, int iw)
{
    return x + (((size_t)r.n * g.H + ih) * g.W + iw) * g.Cin + c;
}

struct AsIs {
    __device__ float4 operator()(float4 v, int) const { return v; }
};

// gather, Cin % 4 == 0: four consecutive reduction indices are one 16-byte load inside one tap; act(value, c) activates what was
// loaded (a padded tap stays 0: torch pads the activated tensor)
template <class Act = AsIs>
__device__ __forceinline__ float4 gather_nhwc4(const Geom &g, const float *x, const Row &r, int kg, Act act = Act())
{
    // kg is decoded before the row's predicate: the two rows a lane loads share the decode, and it is computed once
    int c, ih, iw;
    const bool inside = locate(g, r, kg, g.Cin, c, ih, iw);
    if (!r.ok || kg >= g.K || !inside) return make_float4(0.f, 0.f, 0.f, 0.f);   // past M, past K, padding
    return act(*reinterpret_cast<const float4 *>(nhwc_at(g, x, r, c, ih, iw)), c);
}

// gather, any Cin and any layout: four separate elements; fetch(c, ih, iw) reads one input value and activates it
template <class Fetch>
__device__ __forceinline__ float4 gather_each(const Geom &g, const Row &r, int kg, int cin, Fetch fetch)
{
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c, ih, iw;
        v[j] = r.ok && kg + j < g.K && locate(g, r, kg + j, cin, c, ih, iw) ? fetch(c, ih, iw) : 0.f;   // 0 past M, past K, in the padding
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

template <class P>
__global__ __launch_bounds__(256) void conv_kernel(const P p)
{
    __shared__ __attribute__((aligned(16))) float sA[2][BM * A_PITCH];
    __shared__ __attribute__((aligned(16))) float sB[2][BK * B_PITCH];
    const Geom &g = p.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long m0 = (long)blockIdx.x * BM;
    const int co0 = blockIdx.y * BN;

    // A loader: rows (tid >> 3) and (tid >> 3) + 32, reduction indices (tid & 7) * 4 .. + 3 of the stage
    const int a_col = (tid & 7) * 4;
    Row row[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const long m = m0 + (tid >> 3) + 32 * v;
        row[v].ok = m < g.M;
        const long mm = row[v].ok ? m : 0;
        const int n = (int)(mm / ((long)g.Ho * g.Wo));
        const int rem = (int)(mm - (long)n * g.Ho * g.Wo);
        const int oh = rem / g.Wo, ow = rem - oh * g.Wo;
        row[v].n = n;
        row[v].ih0 = oh * g.stride - g.ph;
        row[v].iw0 = ow * g.stride - g.pw;
    }
    // B loader: reduction rows (tid >> 4) and (tid >> 4) + 16, output channels (tid & 15) * 4 .. + 3 (Cout % 4 == 0)
    const int b_col = (tid & 15) * 4;
    const bool b_ok = !P::kCoutTail || co0 + b_col < g.Cout;

    float4 ra[2], rb[2];
    auto load = [&](int k0) {
#pragma unroll
        for (int v = 0; v < 2; ++v) ra[v] = p.gather(row[v], k0 + a_col);
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int kr = k0 + (tid >> 4) + 16 * v;
            rb[v] = (b_ok && kr < g.K) ? *reinterpret_cast<const float4 *>(g.w + (size_t)kr * g.Cout + co0 + b_col)
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
    for (int k0 = 0; k0 < g.K; k0 += BK) {
        const bool more = k0 + BK < g.K;
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
    if (P::kCoutTail && co >= g.Cout) return;
    const auto col = p.column(co);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.M) continue;
        p.write(m, co, col, acc[r]);
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline int conv_out(int in, int k, int stride, int pad) { return in + 2 * pad >= k ? (in + 2 * pad - k) / stride + 1 : 0; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the guards of the op-level entries: an (N,H,W,C) tensor of 2^40 elements or more; a K or a grid.x that no int holds
inline bool too_large(int N, int H, int W, int C) { return (long)N * H * W * (long)C >= (1L << 40); }
inline bool grid_too_large(int N, int Ho, int Wo, int kh, int kw, int Cin)
{
    return (long)kh * kw * Cin > 0x7fffffffL || ((long)N * Ho * Wo + BM - 1) / BM > 0x7fffffffL;
}

// the caller's part of a Geom; launch fills the rest
inline Geom geom(const float *w, int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw)
{
    return Geom{w, N, H, W, Cin, Cout, kh, kw, stride, ph, pw, 0, 0, 0, 0};
}

template <class P>
int launch(P p, const char *name, hipStream_t st)
{
    Geom &g = p.g;
    g.Ho = conv_out(g.H, g.kh, g.stride, g.ph);
    g.Wo = conv_out(g.W, g.kw, g.stride, g.pw);
    g.M = (long)g.N * g.Ho * g.Wo;
    g.K = g.kh * g.kw * g.Cin;
    const dim3 grid((unsigned)ceil_div(g.M, BM), (unsigned)(P::kCoutTail ? ceil_div(g.Cout, BN) : g.Cout / BN));
    conv_kernel<P><<<grid, 256, 0, st>>>(p);
    LWG_LAUNCH_CHECK(name);
    return LWG_OK;
}

}  // namespace igemm32
}  // namespace lwg
