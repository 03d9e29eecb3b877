// tools/mfma_peak.hip -- what a wave can get out of the two bf16 MFMA shapes, v_mfma_f32_32x32x16_bf16 and
// v_mfma_f32_16x16x32_bf16, at the same output tile per wave (development probe, not part of liblwg).
//   hipcc --offload-arch=gfx950 -O3 tools/mfma_peak.hip -o tools/_build/mfma_peak
// Bare arms: one wave per SIMD (256 threads per CU-sized workgroup), NACC accumulators walked round-robin so that a
// dependent MFMA follows its producer after NACC-1 independent ones; operands in registers, random (power) or zero.
// The 16x16x32 arm holds the same 64 fp32 accumulators per lane as four 32x32 tiles: 16 tiles of 4.
// LDS-fed arms: the halo convolution's loop without its DMA -- a 64 x 64 wave tile, bf16x3 (lo*hi, hi*lo, hi*hi), every
// operand re-read from a swizzled 128-byte-row LDS image ([hi x32 | lo x32] per row, 16-byte slots XOR (row >> 1) & 7) with
// ds_read_b128: eight fragment reads per 12 MFMAs of 32x32x16, per 24 of 16x16x32; one and two waves per SIMD.
// The 16x16x32 kernels ask for two waves per SIMD (a 256-register budget): hipcc then selects the MFMA form whose result is tied
// to its accumulator operand.  With the 512-register budget it selects the untied AGPR form of this four-pass instruction and
// permutes the 64 accumulators through ~100 v_accvgpr moves per iteration (21.9 cycles per MFMA instead of 16).
// Every arm prints TFLOP/s by wall, the cycles of one loop iteration and the in-kernel clock (s_memtime over s_memrealtime).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Stamp { unsigned long long c0, r0; };
__device__ __forceinline__ Stamp stamp_begin() { return {__builtin_amdgcn_s_memtime(), __builtin_amdgcn_s_memrealtime()}; }
// (cycles, 100 MHz ticks) of the loop, one record per workgroup, into a buffer nothing else reads
__device__ __forceinline__ void stamp_end(const Stamp &s, unsigned long long *clk)
{
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        clk[2 * blockIdx.x] = c1 - s.c0;
        clk[2 * blockIdx.x + 1] = r1 - s.r0;
    }
}

template <int NACC>
__global__ __launch_bounds__(256) void mfma_loop(const float4 *in, float *out, unsigned long long *clk, int iters)
{
    const float4 av = in[threadIdx.x], bv = in[256 + threadIdx.x];
    const bf16x8 a = __builtin_bit_cast(bf16x8, av), b = __builtin_bit_cast(bf16x8, bv);
    f32x16 acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
    const Stamp st = stamp_begin();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 32 / NACC; ++u)
#pragma unroll
            for (int k = 0; k < NACC; ++k) acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[k], 0, 0, 0);
    }
    stamp_end(st, clk);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NACC; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[k][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

// the same FLOP per iteration (32 MFMAs of 32x32x16 = 64 of 16x16x32) on 16 accumulator tiles of 4
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void mfma_loop_16(const float4 *in, float *out, unsigned long long *clk, int iters)
{
    const float4 av = in[threadIdx.x], bv = in[256 + threadIdx.x];
    const bf16x8 a = __builtin_bit_cast(bf16x8, av), b = __builtin_bit_cast(bf16x8, bv);
    f32x4 acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[k][r] = 0.f;
    const Stamp st = stamp_begin();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[k], 0, 0, 0);
    }
    stamp_end(st, clk);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += acc[k][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

// LDS image: A rows 0..63 then B rows 0..63, 128 bytes each, two copies 16 KiB apart read on alternate iterations (so
// that no read can be hoisted out of the loop).  One iteration = K 32 of the 64 x 64 tile, three products.
constexpr int kLdsCopy = 128 * 128, kLdsBytes = 2 * kLdsCopy;

template <bool S16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(S16 ? 2 : 1, S16 ? 2 : 10))) void mfma_lds_loop(const float4 *in, float *out, unsigned long long *clk, int iters)
{
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
    for (int i = threadIdx.x; i < kLdsBytes / 16; i += 256) reinterpret_cast<float4 *>(lds)[i] = in[i & 511];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    auto rd = [&](int off) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(lds + off)); };
    float s = 0.f;
    if constexpr (!S16) {
        // lane -> row lane & 31, k = 8 (lane >> 5) + j of a 16-k block: slot 2 kb + (lane >> 5), the lo fragment ^ 64
        const int row = lane & 31, half = lane >> 5;
        int aa[2], bb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            aa[i] = (32 * i + row) * 128 + ((half ^ ((row >> 1) & 7)) << 4);
            bb[i] = 64 * 128 + aa[i];
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        struct Frags { bf16x8 al[2], bh[2], ah[2], bl[2]; };
        auto load = [&](Frags &f, int copy, int kb) {
            const int x = copy * kLdsCopy;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f.al[i] = rd(x + (aa[i] ^ (64 + 32 * kb)));
                f.bh[i] = rd(x + (bb[i] ^ (32 * kb)));
                f.ah[i] = rd(x + (aa[i] ^ (32 * kb)));
                f.bl[i] = rd(x + (bb[i] ^ (64 + 32 * kb)));
            }
        };
        Frags f0, f1;
        load(f0, 0, 0);
        const Stamp st = stamp_begin();
        for (int it = 0; it < iters; ++it) {
            load(f1, it & 1, 1);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const Frags &f = kb ? f1 : f0;
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(t == 0 ? f.al[i] : f.ah[i], t == 1 ? f.bl[j] : f.bh[j],
                                                                                acc[i][j], 0, 0, 0);
                if (kb == 0) load(f0, (it + 1) & 1, 0);
            }
        }
        stamp_end(st, clk);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) s += acc[i][j][r];
    } else {
        // lane -> row lane & 15, k = 8 (lane >> 4) + j of the whole 32-k slice: slot lane >> 4, the lo fragment ^ 64
        const int row = lane & 15, quarter = lane >> 4;
        int aa[4], bb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 16 * i + row;
            aa[i] = r * 128 + ((quarter ^ ((r >> 1) & 7)) << 4);
            bb[i] = 64 * 128 + aa[i];
        }
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
        // the halo loop's two live sets: {al, bh} of the iteration about to run, {ah, bl} read behind its first MFMAs
        struct Frags { bf16x8 a[4], b[4]; };
        auto load = [&](Frags &f, int copy, bool first) {
            const int x = copy * kLdsCopy;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f.a[i] = rd(x + (aa[i] ^ (first ? 64 : 0)));
                f.b[i] = rd(x + (bb[i] ^ (first ? 0 : 64)));
            }
        };
        Frags f0, f1;   // f0 = {al, bh}, f1 = {ah, bl}
        load(f0, 0, true);
        const Stamp st = stamp_begin();
        for (int it = 0; it < iters; ++it) {
            load(f1, it & 1, false);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t == 0 ? f0.a[i] : f1.a[i], t == 1 ? f1.b[j] : f0.b[j],
                                                                            acc[i][j], 0, 0, 0);
                if (t == 0) {   // al is dead: its registers take the next iteration's
#pragma unroll
                    for (int i = 0; i < 4; ++i) f0.a[i] = rd(((it + 1) & 1) * kLdsCopy + (aa[i] ^ 64));
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) f0.b[i] = rd(((it + 1) & 1) * kLdsCopy + bb[i]);
        }
        stamp_end(st, clk);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += acc[i][j][r];
    }
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

static unsigned long long *g_clk;   // device: (cycles, 100 MHz ticks) per workgroup

// mfma32 = MFMAs per iteration and wave counted as 32x32x16 (32768 FLOP each)
template <class K>
static void run(const char *name, K kern, const float4 *in, float *out, int blocks, int iters, double mfma32)
{
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    constexpr int kLaunches = 10;   // ~20 ms each
    for (int w = 0; w < kLaunches; ++w) kern<<<blocks, 256>>>(in, out, g_clk, iters);   // ~200 ms: settle the clocks
    hipEventRecord(e0);
    for (int w = 0; w < kLaunches; ++w) kern<<<blocks, 256>>>(in, out, g_clk, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> c(2 * blocks);
    hipMemcpy(c.data(), g_clk, c.size() * 8, hipMemcpyDeviceToHost);
    double cyc = 0, ghz = 0;
    for (int b = 0; b < blocks; ++b) {
        cyc += (double)c[2 * b] / iters / blocks;
        ghz += (double)c[2 * b] / (double)c[2 * b + 1] * 0.1 / blocks;
    }
    const double flop = (double)kLaunches * blocks * 4 * (double)iters * mfma32 * 32768.0;
    printf("%-44s %8.1f TFLOP/s  (%.1f%% of 2500)  %7.1f cyc/iter  %.2f GHz\n", name, flop / (ms * 1e-3) / 1e12,
           flop / (ms * 1e-3) / 2.5e15 * 100, cyc, ghz);
}

int main()
{
    float4 *in;
    float *out;
    hipMalloc(&in, 512 * 16);
    hipMalloc(&out, 1024 * 256 * 4);
    hipMalloc(&g_clk, 1024 * 16);
    std::vector<unsigned short> h(512 * 8);
    for (int pass = 0; pass < 2; ++pass) {
        for (auto &v : h) v = pass ? (unsigned short)(0x3c00 + (rand() & 0x3ff)) : 0;   // bf16 in [0.0078, 0.03) / zeros
        hipMemcpy(in, h.data(), 512 * 16, hipMemcpyHostToDevice);
        const char *what = pass ? "random" : "zero";
        printf("-- %s operands in registers, 256 workgroups (one wave per SIMD)\n", what);
        run("32x32x16, 2 accumulators", mfma_loop<2>, in, out, 256, 40000, 32);
        run("32x32x16, 4 accumulators", mfma_loop<4>, in, out, 256, 40000, 32);
        run("32x32x16, 8 accumulators", mfma_loop<8>, in, out, 256, 40000, 32);
        run("16x16x32, 16 accumulators of 4", mfma_loop_16, in, out, 256, 40000, 32);
        printf("-- %s operands in registers, 512 workgroups (two waves per SIMD)\n", what);
        run("32x32x16, 4 accumulators", mfma_loop<4>, in, out, 512, 40000, 32);
        run("16x16x32, 16 accumulators of 4", mfma_loop_16, in, out, 512, 40000, 32);
        for (int waves = 1; waves <= 2; ++waves) {
            printf("-- %s operands re-read from LDS (ds_read_b128), bf16x3 on a 64x64 wave tile, %d workgroups (%s per SIMD)\n", what,
                   256 * waves, waves == 1 ? "one wave" : "two waves");
            run("32x32x16, 16 reads per 24 MFMAs", mfma_lds_loop<false>, in, out, 256 * waves, 50000, 24);
            run("16x16x32, 16 reads per 48 MFMAs", mfma_lds_loop<true>, in, out, 256 * waves, 50000, 24);
        }
    }
    return 0;
}
