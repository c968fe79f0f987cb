// msssim_kernels.hip -- gfx950 kernels of multi-scale SSIM (Wang, Simoncelli & Bovik 2003), behind
// rmgr_ssim_hip_compute_msssim_device / _host.  The definition they implement is in include/rmgr/ssim-hip.h.
//
// Kept apart from ssim_kernels.hip on purpose: that file's sha256 is the kernel source id measurements are tied to
// (Makefile, profiles/traffic.json).  The taps and constants below are therefore copies of the engine's, not shared.
//
// Per scale s of a batch (one launch each, every image of the batch in it):
//  * msssim_stats_kernel<U8>: one 256-thread workgroup per 64 x 16 output tile.  It stages the tile plus a 5-pixel halo
//    (edge-clamped) as centred (a', b', a'^2 + b'^2, a'b') in LDS (centre below), blurs the four planes vertically (11 taps, 74 x 16
//    values) into a second LDS buffer, then horizontally (11 taps) into registers, forms cs and ssim per pixel in fp32
//    and sums them in fp64: per thread in a fixed order, then a fixed LDS tree.  One (cs, ssim) partial per tile goes
//    to [image][scale][tile].  No MFMA: plain fp32 VALU, as everywhere on this project's path.
//  * msssim_downsample_kernel<U8>: scale s -> s + 1, the clamped 2 x 2 box mean, two output pixels per thread.  The
//    pyramid is exact in fp32 (the header says why), so its values do not depend on anything but the pixels.
//  * msssim_reduce_kernel: one workgroup per (image, scale) sums that image's tile partials in a fixed order.
// U8 = the source is the caller's uint8 pair (scale 0: any step / stride); otherwise a dense float2 (a, b) plane.
//
// Centring.  MODE_SEPARABLE blurs a' = a - 128 so that E[a'^2] - mu_a'^2 cancels between numbers of at most 16384, not 65025.  Here
// every tile subtracts its OWN integer centre per image -- floor() of A's and of B's pixel at the tile's (clamped) middle: a - c is a
// multiple of 4^-s below 256 in magnitude, exact in fp32 at every scale, and in the flat or dark areas where the cancellation hurts it
// leaves numbers near 0.  On the golden fixtures an fp32 model of this kernel (all scales 1..8) lands within 5.9e-7 of the float64
// definition with the tile centre, 1.3e-5 with 128: a few-pixel scale has no averaging to hide one pixel's rounding.  The centre sits at
// a fixed place of the image, so results stay independent of the batch.
#include "msssim_kernels.h"
#include <algorithm>
#include <cmath>

namespace ssim_hip {
namespace {

typedef float  f2 __attribute__((ext_vector_type(2)));
typedef float  f4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int   kThreads = 256;
constexpr int   kHalo = 5;
constexpr int   kSW = kMsTileW + 2 * kHalo;      // 74 staged columns
constexpr int   kSH = kMsTileH + 2 * kHalo;      // 26 staged rows
static_assert(kMsTileW * kMsTileH % kThreads == 0, "whole output pixels per thread");

struct MsConsts { float g[6]; float c1, c2; };

struct MsStatsArgs {
    const PairDesc* descs;        // U8: the batch's descriptors
    const f2*       plane;        // !U8: [image][y][x] (a, b) of this scale
    uint32_t        w, h, tiles_x, tiles;        // scale size, tiles per row, tiles per image
    d2*             partials;     // [image][part_stride]: this scale's tiles start at part_off
    uint32_t        part_stride, part_off;
    MsConsts        k;
};

struct MsDownArgs {
    const PairDesc* descs;        // U8: scale 0
    const f2*       src;          // !U8: [image][sh][sw]
    f2*             dst;          // [image][dh][dw]
    uint32_t        sw, sh, dw, dh, row_blocks;  // row_blocks: workgroups per output row (512 pixels each)
};

struct MsReduceArgs {
    const d2* partials;
    d2*       sums;               // [image][scale]
    uint32_t  part_stride, scales;
    uint32_t  off[kMsMaxScales], n[kMsMaxScales];
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ f4 fma4(f4 a, float g, f4 acc) { const f4 gg = {g, g, g, g}; return __builtin_elementwise_fma(a, gg, acc); }

template <bool U8>
__device__ __forceinline__ f2 load_px(const PairDesc& d, const f2* plane, int64_t w, int64_t x, int64_t y)
{
    if (U8) {
        f2 p;
        p.x = (float)d.a[x * d.a_step + y * d.a_stride];
        p.y = (float)d.b[x * d.b_step + y * d.b_stride];
        return p;
    }
    return plane[y * w + x];
}

template <bool U8>
__global__ __launch_bounds__(kThreads) void msssim_stats_kernel(MsStatsArgs a)
{
    __shared__ f4 lds[kSH * kSW + kMsTileH * kSW];        // 30784 + 18944 B: three workgroups per CU
    f4* S = lds;                                          // staged tile + halo, [kSH][kSW]
    f4* V = lds + kSH * kSW;                              // vertical blur, [kMsTileH][kSW]
    d2* R = reinterpret_cast<d2*>(lds);                   // the reduction, over S once the vertical pass has read it

    const int tid = threadIdx.x;
    const uint32_t img = blockIdx.x / a.tiles, t = blockIdx.x - img * a.tiles;
    const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int64_t x0 = (int64_t)tx * kMsTileW, y0 = (int64_t)ty * kMsTileH;
    const int64_t w = a.w, h = a.h;
    PairDesc d = {};
    const f2* plane = nullptr;
    if (U8) d = a.descs[img];
    else    plane = a.plane + (size_t)img * a.w * a.h;

    const f2 mid = load_px<U8>(d, plane, w, clamp64(x0 + kMsTileW / 2, w - 1), clamp64(y0 + kMsTileH / 2, h - 1));
    const float cA = floorf(mid.x), cB = floorf(mid.y);
    // every load of the tile is issued before the first one is waited for (a loop that stores each pixel before loading the next
    // waits out the memory latency once per pixel)
    constexpr int kStage = (kSH * kSW + kThreads - 1) / kThreads;
    f2 px[kStage];
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = tid + j * kThreads, r = i / kSW, cx = i - r * kSW;
        if (i < kSH * kSW) px[j] = load_px<U8>(d, plane, w, clamp64(x0 + cx - kHalo, w - 1), clamp64(y0 + r - kHalo, h - 1));
    }
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = tid + j * kThreads;
        if (i < kSH * kSW) {
            const float ca = px[j].x - cA, cb = px[j].y - cB;
            const f4 v = {ca, cb, ca * ca + cb * cb, ca * cb};
            S[i] = v;
        }
    }
    __syncthreads();

    const float g0 = a.k.g[0], g1 = a.k.g[1], g2 = a.k.g[2], g3 = a.k.g[3], g4 = a.k.g[4], g5 = a.k.g[5];
    for (int i = tid; i < kMsTileH * kSW; i += kThreads) {
        const f4* c = S + i;                              // column cx, rows r .. r + 10 of the staged tile
        f4 acc = c[0] * (f4){g5, g5, g5, g5};
        acc = fma4(c[1 * kSW], g4, acc);
        acc = fma4(c[2 * kSW], g3, acc);
        acc = fma4(c[3 * kSW], g2, acc);
        acc = fma4(c[4 * kSW], g1, acc);
        acc = fma4(c[5 * kSW], g0, acc);
        acc = fma4(c[6 * kSW], g1, acc);
        acc = fma4(c[7 * kSW], g2, acc);
        acc = fma4(c[8 * kSW], g3, acc);
        acc = fma4(c[9 * kSW], g4, acc);
        acc = fma4(c[10 * kSW], g5, acc);
        V[i] = acc;
    }
    __syncthreads();

    double scs = 0.0, sss = 0.0;
#pragma unroll
    for (int j = 0; j < kMsTileW * kMsTileH / kThreads; ++j) {
        const int i = tid + j * kThreads, r = i / kMsTileW, cx = i - r * kMsTileW;
        const f4* c = V + r * kSW + cx;
        f4 m = c[0] * (f4){g5, g5, g5, g5};
        m = fma4(c[1], g4, m);
        m = fma4(c[2], g3, m);
        m = fma4(c[3], g2, m);
        m = fma4(c[4], g1, m);
        m = fma4(c[5], g0, m);
        m = fma4(c[6], g1, m);
        m = fma4(c[7], g2, m);
        m = fma4(c[8], g3, m);
        m = fma4(c[9], g4, m);
        m = fma4(c[10], g5, m);
        if (x0 + cx < w && y0 + r < h) {
            // m = (mu_a', mu_b', E[a'^2 + b'^2], E[a'b']): variance and covariance do not move with the origin
            const float sS = m.z - (m.x * m.x + m.y * m.y), sAB = m.w - m.x * m.y;
            const float muA = m.x + cA, muB = m.y + cB;
            const float cs = (2.0f * sAB + a.k.c2) / (sS + a.k.c2);
            const float l = (2.0f * (muA * muB) + a.k.c1) / (muA * muA + muB * muB + a.k.c1);
            scs += (double)cs;
            sss += (double)(l * cs);
        }
    }
    const d2 mine = {scs, sss};
    R[tid] = mine;
    __syncthreads();
#pragma unroll
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) R[tid] += R[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.partials[(size_t)img * a.part_stride + a.part_off + t] = R[0];
}

template <bool U8>
__global__ __launch_bounds__(kThreads) void msssim_downsample_kernel(MsDownArgs a)
{
    const uint32_t row = blockIdx.x / a.row_blocks, bx = blockIdx.x - row * a.row_blocks;
    const uint32_t img = row / a.dh, y = row - img * a.dh;
    const int64_t x = ((int64_t)bx * kThreads + threadIdx.x) * 2;
    if (x >= a.dw) return;
    const int64_t sw = a.sw, sh = a.sh;
    const int64_t ya = clamp64(2 * (int64_t)y, sh - 1), yb = clamp64(2 * (int64_t)y + 1, sh - 1);
    PairDesc d = {};
    const f2* src = nullptr;
    if (U8) d = a.descs[img];
    else    src = a.src + (size_t)img * a.sw * a.sh;
    f2 o[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t xa = clamp64(2 * x + 2 * k, sw - 1), xb = clamp64(2 * x + 2 * k + 1, sw - 1);
        const f2 p00 = load_px<U8>(d, src, sw, xa, ya), p10 = load_px<U8>(d, src, sw, xb, ya);
        const f2 p01 = load_px<U8>(d, src, sw, xa, yb), p11 = load_px<U8>(d, src, sw, xb, yb);
        const f2 q = {0.25f, 0.25f};
        o[k] = ((p00 + p10) + (p01 + p11)) * q;            // exact: see the header
    }
    f2* out = a.dst + (size_t)img * a.dw * a.dh + (size_t)y * a.dw + x;
    out[0] = o[0];
    if (x + 1 < a.dw) out[1] = o[1];
}

__global__ __launch_bounds__(kThreads) void msssim_reduce_kernel(MsReduceArgs a)
{
    __shared__ d2 R[kThreads];
    const int tid = threadIdx.x;
    const uint32_t img = blockIdx.x / a.scales, s = blockIdx.x - img * a.scales;
    const d2* p = a.partials + (size_t)img * a.part_stride + a.off[s];
    const uint32_t n = a.n[s];
    d2 acc = {0.0, 0.0};
    for (uint32_t i = tid; i < n; i += kThreads) acc += p[i];
    R[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if (tid < k) R[tid] += R[tid + k];
        __syncthreads();
    }
    if (tid == 0) a.sums[blockIdx.x] = R[0];
}

MsConsts ms_consts()
{
    MsConsts k;
    // True 1-D Gaussian, sigma 1.5, normalised over the 11 taps, rounded to float: the engine's gf (ssim_kernels.hip launch()).
    double g[6], norm = 0.0;
    for (int i = 0; i <= 5; ++i) {
        g[i] = exp(-(double)(i * i) / (2.0 * 1.5 * 1.5));
        norm += (i == 0) ? g[i] : 2.0 * g[i];
    }
    for (int i = 0; i <= 5; ++i) k.g[i] = (float)(g[i] / norm);
    // c1, c2: products in double, then cast (the engine's, src/ssim.cpp:956-960 of the reference)
    k.c1 = (float)((0.01 * 255.0) * (0.01 * 255.0));
    k.c2 = (float)((0.03 * 255.0) * (0.03 * 255.0));
    return k;
}

const uint64_t kMaxBlocks = (uint64_t(1) << 24) - 1;      // x 256 work-items stays below 2^32

} // namespace

size_t msssim_scratch_bytes(uint32_t width, uint32_t height, uint32_t count, uint32_t scales)
{
    uint64_t tiles = 0, px = 0;
    for (uint32_t s = 0; s < scales; ++s) {
        const uint32_t w = ms_dim(width, s), h = ms_dim(height, s);
        tiles += ms_tiles(w, h);
        if (s > 0) px += (uint64_t)w * h;
    }
    return (size_t)count * (size_t)(tiles * sizeof(d2) + px * sizeof(f2));
}

uint32_t msssim_max_count(uint32_t width, uint32_t height, uint32_t scales)
{
    const uint64_t stats = ms_tiles(width, height);                                                   // the largest statistics grid per image
    const uint64_t down = scales > 1 ? (uint64_t)ms_dim(height, 1) * ((ms_dim(width, 1) + 2 * kThreads - 1) / (2 * kThreads)) : 1;
    const uint64_t per = std::max<uint64_t>(std::max<uint64_t>(stats, down), scales);
    const uint64_t n = kMaxBlocks / per;
    return (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFu);
}

hipError_t launch_msssim(const PairDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales,
                         void* scratch, double* sums_dev, hipStream_t stream)
{
    if (count == 0 || width == 0 || height == 0 || scales < 1 || scales > kMsMaxScales) return hipErrorInvalidValue;
    if (count > msssim_max_count(width, height, scales)) return hipErrorInvalidValue;
    MsReduceArgs ra = {};
    uint32_t tiles = 0;
    for (uint32_t s = 0; s < scales; ++s) {
        ra.off[s] = tiles;
        ra.n[s] = (uint32_t)ms_tiles(ms_dim(width, s), ms_dim(height, s));
        tiles += ra.n[s];
    }
    d2* partials = static_cast<d2*>(scratch);
    f2* planes = reinterpret_cast<f2*>(partials + (size_t)count * tiles);   // scale s >= 1 follows scale s - 1
    const MsConsts k = ms_consts();
    const dim3 block(kThreads);
    f2* cur = nullptr;                                     // plane of scale s (s >= 1)
    for (uint32_t s = 0; s < scales; ++s) {
        const uint32_t w = ms_dim(width, s), h = ms_dim(height, s);
        MsStatsArgs sa;
        sa.descs = descs_dev;
        sa.plane = cur;
        sa.w = w; sa.h = h;
        sa.tiles_x = (w + kMsTileW - 1) / kMsTileW;
        sa.tiles = ra.n[s];
        sa.partials = partials;
        sa.part_stride = tiles;
        sa.part_off = ra.off[s];
        sa.k = k;
        const dim3 grid((uint32_t)((uint64_t)count * sa.tiles));
        if (s == 0) hipLaunchKernelGGL((msssim_stats_kernel<true>), grid, block, 0, stream, sa);
        else        hipLaunchKernelGGL((msssim_stats_kernel<false>), grid, block, 0, stream, sa);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (s + 1 == scales) break;
        MsDownArgs da;
        da.descs = descs_dev;
        da.src = cur;
        da.dst = s == 0 ? planes : cur + (size_t)count * w * h;
        da.sw = w; da.sh = h;
        da.dw = ms_dim(width, s + 1); da.dh = ms_dim(height, s + 1);
        da.row_blocks = (da.dw + 2 * kThreads - 1) / (2 * kThreads);
        const dim3 dgrid((uint32_t)((uint64_t)count * da.dh * da.row_blocks));
        if (s == 0) hipLaunchKernelGGL((msssim_downsample_kernel<true>), dgrid, block, 0, stream, da);
        else        hipLaunchKernelGGL((msssim_downsample_kernel<false>), dgrid, block, 0, stream, da);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        cur = da.dst;
    }
    ra.partials = partials;
    ra.sums = reinterpret_cast<d2*>(sums_dev);
    ra.part_stride = tiles;
    ra.scales = scales;
    hipLaunchKernelGGL(msssim_reduce_kernel, dim3(count * scales), block, 0, stream, ra);
    return hipGetLastError();
}

} // namespace ssim_hip
