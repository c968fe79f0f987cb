// ssimw_kernels.hip -- gfx950 kernels of the gradient of the SSIM MAP, for an upstream gradient given per pixel, behind
// rmgr_ssim_hip_enqueue_ssimf_map_grad (float32 samples) and rmgr_ssim_hip_enqueue_ssimh_map_grad (float16 / bfloat16 samples).  The
// definition they implement is in include/rmgr/ssim-hip.h; tests/ssimw_model.py restates it in float64 and restates the arithmetic
// below in fp32.
//
// This is the gradient flow of ssimf_kernels.hip (and, for 16-bit samples, of ssimh_kernels.hip: widen<TYPE> at the loads, narrow<TYPE>
// before a 2-byte store), copied, not included: those files' kernels are counted by their tests, and their bits are what this file is
// held to.  One thing differs: in step 3 the factor k that multiplies the partials is not the launch-uniform gOut / (W H) but the
// pixel's own gMap(p), read through the plane's descriptor.  Every other instruction is the same and the file is built with the same
// flags (-ffp-contract=off), so a plane whose every element is float(gOut / (W H)) gives the bits of ssimf_grad_kernel /
// ssimh_grad_kernel.
//
// Centring, tiles, summation orders: see the top of ssimf_kernels.hip and the comment above ssimf_grad_kernel.
#include "ssimw_kernels.h"
#include <cmath>

namespace ssim_hip {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

typedef const float __attribute__((address_space(1)))*    gptr_cf32;
typedef const uint16_t __attribute__((address_space(1)))* gptr_cu16;

__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float opaque(float v) { asm("" : "+v"(v)); return v; }

// TYPE: the samples' (and the gradient planes') encoding.
enum { kSWTypeF32 = 0, kSWTypeF16 = 1, kSWTypeBF16 = 2 };

template <int TYPE> struct Sample       { typedef uint16_t T; typedef PairHDesc Pair; typedef GradHDesc Grad; };
template <> struct Sample<kSWTypeF32>   { typedef float    T; typedef PairFDesc Pair; typedef GradFDesc Grad; };

// A stored sample -> float32, exactly (ssimh_kernels.hip).
template <int TYPE>
__device__ __forceinline__ float widen(typename Sample<TYPE>::T s)
{
    if constexpr (TYPE == kSWTypeF32)       return s;
    else if constexpr (TYPE == kSWTypeBF16) return __builtin_bit_cast(float, (uint32_t)s << 16);
    else                                    return (float)__builtin_bit_cast(_Float16, s);
}
// float32 -> the samples' encoding, one rounding to nearest-even (ssimh_kernels.hip).
template <int TYPE>
__device__ __forceinline__ typename Sample<TYPE>::T narrow(float v)
{
    if constexpr (TYPE == kSWTypeF32) {
        return v;
    } else if constexpr (TYPE == kSWTypeBF16) {
        const uint32_t u = __builtin_bit_cast(uint32_t, v);
        const uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;               // no carry out of a finite or infinite value
        return (uint16_t)((u & 0x7FFFFFFFu) > 0x7F800000u ? (u >> 16) | 0x0040u : r);   // NaN: quiet, never rounded into Inf
    } else {
        return __builtin_bit_cast(uint16_t, (_Float16)v);
    }
}

// Row pass of one position, centre tap first, the two dependent chains interleaved.
__device__ __forceinline__ void rows_pair(f2& hA, f2& hB, const f2 (&a)[6], const f2 (&b)[6], const float (&g)[6])
{
    hA = a[0] * f2{g[0], g[0]};
    hB = b[0] * f2{g[0], g[0]};
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        hA = fma_(a[k], f2{g[k], g[k]}, hA);
        hB = fma_(b[k], f2{g[k], g[k]}, hB);
    }
}

// ssimw_grad_kernel: one 256-lane workgroup = one 32 x 32 tile of gradient pixels at an absolute position; everything between the
// samples and the gradient stays in LDS.
//   1. the (widened,) centred samples (a', b') of the tile + 10 (52 x 52, edge-clamped coordinates) -> LDS;
//   2. row pass of (a', b') and (a'^2 + b'^2, a'b') on 52 rows x 42 columns, folded sums and tap order as the forward kernel;
//   3. column pass on the tile + 5 (42 x 42), in source-row order as the forward kernel; per pixel the SSIM terms and the weighted
//      partials k d_mu, k d_aa, k d_ab with k = gMap at that pixel, a plain fp32 product (k = 0 does not hide a NaN statistic) -> LDS;
//      a position outside the image holds 0 and reads nothing from gMap;
//   4. adjoint row pass (42 rows x 32 columns), 5. adjoint column pass (32 x 32), as gathers with the weights of ssimf_grad_kernel;
//   6. dLoss/da = Gt(k d_mu_a) + 2 a' Gt(k d_aa) + b' Gt(k d_ab), rounded once into a 16-bit encoding, one store per pixel.
// k needs no LDS: the work-item that computes a pixel's partials is the one that reads its k, and the load is issued ahead of the
// column pass, whose 22 LDS reads and 20 fused multiply-adds cover it.
enum { GT = kSFTile, GIN = GT + 20, GST = GT + 10 };

template <int TYPE>
struct KWArgs {
    const typename Sample<TYPE>::Pair* descs;
    const typename Sample<TYPE>::Grad* grads;
    const GradOutFDesc*                gouts;
    uint32_t width, height, tiles_x, tiles_y;
    float    c1, c2, range;
    float    gf[6], tail[6], total;
};

// w(q, j) of the adjoint passes for an axis of n pixels (ssimf_kernels.hip).
__device__ __forceinline__ float adjoint_weight(int q, int n, int j, const float (&g)[6], const float (&tail)[6], float total)
{
    const int aj = j < 0 ? -j : j;
    float w = g[aj];
    if (q == 0) w = j >= 0 ? tail[aj] : 0.0f;
    if (q == n - 1) w = j <= 0 ? tail[aj] : 0.0f;
    if (n == 1) w = j == 0 ? total : 0.0f;
    return w;
}

// WHICH: 1 dLoss/dA, 2 dLoss/dB, 3 both.  The statistics are computed in the same (a, b) order in all three, so a gradient has
// the same bits alone and together with the other.
template <int TYPE, int WHICH>
__global__ __launch_bounds__(256)
void ssimw_grad_kernel(const KWArgs<TYPE> args)
{
    typedef const typename Sample<TYPE>::T __attribute__((address_space(1)))* gptr_cs;
    typedef typename Sample<TYPE>::T __attribute__((address_space(1)))*       gptr_s;
    constexpr int NP = WHICH == 3 ? 4 : 3;                       // partial planes: d_mu (of A, or of the one wanted), d_aa, d_ab, d_mu of B
    constexpr int XN = 2 * GIN * GIN > NP * GST * GST ? 2 * GIN * GIN : NP * GST * GST;
    constexpr int YN = 4 * GIN * GST;                            // >= NP * GST * GT
    __shared__ __attribute__((aligned(16))) float lds[XN + YN];
    f2*    in  = reinterpret_cast<f2*>(lds);                     // [GIN][GIN] (a', b')
    float* P   = lds;                                            // [NP][GST][GST], after the row pass has consumed `in`
    f2*    Hab = reinterpret_cast<f2*>(lds + XN);                // [GIN][GST] row pass of (a', b')
    f2*    Hq  = Hab + GIN * GST;                                // [GIN][GST] row pass of (a'^2 + b'^2, a'b')
    float* Q   = lds + XN;                                       // [NP][GST][GT], after the column pass has consumed Hab, Hq

    const int tid = threadIdx.x;
    const int W = (int)args.width, H = (int)args.height;
    const uint32_t per_img = args.tiles_x * args.tiles_y;
    const uint32_t img = blockIdx.x / per_img, lin = blockIdx.x - img * per_img;
    const uint32_t ty = lin / args.tiles_x, tx = lin - ty * args.tiles_x;
    const int x0 = (int)(tx * GT), y0 = (int)(ty * GT);
    const typename Sample<TYPE>::Pair pd = args.descs[img];
    const typename Sample<TYPE>::Grad gd = args.grads[img];
    const GradOutFDesc go = args.gouts[img];
    const gptr_cs pa = (gptr_cs)pd.a, pb = (gptr_cs)pd.b;
    const gptr_cf32 pk = (gptr_cf32)go.g;
    const float gf[6] = {args.gf[0], args.gf[1], args.gf[2], args.gf[3], args.gf[4], args.gf[5]};
    const float tail[6] = {args.tail[0], args.tail[1], args.tail[2], args.tail[3], args.tail[4], args.tail[5]};

    f2 cen;                                                      // the strip column's centre (top of ssimf_kernels.hip)
    {
        const int xs = x0 & ~(kSFStripW - 1);
        const int64_t cx = xs + 64 < W ? xs + 64 : W - 1, cy = (H - 1) / 2;
        const float sa = widen<TYPE>(pa[cx * pd.a_step + cy * pd.a_stride]), sb = widen<TYPE>(pb[cx * pd.b_step + cy * pd.b_stride]);
        cen = f2{__builtin_fabsf(sa) <= args.range ? sa : 0.0f, __builtin_fabsf(sb) <= args.range ? sb : 0.0f};
    }

    // 1. samples
    for (int idx = tid; idx < GIN * GIN; idx += 256) {
        const int j = idx / GIN, i = idx - j * GIN;
        int x = x0 - 10 + i, y = y0 - 10 + j;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        const f2 v = {widen<TYPE>(pa[(int64_t)x * pd.a_step + (int64_t)y * pd.a_stride]), widen<TYPE>(pb[(int64_t)x * pd.b_step + (int64_t)y * pd.b_stride])};
        in[idx] = v - cen;
    }
    __syncthreads();

    // 2. row pass: H*[j][u] is the blur along x at image column x0 - 5 + u of source row y0 - 10 + j
    for (int idx = tid; idx < GIN * GST; idx += 256) {
        const int j = idx / GST, u = idx - j * GST;
        const f2* row = in + j * GIN + u;
        f2 ab[11], q[11];
#pragma unroll
        for (int t = 0; t < 11; ++t) {
            ab[t] = row[t];
            q[t] = f2{__builtin_fmaf(ab[t].y, ab[t].y, ab[t].x * ab[t].x), ab[t].x * ab[t].y};
        }
        const f2 sab[6] = {ab[5], ab[6] + ab[4], ab[7] + ab[3], ab[8] + ab[2], ab[9] + ab[1], ab[10] + ab[0]};
        const f2 sq[6] = {q[5], q[6] + q[4], q[7] + q[3], q[8] + q[2], q[9] + q[1], q[10] + q[0]};
        f2 hab, hq;
        rows_pair(hab, hq, sab, sq, gf);
        Hab[idx] = hab;
        Hq[idx] = hq;
    }
    __syncthreads();

    // 3. column pass, SSIM terms, partials weighted by the pixel's own k
    for (int idx = tid; idx < GST * GST; idx += 256) {
        const int v = idx / GST, u = idx - v * GST;
        const int px = x0 - 5 + u, py = y0 - 5 + v;
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (px >= 0 && px < W && py >= 0 && py < H) {
            const float k = pk[(int64_t)px * go.g_step + (int64_t)py * go.g_stride];      // in flight during the column pass
            const f2* cab = Hab + v * GST + u;
            const f2* cq = Hq + v * GST + u;
            f2 m = cab[0] * f2{gf[5], gf[5]}, e = cq[0] * f2{gf[5], gf[5]};
#pragma unroll
            for (int t = 1; t < 11; ++t) {
                const float w = gf[t < 5 ? 5 - t : t - 5];
                m = fma_(cab[t * GST], f2{w, w}, m);
                e = fma_(cq[t * GST], f2{w, w}, e);
            }
            // the forward kernel's terms (ssim_px2), then the derivative
            const float pc = opaque(m.x * m.y), tc = opaque(opaque(m.x * m.x) + opaque(m.y * m.y));
            const float sS = opaque(e.x - tc), sAB = opaque(e.y - pc);
            const float uA = m.x + cen.x, uB = m.y + cen.y;
            const float muAB = opaque(uA * uB), tm = opaque(opaque(uA * uA) + opaque(uB * uB));
            const float A1 = __builtin_fmaf(2.0f, muAB, args.c1), A2 = __builtin_fmaf(2.0f, sAB, args.c2);
            const float B1 = tm + args.c1, B2 = sS + args.c2;
            const float r1 = __builtin_amdgcn_rcpf(B1), r2 = __builtin_amdgcn_rcpf(B2);
            const float r12 = opaque(r1 * r2);
            const float ssim = opaque(opaque(A1 * A2) * r12);
            const float dab = opaque(opaque(2.0f * A1) * r12);
            const float daa = -opaque(ssim * r2);
            const float f1 = opaque(A2 * r12), f2_ = opaque(ssim * r1);
            const float dmA = opaque(opaque(opaque(opaque(2.0f * uB) * f1) - opaque(opaque(2.0f * uA) * f2_)) - opaque(opaque(2.0f * m.x) * daa)) - opaque(m.y * dab);
            const float dmB = opaque(opaque(opaque(opaque(2.0f * uA) * f1) - opaque(opaque(2.0f * uB) * f2_)) - opaque(opaque(2.0f * m.y) * daa)) - opaque(m.x * dab);
            d[0] = k * (WHICH == 2 ? dmB : dmA);
            d[1] = k * daa;
            d[2] = k * dab;
            d[3] = k * dmB;
        }
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) P[pl * GST * GST + idx] = d[pl];      // `in` is dead: every lane is past the barrier above
    }
    __syncthreads();

    // 4. adjoint row pass: Q[pl][v][x], x = tid % 32 for every position of this lane
    {
        const int x = tid & (GT - 1), qx = x0 + x;
        float wx[11];
#pragma unroll
        for (int j = -5; j <= 5; ++j) wx[j + 5] = adjoint_weight(qx, W, j, gf, tail, args.total);
        for (int idx = tid; idx < GST * GT; idx += 256) {
            const int v = idx / GT;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
                const float* src = P + pl * GST * GST + v * GST + x;
                float acc = src[0] * wx[0];
#pragma unroll
                for (int t = 1; t < 11; ++t) acc = __builtin_fmaf(src[t], wx[t], acc);
                Q[pl * GST * GT + idx] = acc;
            }
        }
    }
    __syncthreads();

    // 5. adjoint column pass, 6. the gradient
    for (int idx = tid; idx < GT * GT; idx += 256) {
        const int y = idx / GT, x = idx - y * GT;
        const int qx = x0 + x, qy = y0 + y;
        if (qx >= W || qy >= H) continue;
        float wy[11];
#pragma unroll
        for (int j = -5; j <= 5; ++j) wy[j + 5] = adjoint_weight(qy, H, j, gf, tail, args.total);
        float r[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            const float* src = Q + pl * GST * GT + y * GT + x;
            float acc = src[0] * wy[0];
#pragma unroll
            for (int t = 1; t < 11; ++t) acc = __builtin_fmaf(src[t * GT], wy[t], acc);
            r[pl] = acc;
        }
        const float a = widen<TYPE>(pa[(int64_t)qx * pd.a_step + (int64_t)qy * pd.a_stride]) - cen.x;
        const float b = widen<TYPE>(pb[(int64_t)qx * pd.b_step + (int64_t)qy * pd.b_stride]) - cen.y;
        if constexpr (WHICH != 2) {
            const float g = opaque(r[0] + opaque(opaque(2.0f * a) * r[1])) + opaque(b * r[2]);
            ((gptr_s)gd.ga)[(int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride] = narrow<TYPE>(g);
        }
        if constexpr (WHICH != 1) {
            const float g = opaque(r[WHICH == 3 ? 3 : 0] + opaque(opaque(2.0f * b) * r[1])) + opaque(a * r[2]);
            ((gptr_s)gd.gb)[(int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride] = narrow<TYPE>(g);
        }
    }
}

// the true 1-D Gaussian, sigma 1.5, normalised over the 11 taps, rounded to float: the engine's taps, centre first (16-bit samples: the
// fixed window)
void gaussian_taps(float (&gf)[6])
{
    double g[6], norm = 0.0;
    for (int i = 0; i <= 5; ++i) {
        g[i] = exp(-(double)(i * i) / (2.0 * 1.5 * 1.5));
        norm += (i == 0) ? g[i] : 2.0 * g[i];
    }
    for (int i = 0; i <= 5; ++i) gf[i] = (float)(g[i] / norm);
}

template <int TYPE>
hipError_t launch(uint32_t width, uint32_t height, uint32_t count, const typename Sample<TYPE>::Pair* descs_dev,
                  const typename Sample<TYPE>::Grad* grads_dev, const GradOutFDesc* gouts_dev, float data_range, const float* taps, int which,
                  hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!(data_range > 0.0f) || !std::isfinite(data_range) || which < 1 || which > 3 || count > ssimf_max_count(width, height)) return hipErrorInvalidValue;
    KWArgs<TYPE> ka;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.gouts = gouts_dev;
    ka.width = width; ka.height = height;
    ka.tiles_x = (width + kSFTile - 1) / kSFTile; ka.tiles_y = (height + kSFTile - 1) / kSFTile;
    ka.range = data_range;
    ssimf_constants(data_range, ka.c1, ka.c2);
    if (taps) { for (int i = 0; i < 6; ++i) ka.gf[i] = taps[i]; }      // the caller's window (float32 samples)
    else      gaussian_taps(ka.gf);
    // tail[d] = g_d + ... + g_5 and the sum of all eleven taps: sums of the float taps in double, rounded once
    double t = 0.0;
    for (int i = 5; i >= 0; --i) { t += (double)ka.gf[i]; ka.tail[i] = (float)t; }
    ka.total = (float)(2.0 * t - (double)ka.gf[0]);
    const dim3 grid((uint32_t)((uint64_t)ka.tiles_x * ka.tiles_y * count)), block(256);
    if (which == 1)      hipLaunchKernelGGL((ssimw_grad_kernel<TYPE, 1>), grid, block, 0, stream, ka);
    else if (which == 2) hipLaunchKernelGGL((ssimw_grad_kernel<TYPE, 2>), grid, block, 0, stream, ka);
    else                 hipLaunchKernelGGL((ssimw_grad_kernel<TYPE, 3>), grid, block, 0, stream, ka);
    return hipGetLastError();
}

} // namespace

hipError_t launch_ssimw_grad_f(uint32_t width, uint32_t height, uint32_t count, const PairFDesc* descs_dev, const GradFDesc* grads_dev,
                               const GradOutFDesc* gouts_dev, float data_range, const float (&taps)[6], int which, hipStream_t stream)
{
    return launch<kSWTypeF32>(width, height, count, descs_dev, grads_dev, gouts_dev, data_range, taps, which, stream);
}

hipError_t launch_ssimw_grad_h(uint32_t width, uint32_t height, uint32_t count, const PairHDesc* descs_dev, const GradHDesc* grads_dev,
                               int type, const GradOutFDesc* gouts_dev, float data_range, int which, hipStream_t stream)
{
    if (type == kSHTypeBF16) return launch<kSWTypeBF16>(width, height, count, descs_dev, grads_dev, gouts_dev, data_range, NULL, which, stream);
    if (type == kSHTypeF16)  return launch<kSWTypeF16>(width, height, count, descs_dev, grads_dev, gouts_dev, data_range, NULL, which, stream);
    return hipErrorInvalidValue;
}

} // namespace ssim_hip
