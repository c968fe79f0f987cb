// ssim3hk_kernels.hip -- gfx950 kernels of SSIM on float16 / bfloat16 VOLUMES under a window of 3, 5, 7 or 9 taps per axis (radius R = 1
// .. 4) and of its gradient for both upstream forms, behind the rmgr_ssim_hip_*_ssim3h_win* entries.  The definition is in
// include/rmgr/ssim-hip.h: ssim3f_win's, applied to the samples widened to float32, with the gradient rounded once into the samples'
// encoding.  Windows of 11 taps run on the kernels of ssim3h_kernels.hip with the window's taps.
//
// This is the flow of ssim3k_kernels.hip, copied -- not included: that file's kernels are counted and budgeted by its tests -- and
// templated on the encoding as well as the radius: the same tiles, LDS planes, x / y passes, register rings, cells, chunks, coefficient
// volumes and adjoint weights, built with the same flags (-ffp-contract=off).  Two things differ, exactly as ssim3h_kernels.hip differs
// from ssim3f_kernels.hip:
//  * how a sample gets into a register: a 2-byte load and an exact widening (widen<TYPE>: bfloat16 is the upper half of a float32, a
//    shift; float16 goes through the hardware convert, which keeps subnormals and maps NaN and Inf to NaN and Inf).  That is fetch() of
//    the walks, centre_of, and the adjoint's re-read of a and b at the output voxel.  From `f2{va, vb} - cen` on every instruction is
//    ssim3k's, which is what gives value, map, sums, coefficient volumes and the float32 gradient the bits of ssim3k on the widened volumes;
//  * how a gradient voxel leaves one: narrow<TYPE> rounds the float32 value once, to nearest-even, and a 2-byte store writes it
//    (float16: the hardware convert, subnormals kept, overflow to Inf; bfloat16: integer rounding of the bit pattern, NaN kept NaN).
// The coefficient volumes, the map and the upstream gradient (scalar or per voxel) stay float32; the per-volume reduction is
// ssim3f_kernels.hip's own kernel (launch_ssim3f_reduce).
//
//  * ssim3hk_walk_kernel<TYPE, R, MODE>: ssim3k_walk_kernel<R, MODE>.  MODE 0: value, map, sums.  MODE 1 / 2 / 3: the coefficient volumes
//    of dLoss/dA, dLoss/dB, both -- for both upstream forms, by a branch on a kernel argument.
//  * ssim3hk_adjoint_kernel<TYPE, R, WHICH>: ssim3k_adjoint_kernel<R, WHICH>.
// Chunks, centring, cells and the adjoint weights: see the tops of ssim3k_kernels.hip and ssim3f_kernels.hip; the rules are the same, on
// the widened samples, and none of them depends on the size of a sample.
#include "ssim3hk_kernels.h"

namespace ssim_hip {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

typedef const float __attribute__((address_space(1)))*    gptr_cf32;
typedef float __attribute__((address_space(1)))*          gptr_f32;
typedef double __attribute__((address_space(1)))*         gptr_f64;
typedef const uint16_t __attribute__((address_space(1)))* gptr_cu16;
typedef uint16_t __attribute__((address_space(1)))*       gptr_u16;

__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float opaque(float v) { asm("" : "+v"(v)); return v; }

// A stored sample -> float32, exactly (ssim3h_kernels.hip: widen).
template <int TYPE>
__device__ __forceinline__ float widen(uint16_t s)
{
    if constexpr (TYPE == kSHTypeBF16) return __builtin_bit_cast(float, (uint32_t)s << 16);
    else                               return (float)__builtin_bit_cast(_Float16, s);
}
// float32 -> the samples' encoding, one rounding to nearest-even (ssim3h_kernels.hip: narrow).
template <int TYPE>
__device__ __forceinline__ uint16_t narrow(float v)
{
    if constexpr (TYPE == kSHTypeBF16) {
        const uint32_t u = __builtin_bit_cast(uint32_t, v);
        const uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;               // no carry out of a finite or infinite value
        return (uint16_t)((u & 0x7FFFFFFFu) > 0x7F800000u ? (u >> 16) | 0x0040u : r);   // NaN: quiet, never rounded into Inf
    } else {
        return __builtin_bit_cast(uint16_t, (_Float16)v);
    }
}

enum { T = kS3Tile, MAXR = 4 };

// The planes of radius R: the staged tile + R, the x pass's rows, loads and x-pass positions per lane.
template <int R> struct Shape {
    enum { TIN = T + 2 * R, NIN = TIN * TIN, NROW = TIN * T, NLOAD = (NIN + 255) / 256, NXP = (NROW + 255) / 256, NT = 2 * R + 1 };
};

struct K3HKArgs {
    const Pair3HDesc*    descs;
    const Grad3HDesc*    grads;
    const float*         g_out;       // the scalar upstream form, or NULL
    const GradOut3FDesc* gouts;       // the per-voxel upstream form (g_out == NULL)
    uint32_t width, height, depth, tiles_x, tiles_y, chunks, chunk_slices, cells_z;
    double*  partials;            // [volume][cell_z][tile_y][tile_x]
    float*   coef;                // [volume][plane][z][y][x]
    float    c1, c2, range;
    float    gf[MAXR + 1], tail[MAXR + 1], total;
};

// The workgroup's place: volume-major, then z-chunk, then tile row, then tile column (ssim3f_kernels.hip: place_of).
struct Place { uint32_t vol; int x0, y0, z0, z_end; uint32_t tx, ty; };

__device__ __forceinline__ Place place_of(const K3HKArgs& args)
{
    const uint32_t tiles = args.tiles_x * args.tiles_y, per_vol = tiles * args.chunks;
    Place p;
    p.vol = blockIdx.x / per_vol;
    const uint32_t rem = blockIdx.x - p.vol * per_vol, chunk = rem / tiles, lin = rem - chunk * tiles;
    p.ty = lin / args.tiles_x; p.tx = lin - p.ty * args.tiles_x;
    p.x0 = (int)(p.tx * T); p.y0 = (int)(p.ty * T);
    const uint64_t z0 = (uint64_t)chunk * args.chunk_slices, z1 = z0 + args.chunk_slices;
    p.z0 = (int)z0;
    p.z_end = (int)(z1 < args.depth ? z1 : args.depth);
    return p;
}

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// The volume's centre: the widened sample at ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2) when its magnitude is at most dataRange, else 0.
template <int TYPE>
__device__ __forceinline__ f2 centre_of(const Pair3HDesc& pd, int W, int H, int D, float range)
{
    const int64_t cx = (W - 1) / 2, cy = (H - 1) / 2, cz = (D - 1) / 2;
    const float sa = widen<TYPE>(((gptr_cu16)pd.a)[cx * pd.a_step + cy * pd.a_stride + cz * pd.a_slice]);
    const float sb = widen<TYPE>(((gptr_cu16)pd.b)[cx * pd.b_step + cy * pd.b_stride + cz * pd.b_slice]);
    return f2{__builtin_fabsf(sa) <= range ? sa : 0.0f, __builtin_fabsf(sb) <= range ? sb : 0.0f};
}

// MODE 0: value, map, sums.  MODE 1 / 2 / 3: the coefficient volumes of dLoss/dA, dLoss/dB, both.  The statistics are computed in the
// same order in all four.
template <int TYPE, int R, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3hk_walk_kernel(const K3HKArgs args)
{
    typedef Shape<R> S;
    constexpr int TIN = S::TIN, NIN = S::NIN, NROW = S::NROW, NLOAD = S::NLOAD, NT = S::NT;
    constexpr int NP = MODE == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) f2 inAB[NIN];     // (a', b') of the tile + R
    __shared__ __attribute__((aligned(16))) f2 inQ[NIN];      // (a'^2 + b'^2, a'b')
    __shared__ __attribute__((aligned(16))) f2 Hab[NROW];     // x pass, 16 + 2R rows x 16 columns
    __shared__ __attribute__((aligned(16))) f2 Hq[NROW];
    __shared__ double red[4];

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const Pair3HDesc pd = args.descs[pl.vol];
    const gptr_cu16 pa = (gptr_cu16)pd.a, pb = (gptr_cu16)pd.b;
    float gf[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) gf[i] = args.gf[i];
    const f2 cen = centre_of<TYPE>(pd, W, H, D, args.range);

    // staging positions: element idx of the plane is voxel (clamp(x0 - R + idx % TIN), clamp(y0 - R + idx / TIN))
    int sp[NLOAD];
    int64_t offA[NLOAD], offB[NLOAD];
#pragma unroll
    for (int t = 0; t < NLOAD; ++t) {
        int idx = tid + 256 * t;
        idx = idx < NIN ? idx : NIN - 1;
        const int j = idx / TIN, i = idx - j * TIN;
        const int64_t x = clampi(pl.x0 - R + i, W), y = clampi(pl.y0 - R + j, H);
        sp[t] = idx;
        offA[t] = x * pd.a_step + y * pd.a_stride;
        offB[t] = x * pd.b_step + y * pd.b_stride;
    }
    float va[NLOAD], vb[NLOAD];
    auto fetch = [&](int s) {
        const int64_t zc = clampi(s, D);
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            va[t] = widen<TYPE>(pa[offA[t] + zc * pd.a_slice]);
            vb[t] = widen<TYPE>(pb[offB[t] + zc * pd.b_slice]);
        }
    };

    const int qx = pl.x0 + lx, qy = pl.y0 + ly;
    const bool inside = qx < W && qy < H;
    const uint64_t voxels = (uint64_t)W * (uint64_t)H * (uint64_t)D;
    // the weight of the voxel's partial derivatives: one float for the volume, or the lane's column of gMap
    float k_vol = 0.0f;
    gptr_cf32 pg = nullptr;
    int64_t offG = 0, g_slice = 0;
    if constexpr (MODE != 0) {
        if (args.g_out) {
            k_vol = (float)((double)((gptr_cf32)args.g_out)[pl.vol] / ((double)W * (double)H * (double)D));
        } else {
            const GradOut3FDesc go = args.gouts[pl.vol];
            pg = (gptr_cf32)go.g;
            offG = inside ? (int64_t)qx * go.g_step + (int64_t)qy * go.g_stride : 0;
            g_slice = go.g_slice;
        }
    }

    f2 accAB[NT], accQ[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) accAB[i] = accQ[i] = f2{0.0f, 0.0f};
    double colsum = 0.0;

    fetch(pl.z0 - R);
#pragma unroll 1
    for (int s = pl.z0 - R; s < pl.z_end + R; ++s) {
        // 0. k of the slice this iteration finishes, z = s - R < z_end; no address is formed outside the volume or during the warm-up
        const int z = s - R;
        float k = k_vol;
        if constexpr (MODE != 0) {
            if (pg && inside && z >= pl.z0)
                k = pg[offG + (int64_t)z * g_slice];
        }
        // 1. the slice's centred samples and products -> LDS; the next slice's samples -> registers
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            const f2 ab = f2{va[t], vb[t]} - cen;
            inAB[sp[t]] = ab;
            inQ[sp[t]] = f2{__builtin_fmaf(ab.y, ab.y, ab.x * ab.x), ab.x * ab.y};
        }
        fetch(s + 1);
        __syncthreads();
        // 2. x pass: folded sums, centre tap first
#pragma unroll
        for (int it = 0; it < S::NXP; ++it) {
            const int idx = tid + 256 * it;
            if (idx < NROW) {
                const int j = idx >> 4, u = idx & (T - 1);
                const f2* rab = inAB + j * TIN + u;
                const f2* rq = inQ + j * TIN + u;
                f2 hab = rab[R] * f2{gf[0], gf[0]}, hq = rq[R] * f2{gf[0], gf[0]};
#pragma unroll
                for (int i = 1; i <= R; ++i) {
                    hab = fma_(rab[R + i] + rab[R - i], f2{gf[i], gf[i]}, hab);
                    hq = fma_(rq[R + i] + rq[R - i], f2{gf[i], gf[i]}, hq);
                }
                Hab[idx] = hab;
                Hq[idx] = hq;
            }
        }
        __syncthreads();
        // 3. y pass of the lane's column, rows y - R .. y + R in that order, the first product plain
        f2 m, e;
        {
            const f2* cab = Hab + ly * T + lx;
            const f2* cq = Hq + ly * T + lx;
            m = cab[0] * f2{gf[R], gf[R]};
            e = cq[0] * f2{gf[R], gf[R]};
#pragma unroll
            for (int t = 1; t < NT; ++t) {
                const float w = gf[t < R ? R - t : t - R];
                m = fma_(cab[t * T], f2{w, w}, m);
                e = fma_(cq[t * T], f2{w, w}, e);
            }
        }
        // 4. z pass: ring entry i is the running sum of output slice s - R + i
#pragma unroll
        for (int i = 0; i < NT - 1; ++i) {
            const float w = gf[i < R ? R - i : i - R];
            accAB[i] = fma_(m, f2{w, w}, accAB[i + 1]);
            accQ[i] = fma_(e, f2{w, w}, accQ[i + 1]);
        }
        accAB[NT - 1] = m * f2{gf[R], gf[R]};
        accQ[NT - 1] = e * f2{gf[R], gf[R]};
        if (z < pl.z0) continue;
        // 5. ring entry 0 is the finished slice z
        const f2 mm = accAB[0], ee = accQ[0];
        const float pc = opaque(mm.x * mm.y), tc = opaque(opaque(mm.x * mm.x) + opaque(mm.y * mm.y));
        const float sS = opaque(ee.x - tc), sAB = opaque(ee.y - pc);
        const float uA = mm.x + cen.x, uB = mm.y + cen.y;
        const float muAB = opaque(uA * uB), tm = opaque(opaque(uA * uA) + opaque(uB * uB));
        const float A1 = __builtin_fmaf(2.0f, muAB, args.c1), A2 = __builtin_fmaf(2.0f, sAB, args.c2);
        const float B1 = tm + args.c1, B2 = sS + args.c2;
        if constexpr (MODE == 0) {
            const float v = opaque(A1 * A2) * __builtin_amdgcn_rcpf(opaque(B1 * B2));
            if (inside) {
                colsum += (double)v;
                if (pd.map)
                    ((gptr_f32)pd.map)[(int64_t)qx * pd.map_step + (int64_t)qy * pd.map_stride + (int64_t)z * pd.map_slice] = v;
            }
            if (((z + 1) & (kS3CellZ - 1)) == 0 || z == pl.z_end - 1) {       // the cell is complete: 64-lane butterflies, then the four waves in order
                double t = colsum;
                colsum = 0.0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
                if ((tid & 63) == 0) red[tid >> 6] = t;
                __syncthreads();
                if (tid == 0) {
                    const uint64_t cell = (((uint64_t)pl.vol * args.cells_z + (uint32_t)z / kS3CellZ) * args.tiles_y + pl.ty) * args.tiles_x + pl.tx;
                    ((gptr_f64)args.partials)[cell] = (red[0] + red[1]) + (red[2] + red[3]);
                }
            }
        } else {
            const float r1 = __builtin_amdgcn_rcpf(B1), r2 = __builtin_amdgcn_rcpf(B2);
            const float r12 = opaque(r1 * r2);
            const float ssim = opaque(opaque(A1 * A2) * r12);
            const float dab = opaque(opaque(2.0f * A1) * r12);
            const float daa = -opaque(ssim * r2);
            const float f1 = opaque(A2 * r12), f2_ = opaque(ssim * r1);
            const float dmA = opaque(opaque(opaque(opaque(2.0f * uB) * f1) - opaque(opaque(2.0f * uA) * f2_)) - opaque(opaque(2.0f * mm.x) * daa)) - opaque(mm.y * dab);
            const float dmB = opaque(opaque(opaque(opaque(2.0f * uA) * f1) - opaque(opaque(2.0f * uB) * f2_)) - opaque(opaque(2.0f * mm.y) * daa)) - opaque(mm.x * dab);
            if (inside) {
                const gptr_f32 out = (gptr_f32)args.coef + (uint64_t)pl.vol * NP * voxels + ((uint64_t)z * H + qy) * W + qx;
                out[0] = k * (MODE == 2 ? dmB : dmA);
                out[voxels] = k * daa;
                out[2 * voxels] = k * dab;
                if constexpr (MODE == 3) out[3 * voxels] = k * dmB;
            }
        }
    }
}

// What gradient voxel q of an axis of n voxels collects from p = q + j (ssim3k_kernels.hip: adjoint_weight).
template <int R>
__device__ __forceinline__ float adjoint_weight(int q, int n, int j, const float (&g)[R + 1], const float (&tail)[R + 1], float total)
{
    const int aj = j < 0 ? -j : j;
    float w = g[aj];
    if (q == 0) w = j >= 0 ? tail[aj] : 0.0f;
    if (q == n - 1) w = j <= 0 ? tail[aj] : 0.0f;
    if (n == 1) w = j == 0 ? total : 0.0f;
    return w;
}

// WHICH: 1 dLoss/dA, 2 dLoss/dB, 3 both.  Every pass is a gather in the order j = -R .. R, the first product plain, the others fused; a
// coefficient outside the volume is 0 (the clamp is in the weights).  The float32 gradient voxel is rounded once on its way out.
template <int TYPE, int R, int WHICH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3hk_adjoint_kernel(const K3HKArgs args)
{
    typedef Shape<R> S;
    constexpr int TIN = S::TIN, NIN = S::NIN, NROW = S::NROW, NLOAD = S::NLOAD, NT = S::NT;
    constexpr int NP = WHICH == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) float P[NP][NIN];      // the slice's coefficients on the tile + R
    __shared__ __attribute__((aligned(16))) float Q[NP][NROW];     // adjoint x pass, 16 + 2R rows x 16 columns

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const Pair3HDesc pd = args.descs[pl.vol];
    const Grad3HDesc gd = args.grads[pl.vol];
    float gf[R + 1], tail[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) { gf[i] = args.gf[i]; tail[i] = args.tail[i]; }
    const f2 cen = centre_of<TYPE>(pd, W, H, D, args.range);
    const uint64_t plane = (uint64_t)W * (uint64_t)H, voxels = plane * (uint64_t)D;
    const gptr_cf32 coef = (gptr_cf32)args.coef + (uint64_t)pl.vol * NP * voxels;

    int sp[NLOAD];
    int64_t off[NLOAD];            // < 0: outside the volume
#pragma unroll
    for (int t = 0; t < NLOAD; ++t) {
        int idx = tid + 256 * t;
        idx = idx < NIN ? idx : NIN - 1;
        const int j = idx / TIN, i = idx - j * TIN;
        const int x = pl.x0 - R + i, y = pl.y0 - R + j;
        sp[t] = idx;
        off[t] = (x >= 0 && x < W && y >= 0 && y < H) ? (int64_t)y * W + x : -1;
    }
    float v[NP][NLOAD];
    auto fetch = [&](int s) {
        const bool zok = s >= 0 && s < D;
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            const bool ok = zok && off[t] >= 0;
            const uint64_t at = ok ? (uint64_t)s * plane + (uint64_t)off[t] : 0;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float c = coef[(uint64_t)p * voxels + at];
                v[p][t] = ok ? c : 0.0f;
            }
        }
    };

    const int qx = pl.x0 + lx, qy = pl.y0 + ly;
    const bool inside = qx < W && qy < H;
    float wx[NT], wy[NT];
#pragma unroll
    for (int j = -R; j <= R; ++j) {
        wx[j + R] = adjoint_weight<R>(qx, W, j, gf, tail, args.total);
        wy[j + R] = adjoint_weight<R>(qy, H, j, gf, tail, args.total);
    }

    float acc[NP][NT];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[p][i] = 0.0f;

    fetch(pl.z0 - R);
#pragma unroll 1
    for (int s = pl.z0 - R; s < pl.z_end + R; ++s) {
#pragma unroll
        for (int t = 0; t < NLOAD; ++t)
#pragma unroll
            for (int p = 0; p < NP; ++p) P[p][sp[t]] = v[p][t];
        fetch(s + 1);
        __syncthreads();
        // adjoint x pass; the column of every one of a lane's positions is lx
#pragma unroll
        for (int it = 0; it < S::NXP; ++it) {
            const int idx = tid + 256 * it;
            if (idx < NROW) {
                const int j = idx >> 4;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const float* src = &P[p][j * TIN + lx];
                    float a = src[0] * wx[0];
#pragma unroll
                    for (int t = 1; t < NT; ++t) a = __builtin_fmaf(src[t], wx[t], a);
                    Q[p][idx] = a;
                }
            }
        }
        __syncthreads();
        // adjoint y pass, then the z pass: ring entry i is gradient slice q = s - R + i, which collects this slice as j = R - i
        float wz[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) wz[i] = adjoint_weight<R>(s - R + i, D, R - i, gf, tail, args.total);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float* src = &Q[p][ly * T + lx];
            float r = src[0] * wy[0];
#pragma unroll
            for (int t = 1; t < NT; ++t) r = __builtin_fmaf(src[t * T], wy[t], r);
#pragma unroll
            for (int i = 0; i < NT - 1; ++i) acc[p][i] = __builtin_fmaf(r, wz[i], acc[p][i + 1]);
            acc[p][NT - 1] = r * wz[NT - 1];
        }
        const int z = s - R;
        if (z < pl.z0 || !inside) continue;
        const float a = widen<TYPE>(((gptr_cu16)pd.a)[(int64_t)qx * pd.a_step + (int64_t)qy * pd.a_stride + (int64_t)z * pd.a_slice]) - cen.x;
        const float b = widen<TYPE>(((gptr_cu16)pd.b)[(int64_t)qx * pd.b_step + (int64_t)qy * pd.b_stride + (int64_t)z * pd.b_slice]) - cen.y;
        if constexpr (WHICH != 2) {
            const float g = opaque(acc[0][0] + opaque(opaque(2.0f * a) * acc[1][0])) + opaque(b * acc[2][0]);
            ((gptr_u16)gd.ga)[(int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride + (int64_t)z * gd.ga_slice] = narrow<TYPE>(g);
        }
        if constexpr (WHICH != 1) {
            const float g = opaque(acc[WHICH == 3 ? 3 : 0][0] + opaque(opaque(2.0f * b) * acc[1][0])) + opaque(a * acc[2][0]);
            ((gptr_u16)gd.gb)[(int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride + (int64_t)z * gd.gb_slice] = narrow<TYPE>(g);
        }
    }
}

// What every launch of this file takes by value.  C1, C2 and the refusals (data_range, geometry) are ssim3f_walk_constants'.
bool fill_args(K3HKArgs& ka, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, int type, float data_range)
{
    Walk3FConstants wc;
    if (radius < 1 || radius > MAXR || (type != kSHTypeF16 && type != kSHTypeBF16) || !ssim3f_walk_constants(geo, data_range, wc)) return false;
    ka.descs = NULL; ka.grads = NULL; ka.g_out = NULL; ka.gouts = NULL; ka.partials = NULL; ka.coef = NULL;
    ka.width = geo.width; ka.height = geo.height; ka.depth = geo.depth;
    ka.tiles_x = geo.tiles_x; ka.tiles_y = geo.tiles_y; ka.chunks = geo.chunks; ka.chunk_slices = geo.chunk_slices; ka.cells_z = geo.cells_z;
    ka.c1 = wc.c1; ka.c2 = wc.c2; ka.range = data_range;
    float tail[kSKMaxRadius + 1];
    window_tails(radius, gf, tail, ka.total);
    for (int i = 0; i <= MAXR; ++i) { ka.gf[i] = gf[i]; ka.tail[i] = tail[i]; }
    return true;
}

dim3 grid_of(const Geometry3F& geo) { return dim3((uint32_t)((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count)); }

template <int TYPE, int R>
hipError_t launch_walk(const K3HKArgs& ka, int mode, dim3 grid, hipStream_t stream)
{
    const dim3 block(256);
    if (mode == 0)      hipLaunchKernelGGL((ssim3hk_walk_kernel<TYPE, R, 0>), grid, block, 0, stream, ka);
    else if (mode == 1) hipLaunchKernelGGL((ssim3hk_walk_kernel<TYPE, R, 1>), grid, block, 0, stream, ka);
    else if (mode == 2) hipLaunchKernelGGL((ssim3hk_walk_kernel<TYPE, R, 2>), grid, block, 0, stream, ka);
    else                hipLaunchKernelGGL((ssim3hk_walk_kernel<TYPE, R, 3>), grid, block, 0, stream, ka);
    return hipGetLastError();
}

template <int TYPE, int R>
hipError_t launch_adjoint(const K3HKArgs& ka, int which, dim3 grid, hipStream_t stream)
{
    const dim3 block(256);
    if (which == 1)      hipLaunchKernelGGL((ssim3hk_adjoint_kernel<TYPE, R, 1>), grid, block, 0, stream, ka);
    else if (which == 2) hipLaunchKernelGGL((ssim3hk_adjoint_kernel<TYPE, R, 2>), grid, block, 0, stream, ka);
    else                 hipLaunchKernelGGL((ssim3hk_adjoint_kernel<TYPE, R, 3>), grid, block, 0, stream, ka);
    return hipGetLastError();
}

template <int TYPE>
hipError_t launch_walk_of(uint32_t radius, const K3HKArgs& ka, int mode, dim3 grid, hipStream_t stream)
{
    switch (radius) {
    case 1:  return launch_walk<TYPE, 1>(ka, mode, grid, stream);
    case 2:  return launch_walk<TYPE, 2>(ka, mode, grid, stream);
    case 3:  return launch_walk<TYPE, 3>(ka, mode, grid, stream);
    default: return launch_walk<TYPE, 4>(ka, mode, grid, stream);
    }
}

template <int TYPE>
hipError_t launch_adjoint_of(uint32_t radius, const K3HKArgs& ka, int which, dim3 grid, hipStream_t stream)
{
    switch (radius) {
    case 1:  return launch_adjoint<TYPE, 1>(ka, which, grid, stream);
    case 2:  return launch_adjoint<TYPE, 2>(ka, which, grid, stream);
    case 3:  return launch_adjoint<TYPE, 3>(ka, which, grid, stream);
    default: return launch_adjoint<TYPE, 4>(ka, which, grid, stream);
    }
}

} // namespace

hipError_t launch_ssim3hk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3HDesc* descs_dev, int type,
                          float data_range, double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3HKArgs ka;
    if (!fill_args(ka, radius, gf, geo, type, data_range)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.partials = partials;
    const hipError_t e = type == kSHTypeBF16 ? launch_walk_of<kSHTypeBF16>(radius, ka, 0, grid_of(geo), stream)
                                             : launch_walk_of<kSHTypeF16>(radius, ka, 0, grid_of(geo), stream);
    if (e != hipSuccess) return e;
    return launch_ssim3f_reduce(geo, partials, sums, stream);
}

hipError_t launch_ssim3hk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3HDesc* descs_dev,
                               const Grad3HDesc* grads_dev, int type, const float* g_out, const GradOut3FDesc* gouts_dev, float data_range,
                               int which, float* coef, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3HKArgs ka;
    if (which < 1 || which > 3 || (g_out == NULL) == (gouts_dev == NULL) || !fill_args(ka, radius, gf, geo, type, data_range)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.gouts = gouts_dev; ka.coef = coef;
    const bool bf = type == kSHTypeBF16;
    const hipError_t e = bf ? launch_walk_of<kSHTypeBF16>(radius, ka, which, grid_of(geo), stream)
                            : launch_walk_of<kSHTypeF16>(radius, ka, which, grid_of(geo), stream);
    if (e != hipSuccess) return e;
    return bf ? launch_adjoint_of<kSHTypeBF16>(radius, ka, which, grid_of(geo), stream)
              : launch_adjoint_of<kSHTypeF16>(radius, ka, which, grid_of(geo), stream);
}

} // namespace ssim_hip
