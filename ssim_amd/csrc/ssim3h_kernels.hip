// ssim3h_kernels.hip -- gfx950 kernels of SSIM on float16 / bfloat16 VOLUMES (a three-dimensional window), of its gradient and of the
// gradient of its map for a per-voxel upstream gradient, behind rmgr_ssim_hip_enqueue_ssim3h, rmgr_ssim_hip_compute_ssim3h_device / _host,
// rmgr_ssim_hip_enqueue_ssim3h_grad and rmgr_ssim_hip_enqueue_ssim3h_map_grad.  The definition they implement is in
// include/rmgr/ssim-hip.h: ssim3f's, applied to the samples widened to float32, with the gradient rounded once into the samples' encoding.
//
// This is the flow of ssim3f_kernels.hip and ssim3w_kernels.hip, copied, not included (those files' kernels are counted and budgeted by
// the tests), and templated on the encoding: the same tiles, LDS planes, x / y passes, register rings, cells, chunks, coefficient
// volumes and adjoint weights.  Two things differ, exactly as ssimh_kernels.hip differs from ssimf_kernels.hip:
//  * how a sample gets into a register: a 2-byte load and an exact widening (widen<TYPE>: bfloat16 is the upper half of a float32, a
//    shift; float16 goes through the hardware convert, which keeps subnormals and maps NaN and Inf to NaN and Inf).  Byte offsets scale
//    by 2.  That is fetch() of the walks, centre_of, and the adjoint's re-read of a and b at the output voxel.  From `f2{va, vb} - cen`
//    on every instruction is ssim3f's, built with the same flags (-ffp-contract=off), which is what gives value, map, sums, coefficient
//    volumes and the float32 gradient the bits of ssim3f on the widened volumes;
//  * how a gradient voxel leaves one: narrow<TYPE> rounds the float32 value once, to nearest-even, and a 2-byte store writes it
//    (float16: the hardware convert, subnormals kept, overflow to Inf; bfloat16: integer rounding of the bit pattern, NaN kept NaN).
// Loads and stores are the plain per-sample form: a base pointer is only 2-byte aligned, the strides are arbitrary, and the walks are
// VALU- and LDS-bound.  The coefficient volumes, the map and the upstream gradient (scalar or per voxel) stay float32; the per-volume
// reduction is ssim3f_kernels.hip's own kernel (launch_ssim3f_reduce).
//
//  * ssim3h_walk_kernel<TYPE, MODE>: ssim3f_walk_kernel<MODE>, MODE 0 (value, map, sums) and 1 / 2 / 3 (coefficient volumes, uniform k).
//  * ssim3h_mapwalk_kernel<TYPE, MODE>: ssim3w_walk_kernel<MODE>, MODE 1 / 2 / 3 with k = gMap(p) read per voxel.
//  * ssim3h_adjoint_kernel<TYPE, WHICH>: ssim3f_adjoint_kernel<WHICH>.
// Chunks, centring and the adjoint weights: see the top of ssim3f_kernels.hip; the rules are the same, on the widened samples.
#include "ssim3h_kernels.h"

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

// A stored sample -> float32, exactly (ssimh_kernels.hip: widen).
template <int TYPE>
__device__ __forceinline__ float widen(uint16_t s)
{
    if constexpr (TYPE == kSHTypeBF16) return __builtin_bit_cast(float, (uint32_t)s << 16);
    else                               return (float)__builtin_bit_cast(_Float16, s);
}
// float32 -> the samples' encoding, one rounding to nearest-even (ssimh_kernels.hip: narrow).
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

enum { T = kS3Tile, TIN = T + 10, NIN = TIN * TIN, NROW = TIN * T, NLOAD = (NIN + 255) / 256 };

struct K3HArgs {
    const Pair3HDesc*    descs;
    const Grad3HDesc*    grads;
    const GradOut3FDesc* gouts;   // the per-voxel upstream gradient (ssim3h_mapwalk_kernel)
    const float*         g_out;   // the per-volume upstream gradient (ssim3h_walk_kernel, MODE != 0)
    uint32_t width, height, depth, tiles_x, tiles_y, chunks, chunk_slices, cells_z;
    double*  partials;            // [volume][cell_z][tile_y][tile_x]
    float*   coef;                // [volume][plane][z][y][x]
    float    c1, c2, range;
    float    gf[6], tail[6], total;
};

// The workgroup's place: volume-major, then z-chunk, then tile row, then tile column.
struct Place { uint32_t vol; int x0, y0, z0, z_end; uint32_t tx, ty; };

__device__ __forceinline__ Place place_of(const K3HArgs& args)
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

// MODE 0: value, map, sums.  MODE 1 / 2 / 3: the coefficient volumes of dLoss/dA, dLoss/dB, both.  PERVOXEL: the weight k of the
// voxel's partial derivatives is gMap(p), read per voxel (MODE != 0), not the launch-uniform float(gOut / (W H D)).  The statistics are
// computed in the same order in all of them.
template <int TYPE, int MODE, bool PERVOXEL>
__device__ __forceinline__ void walk_body(const K3HArgs& args)
{
    constexpr int NP = MODE == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) f2 inAB[NIN];     // (a', b') of the tile + 5
    __shared__ __attribute__((aligned(16))) f2 inQ[NIN];      // (a'^2 + b'^2, a'b')
    __shared__ __attribute__((aligned(16))) f2 Hab[NROW];     // x pass, 26 rows x 16 columns
    __shared__ __attribute__((aligned(16))) f2 Hq[NROW];
    __shared__ double red[MODE == 0 ? 4 : 1];

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const Pair3HDesc pd = args.descs[pl.vol];
    const gptr_cu16 pa = (gptr_cu16)pd.a, pb = (gptr_cu16)pd.b;
    const float gf[6] = {args.gf[0], args.gf[1], args.gf[2], args.gf[3], args.gf[4], args.gf[5]};
    const f2 cen = centre_of<TYPE>(pd, W, H, D, args.range);

    // staging positions: element idx of the 26 x 26 plane is voxel (clamp(x0 - 5 + idx % 26), clamp(y0 - 5 + idx / 26))
    int sp[NLOAD];
    int64_t offA[NLOAD], offB[NLOAD];
#pragma unroll
    for (int t = 0; t < NLOAD; ++t) {
        int idx = tid + 256 * t;
        idx = idx < NIN ? idx : NIN - 1;
        const int j = idx / TIN, i = idx - j * TIN;
        const int64_t x = clampi(pl.x0 - 5 + i, W), y = clampi(pl.y0 - 5 + j, H);
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
    float k = 0.0f;
    gptr_cf32 pg = nullptr;
    int64_t offG = 0, sliceG = 0;
    if constexpr (PERVOXEL) {
        const GradOut3FDesc go = args.gouts[pl.vol];
        pg = (gptr_cf32)go.g;
        offG = inside ? (int64_t)qx * go.g_step + (int64_t)qy * go.g_stride : 0;      // the lane's column of gMap
        sliceG = go.g_slice;
    } else if constexpr (MODE != 0) {
        k = (float)((double)((gptr_cf32)args.g_out)[pl.vol] / ((double)W * (double)H * (double)D));
    }

    f2 accAB[11], accQ[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) accAB[i] = accQ[i] = f2{0.0f, 0.0f};
    double colsum = 0.0;

    fetch(pl.z0 - 5);
#pragma unroll 1
    for (int s = pl.z0 - 5; s < pl.z_end + 5; ++s) {
        const int z = s - 5;
        // 0. (PERVOXEL) k of the slice this iteration finishes, z = s - 5 < z_end; no address is formed outside the volume or during the
        //    warm-up; the load's latency sits under the LDS passes
        if constexpr (PERVOXEL) {
            k = 0.0f;
            if (inside && z >= pl.z0)
                k = pg[offG + (int64_t)z * sliceG];
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
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + 256 * it;
            if (idx < NROW) {
                const int j = idx >> 4, u = idx & (T - 1);
                const f2* rab = inAB + j * TIN + u;
                const f2* rq = inQ + j * TIN + u;
                f2 hab = rab[5] * f2{gf[0], gf[0]}, hq = rq[5] * f2{gf[0], gf[0]};
#pragma unroll
                for (int i = 1; i <= 5; ++i) {
                    hab = fma_(rab[5 + i] + rab[5 - i], f2{gf[i], gf[i]}, hab);
                    hq = fma_(rq[5 + i] + rq[5 - i], f2{gf[i], gf[i]}, hq);
                }
                Hab[idx] = hab;
                Hq[idx] = hq;
            }
        }
        __syncthreads();
        // 3. y pass of the lane's column, rows y - 5 .. y + 5 in that order, the first product plain
        f2 m, e;
        {
            const f2* cab = Hab + ly * T + lx;
            const f2* cq = Hq + ly * T + lx;
            m = cab[0] * f2{gf[5], gf[5]};
            e = cq[0] * f2{gf[5], gf[5]};
#pragma unroll
            for (int t = 1; t < 11; ++t) {
                const float w = gf[t < 5 ? 5 - t : t - 5];
                m = fma_(cab[t * T], f2{w, w}, m);
                e = fma_(cq[t * T], f2{w, w}, e);
            }
        }
        // 4. z pass: ring entry i is the running sum of output slice s - 5 + i
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const float w = gf[i < 5 ? 5 - i : i - 5];
            accAB[i] = fma_(m, f2{w, w}, accAB[i + 1]);
            accQ[i] = fma_(e, f2{w, w}, accQ[i + 1]);
        }
        accAB[10] = m * f2{gf[5], gf[5]};
        accQ[10] = e * f2{gf[5], gf[5]};
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

template <int TYPE, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3h_walk_kernel(const K3HArgs args)
{
    walk_body<TYPE, MODE, false>(args);
}

template <int TYPE, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3h_mapwalk_kernel(const K3HArgs args)
{
    static_assert(MODE >= 1 && MODE <= 3, "the value walk has no upstream gradient");
    walk_body<TYPE, MODE, true>(args);
}

// What gradient voxel q of an axis of n voxels collects from p = q + j (ssim3f_kernels.hip: adjoint_weight).
__device__ __forceinline__ float adjoint_weight(int q, int n, int j, const float (&g)[6], const float (&tail)[6], float total)
{
    const int aj = j < 0 ? -j : j;
    float w = g[aj];
    if (q == 0) w = j >= 0 ? tail[aj] : 0.0f;
    if (q == n - 1) w = j <= 0 ? tail[aj] : 0.0f;
    if (n == 1) w = j == 0 ? total : 0.0f;
    return w;
}

// WHICH: 1 dLoss/dA, 2 dLoss/dB, 3 both.  Every pass is a gather in the order j = -5 .. 5, the first product plain, the others fused; a
// coefficient outside the volume is 0 (the clamp is in the weights).  The float32 gradient voxel is rounded once on its way out.
template <int TYPE, int WHICH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3h_adjoint_kernel(const K3HArgs args)
{
    constexpr int NP = WHICH == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) float P[NP][NIN];      // the slice's coefficients on the tile + 5
    __shared__ __attribute__((aligned(16))) float Q[NP][NROW];     // adjoint x pass, 26 rows x 16 columns

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const Pair3HDesc pd = args.descs[pl.vol];
    const Grad3HDesc gd = args.grads[pl.vol];
    const float gf[6] = {args.gf[0], args.gf[1], args.gf[2], args.gf[3], args.gf[4], args.gf[5]};
    const float tail[6] = {args.tail[0], args.tail[1], args.tail[2], args.tail[3], args.tail[4], args.tail[5]};
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
        const int x = pl.x0 - 5 + i, y = pl.y0 - 5 + j;
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
    float wx[11], wy[11];
#pragma unroll
    for (int j = -5; j <= 5; ++j) {
        wx[j + 5] = adjoint_weight(qx, W, j, gf, tail, args.total);
        wy[j + 5] = adjoint_weight(qy, H, j, gf, tail, args.total);
    }

    float acc[NP][11];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 11; ++i) acc[p][i] = 0.0f;

    fetch(pl.z0 - 5);
#pragma unroll 1
    for (int s = pl.z0 - 5; s < pl.z_end + 5; ++s) {
#pragma unroll
        for (int t = 0; t < NLOAD; ++t)
#pragma unroll
            for (int p = 0; p < NP; ++p) P[p][sp[t]] = v[p][t];
        fetch(s + 1);
        __syncthreads();
        // adjoint x pass; the column of both of a lane's positions is lx
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + 256 * it;
            if (idx < NROW) {
                const int j = idx >> 4;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const float* src = &P[p][j * TIN + lx];
                    float a = src[0] * wx[0];
#pragma unroll
                    for (int t = 1; t < 11; ++t) a = __builtin_fmaf(src[t], wx[t], a);
                    Q[p][idx] = a;
                }
            }
        }
        __syncthreads();
        // adjoint y pass, then the z pass: ring entry i is gradient slice q = s - 5 + i, which collects this slice as j = 5 - i
        float wz[11];
#pragma unroll
        for (int i = 0; i < 11; ++i) wz[i] = adjoint_weight(s - 5 + i, D, 5 - i, gf, tail, args.total);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float* src = &Q[p][ly * T + lx];
            float r = src[0] * wy[0];
#pragma unroll
            for (int t = 1; t < 11; ++t) r = __builtin_fmaf(src[t * T], wy[t], r);
#pragma unroll
            for (int i = 0; i < 10; ++i) acc[p][i] = __builtin_fmaf(r, wz[i], acc[p][i + 1]);
            acc[p][10] = r * wz[10];
        }
        const int z = s - 5;
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

// The arguments every walk takes by value: geometry, C1, C2 and the taps of launch_ssim3f (ssim3f_walk_constants), and the adjoint's
// tail[d] = g_d + ... + g_5 and the sum of all eleven taps: sums of the float taps in double, rounded once (ssim3f_kernels.hip: fill_args).
bool fill_args(K3HArgs& ka, const Geometry3F& geo, int type, float data_range)
{
    Walk3FConstants wc;
    if ((type != kSHTypeF16 && type != kSHTypeBF16) || !ssim3f_walk_constants(geo, data_range, wc)) return false;
    ka.descs = NULL; ka.grads = NULL; ka.gouts = NULL; ka.g_out = NULL; ka.partials = NULL; ka.coef = NULL;
    ka.width = geo.width; ka.height = geo.height; ka.depth = geo.depth;
    ka.tiles_x = geo.tiles_x; ka.tiles_y = geo.tiles_y; ka.chunks = geo.chunks; ka.chunk_slices = geo.chunk_slices; ka.cells_z = geo.cells_z;
    ka.c1 = wc.c1; ka.c2 = wc.c2; ka.range = data_range;
    for (int i = 0; i < 6; ++i) ka.gf[i] = wc.gf[i];
    double t = 0.0;
    for (int i = 5; i >= 0; --i) { t += (double)ka.gf[i]; ka.tail[i] = (float)t; }
    ka.total = (float)(2.0 * t - (double)ka.gf[0]);
    return true;
}

dim3 grid_of(const Geometry3F& geo) { return dim3((uint32_t)((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count)); }

template <int TYPE>
hipError_t launch_adjoint(const Geometry3F& geo, const K3HArgs& ka, int which, hipStream_t stream)
{
    const dim3 grid = grid_of(geo), block(256);
    if (which == 1)      hipLaunchKernelGGL((ssim3h_adjoint_kernel<TYPE, 1>), grid, block, 0, stream, ka);
    else if (which == 2) hipLaunchKernelGGL((ssim3h_adjoint_kernel<TYPE, 2>), grid, block, 0, stream, ka);
    else                 hipLaunchKernelGGL((ssim3h_adjoint_kernel<TYPE, 3>), grid, block, 0, stream, ka);
    return hipGetLastError();
}

template <int TYPE>
hipError_t launch_grad(const Geometry3F& geo, const K3HArgs& ka, int which, hipStream_t stream)
{
    const dim3 grid = grid_of(geo), block(256);
    if (ka.gouts) {
        if (which == 1)      hipLaunchKernelGGL((ssim3h_mapwalk_kernel<TYPE, 1>), grid, block, 0, stream, ka);
        else if (which == 2) hipLaunchKernelGGL((ssim3h_mapwalk_kernel<TYPE, 2>), grid, block, 0, stream, ka);
        else                 hipLaunchKernelGGL((ssim3h_mapwalk_kernel<TYPE, 3>), grid, block, 0, stream, ka);
    } else {
        if (which == 1)      hipLaunchKernelGGL((ssim3h_walk_kernel<TYPE, 1>), grid, block, 0, stream, ka);
        else if (which == 2) hipLaunchKernelGGL((ssim3h_walk_kernel<TYPE, 2>), grid, block, 0, stream, ka);
        else                 hipLaunchKernelGGL((ssim3h_walk_kernel<TYPE, 3>), grid, block, 0, stream, ka);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_adjoint<TYPE>(geo, ka, which, stream);
}

} // namespace

hipError_t launch_ssim3h(const Geometry3F& geo, const Pair3HDesc* descs_dev, int type, float data_range, double* partials, double* sums,
                         hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3HArgs ka;
    if (!fill_args(ka, geo, type, data_range)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.partials = partials;
    const dim3 grid = grid_of(geo), block(256);
    if (type == kSHTypeBF16) hipLaunchKernelGGL((ssim3h_walk_kernel<kSHTypeBF16, 0>), grid, block, 0, stream, ka);
    else                     hipLaunchKernelGGL((ssim3h_walk_kernel<kSHTypeF16, 0>), grid, block, 0, stream, ka);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ssim3f_reduce(geo, partials, sums, stream);
}

hipError_t launch_ssim3h_grad(const Geometry3F& geo, const Pair3HDesc* descs_dev, const Grad3HDesc* grads_dev, int type, const float* g_out,
                              float data_range, int which, float* coef, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3HArgs ka;
    if (which < 1 || which > 3 || g_out == NULL || !fill_args(ka, geo, type, data_range)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.coef = coef;
    return type == kSHTypeBF16 ? launch_grad<kSHTypeBF16>(geo, ka, which, stream) : launch_grad<kSHTypeF16>(geo, ka, which, stream);
}

hipError_t launch_ssim3h_map_grad(const Geometry3F& geo, const Pair3HDesc* descs_dev, const Grad3HDesc* grads_dev, const GradOut3FDesc* gouts_dev,
                                  int type, float data_range, int which, float* coef, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3HArgs ka;
    if (which < 1 || which > 3 || gouts_dev == NULL || !fill_args(ka, geo, type, data_range)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.gouts = gouts_dev; ka.coef = coef;
    return type == kSHTypeBF16 ? launch_grad<kSHTypeBF16>(geo, ka, which, stream) : launch_grad<kSHTypeF16>(geo, ka, which, stream);
}

} // namespace ssim_hip
