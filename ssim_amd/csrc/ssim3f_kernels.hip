// ssim3f_kernels.hip -- gfx950 kernels of SSIM on float32 VOLUMES (a three-dimensional window) and of its gradient, behind
// rmgr_ssim_hip_enqueue_ssim3f, rmgr_ssim_hip_compute_ssim3f_device / _host and rmgr_ssim_hip_enqueue_ssim3f_grad.  The definition they
// implement is in include/rmgr/ssim-hip.h; tests/ssim3f_model.py restates it in float64 and restates the arithmetic below in fp32.
//
// Kept apart from the 2-D files on purpose: their kernels are counted and budgeted by the tests.  What resembles ssimf_kernels.hip (the
// folded row pass, the SSIM terms, the derivative, the adjoint weights, the per-image reduction) is copied here, not included.
//
//  * ssim3f_walk_kernel<MODE>: one 256-lane workgroup owns a 16 x 16 tile of (x, y) at an absolute position and walks a chunk of z.  Per
//    source slice (edge-clamped on every axis, any step / stride / sliceStride, 64-bit offsets) the workgroup loads the tile + 5 of A and
//    B one slice ahead into registers, centres them, writes (a', b') and (a'^2 + b'^2, a'b') of the 26 x 26 positions into LDS, runs the
//    x pass on 26 rows x 16 columns (LDS to LDS) and the y pass on its own column (one lane = one column of z), and scatters the four
//    blurred values into 11-deep register rings (the z pass); the rings' oldest entry is the finished slice z - 5.  No intermediate
//    volume touches HBM.  MODE 0: the SSIM value, the optional map store and the lane's fp64 sum, flushed once per reduction cell (16 x 16
//    x 8 voxels at an absolute position) through a fixed tree.  MODE 1 / 2 / 3 (dLoss/dA, dLoss/dB, both): the weighted partial
//    derivatives k d_mu, k d_aa, k d_ab (and k d_mu of B) of the voxel go to the coefficient volumes in the context's scratch.
//  * ssim3f_reduce_kernel: each volume's cell partials summed in a fixed order.
//  * ssim3f_adjoint_kernel<WHICH>: the same walk over the coefficient volumes, zero outside the volume: adjoint x pass and y pass in LDS as
//    weighted gathers, the adjoint z pass in register rings, then dLoss/da = Gt(k d_mu_a) + 2 a' Gt(k d_aa) + b' Gt(k d_ab).  Its launch
//    is a host function of its own (launch_ssim3f_adjoint): the backward for a per-voxel upstream gradient (ssim3w_kernels.hip) fills
//    the coefficient volumes with a walk of its own and runs this one unchanged.
//
// Chunks.  A chunk of z starts 5 slices early and runs 5 slices late (10 warm-up slices); every output voxel receives the 11 slice values of
// its window in source order, the first one multiplied into zero, whatever slice the chunk starts at, and a cell never straddles two
// chunks (chunk depths are multiples of the cell depth): value, map, sums and gradients have the same bits for every chunk depth.
//
// Centring.  Both walks blur a' = a - cA, b' = b - cB with ONE centre per volume: A's and B's sample at ((W - 1) / 2, (H - 1) / 2,
// (D - 1) / 2) when its magnitude is at most dataRange, else 0.  One centre for the whole volume (not one per 128 columns as in 2-D) lets
// the backward keep the coefficients of the centred variables in scratch: a coefficient and the voxel that collects it always share
// their centre.  The derivative is taken in the centred variables, as in ssimf_kernels.hip.
#include "ssim3f_kernels.h"
#include <algorithm>
#include <cmath>

namespace ssim_hip {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

typedef const float __attribute__((address_space(1)))* gptr_cf32;
typedef float __attribute__((address_space(1)))*       gptr_f32;
typedef double __attribute__((address_space(1)))*      gptr_f64;

__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float opaque(float v) { asm("" : "+v"(v)); return v; }

enum { T = kS3Tile, TIN = T + 10, NIN = TIN * TIN, NROW = TIN * T, NLOAD = (NIN + 255) / 256 };

struct K3Args {
    const Pair3FDesc* descs;
    const Grad3FDesc* grads;
    const float*      g_out;
    uint32_t width, height, depth, tiles_x, tiles_y, chunks, chunk_slices, cells_z;
    double*  partials;            // [volume][cell_z][tile_y][tile_x]
    float*   coef;                // [volume][plane][z][y][x]
    float    c1, c2, range;
    float    gf[6], tail[6], total;
};

// The workgroup's place: volume-major, then z-chunk, then tile row, then tile column.
struct Place { uint32_t vol; int x0, y0, z0, z_end; uint32_t tx, ty; };

__device__ __forceinline__ Place place_of(const K3Args& args)
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

// The volume's centre (top of the file).
__device__ __forceinline__ f2 centre_of(const Pair3FDesc& pd, int W, int H, int D, float range)
{
    const int64_t cx = (W - 1) / 2, cy = (H - 1) / 2, cz = (D - 1) / 2;
    const float sa = ((gptr_cf32)pd.a)[cx * pd.a_step + cy * pd.a_stride + cz * pd.a_slice];
    const float sb = ((gptr_cf32)pd.b)[cx * pd.b_step + cy * pd.b_stride + cz * pd.b_slice];
    return f2{__builtin_fabsf(sa) <= range ? sa : 0.0f, __builtin_fabsf(sb) <= range ? sb : 0.0f};
}

// MODE 0: value, map, sums.  MODE 1 / 2 / 3: the coefficient volumes of dLoss/dA, dLoss/dB, both.  The statistics are computed in the
// same order in all four.
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3f_walk_kernel(const K3Args args)
{
    constexpr int NP = MODE == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) f2 inAB[NIN];     // (a', b') of the tile + 5
    __shared__ __attribute__((aligned(16))) f2 inQ[NIN];      // (a'^2 + b'^2, a'b')
    __shared__ __attribute__((aligned(16))) f2 Hab[NROW];     // x pass, 26 rows x 16 columns
    __shared__ __attribute__((aligned(16))) f2 Hq[NROW];
    __shared__ double red[4];

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const Pair3FDesc pd = args.descs[pl.vol];
    const gptr_cf32 pa = (gptr_cf32)pd.a, pb = (gptr_cf32)pd.b;
    const float gf[6] = {args.gf[0], args.gf[1], args.gf[2], args.gf[3], args.gf[4], args.gf[5]};
    const f2 cen = centre_of(pd, W, H, D, args.range);

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
            va[t] = pa[offA[t] + zc * pd.a_slice];
            vb[t] = pb[offB[t] + zc * pd.b_slice];
        }
    };

    const int qx = pl.x0 + lx, qy = pl.y0 + ly;
    const bool inside = qx < W && qy < H;
    const uint64_t voxels = (uint64_t)W * (uint64_t)H * (uint64_t)D;
    float k = 0.0f;
    if constexpr (MODE != 0)
        k = (float)((double)((gptr_cf32)args.g_out)[pl.vol] / ((double)W * (double)H * (double)D));

    f2 accAB[11], accQ[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) accAB[i] = accQ[i] = f2{0.0f, 0.0f};
    double colsum = 0.0;

    fetch(pl.z0 - 5);
#pragma unroll 1
    for (int s = pl.z0 - 5; s < pl.z_end + 5; ++s) {
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
        const int z = s - 5;
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

// Per-volume sum of the cell partials in a fixed order: thread t of 1024 adds cells t, t + 1024, ... in that order, each wave runs a
// fixed xor butterfly, and the 16 wave totals are added in wave order.  One workgroup per volume.
constexpr int kReduceThreads = 1024;

__global__ __launch_bounds__(kReduceThreads) void ssim3f_reduce_kernel(const double* __restrict__ partials, uint64_t per_volume, double* __restrict__ sums)
{
    __shared__ double sh[kReduceThreads / 64];
    const double* p = partials + (size_t)blockIdx.x * per_volume;
    double acc = 0.0;
    for (uint64_t i = threadIdx.x; i < per_volume; i += kReduceThreads)
        acc += p[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63u) == 0)
        sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
#pragma unroll
        for (int w = 1; w < kReduceThreads / 64; ++w)
            t += sh[w];
        sums[blockIdx.x] = t;
    }
}

// What gradient voxel q of an axis of n voxels collects from p = q + j: the tap g|j| in the interior, and on the first (last) voxel the
// sum of the taps the forward pass clamped onto it, tail[|j|] = g|j| + ... + g5 for j >= 0 (j <= 0); the sum of all taps when n == 1.
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
// coefficient outside the volume is 0 (the clamp is in the weights).
template <int WHICH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3f_adjoint_kernel(const K3Args args)
{
    constexpr int NP = WHICH == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) float P[NP][NIN];      // the slice's coefficients on the tile + 5
    __shared__ __attribute__((aligned(16))) float Q[NP][NROW];     // adjoint x pass, 26 rows x 16 columns

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const Pair3FDesc pd = args.descs[pl.vol];
    const Grad3FDesc gd = args.grads[pl.vol];
    const float gf[6] = {args.gf[0], args.gf[1], args.gf[2], args.gf[3], args.gf[4], args.gf[5]};
    const float tail[6] = {args.tail[0], args.tail[1], args.tail[2], args.tail[3], args.tail[4], args.tail[5]};
    const f2 cen = centre_of(pd, W, H, D, args.range);
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
        const float a = ((gptr_cf32)pd.a)[(int64_t)qx * pd.a_step + (int64_t)qy * pd.a_stride + (int64_t)z * pd.a_slice] - cen.x;
        const float b = ((gptr_cf32)pd.b)[(int64_t)qx * pd.b_step + (int64_t)qy * pd.b_stride + (int64_t)z * pd.b_slice] - cen.y;
        if constexpr (WHICH != 2) {
            const float g = opaque(acc[0][0] + opaque(opaque(2.0f * a) * acc[1][0])) + opaque(b * acc[2][0]);
            ((gptr_f32)gd.ga)[(int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride + (int64_t)z * gd.ga_slice] = g;
        }
        if constexpr (WHICH != 1) {
            const float g = opaque(acc[WHICH == 3 ? 3 : 0][0] + opaque(opaque(2.0f * b) * acc[1][0])) + opaque(a * acc[2][0]);
            ((gptr_f32)gd.gb)[(int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride + (int64_t)z * gd.gb_slice] = g;
        }
    }
}

const uint64_t kMaxBlocks = (uint64_t(1) << 24) - 1;      // x 256 work-items stays below 2^32

// The engine's 11-tap Gaussian, sigma 1.5, centre first: g_i = exp(-(i i) / (2 s s)), the norm accumulated in double in the order
// i = 0 .. 5, g_0 once and the others twice; tap i = float(g_i / norm) -- the taps of every other kernel file, bit for bit.
void engine_taps(float (&gf)[6])
{
    double g[6], norm = 0.0;
    for (int i = 0; i < 6; ++i) {
        g[i] = std::exp(-(double)(i * i) / (2.0 * 1.5 * 1.5));
        norm += i == 0 ? g[i] : 2.0 * g[i];
    }
    for (int i = 0; i < 6; ++i) gf[i] = (float)(g[i] / norm);
}

void constants3f(float data_range, float& c1, float& c2)      // ssimf_constants(), copied
{
    const double R = (double)data_range;
    c1 = (float)((0.01 * R) * (0.01 * R));
    c2 = (float)((0.03 * R) * (0.03 * R));
}

bool fill_args(K3Args& ka, const Geometry3F& geo, float data_range, const float* taps)
{
    if (!(data_range > 0.0f) || !std::isfinite(data_range) || geo.count == 0 || geo.count > ssim3f_max_count(geo.width, geo.height, geo.depth)) return false;
    if ((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count > kMaxBlocks || geo.chunk_slices % kS3CellZ != 0) return false;
    ka.descs = NULL; ka.grads = NULL; ka.g_out = NULL; ka.partials = NULL; ka.coef = NULL;
    ka.width = geo.width; ka.height = geo.height; ka.depth = geo.depth;
    ka.tiles_x = geo.tiles_x; ka.tiles_y = geo.tiles_y; ka.chunks = geo.chunks; ka.chunk_slices = geo.chunk_slices; ka.cells_z = geo.cells_z;
    ka.range = data_range;
    constants3f(data_range, ka.c1, ka.c2);
    if (taps) { for (int i = 0; i < 6; ++i) ka.gf[i] = taps[i]; }       // an 11-tap window of the caller's
    else engine_taps(ka.gf);
    // tail[d] = g_d + ... + g_5 and the sum of all eleven taps: sums of the float taps in double, rounded once
    double t = 0.0;
    for (int i = 5; i >= 0; --i) { t += (double)ka.gf[i]; ka.tail[i] = (float)t; }
    ka.total = (float)(2.0 * t - (double)ka.gf[0]);
    return true;
}

} // namespace

uint32_t ssim3f_max_count(uint32_t width, uint32_t height, uint32_t depth)
{
    if (width == 0 || height == 0 || depth == 0 || width > kS3MaxDim || height > kS3MaxDim || depth > kS3MaxDim) return 0;
    const uint64_t tiles = (uint64_t)((width + kS3Tile - 1) / kS3Tile) * ((height + kS3Tile - 1) / kS3Tile);
    return (uint32_t)std::min<uint64_t>(kMaxBlocks / tiles, 65535);
}

Geometry3F plan3f(uint32_t width, uint32_t height, uint32_t depth, uint32_t count, int cu_count, uint32_t warmup)
{
    Geometry3F g;
    g.width = width; g.height = height; g.depth = depth; g.count = count;
    g.tiles_x = (width + kS3Tile - 1) / kS3Tile;
    g.tiles_y = (height + kS3Tile - 1) / kS3Tile;
    g.cells_z = (depth + kS3CellZ - 1) / kS3CellZ;
    // four workgroups of four waves per CU (the walk's occupancy): a round; pick the chunk depth (whole cells, doubling) that finishes the launch's workgroups in
    // the fewest slice-times, the warm-up slices (10 for the 11-tap window) included, among those whose grid fits
    const uint64_t slots = (uint64_t)(cu_count > 0 ? cu_count : 256) * 4;
    const uint64_t cols = (uint64_t)g.tiles_x * g.tiles_y * std::max<uint32_t>(count, 1);
    uint64_t best = ~uint64_t(0), best_slices = 0;
    for (uint64_t slices = kS3CellZ;; slices *= 2) {
        const uint64_t chunks = (depth + slices - 1) / slices;
        if (cols * chunks <= kMaxBlocks) {
            const uint64_t rounds = (cols * chunks + slots - 1) / slots;
            const uint64_t cost = rounds * (std::min<uint64_t>(slices, depth) + warmup);
            if (cost <= best) { best = cost; best_slices = slices; }
        }
        if (slices >= depth) {
            if (best_slices == 0) best_slices = slices;
            break;
        }
    }
    g.chunk_slices = (uint32_t)best_slices;
    g.chunks = (uint32_t)((depth + best_slices - 1) / best_slices);
    return g;
}

hipError_t launch_ssim3f(const Geometry3F& geo, const Pair3FDesc* descs_dev, float data_range, double* partials, double* sums, hipStream_t stream,
                         const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3Args ka;
    if (!fill_args(ka, geo, data_range, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.partials = partials;
    const dim3 grid((uint32_t)((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count)), block(256);
    hipLaunchKernelGGL((ssim3f_walk_kernel<0>), grid, block, 0, stream, ka);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ssim3f_reduce(geo, partials, sums, stream);
}

hipError_t launch_ssim3f_reduce(const Geometry3F& geo, const double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    hipLaunchKernelGGL(ssim3f_reduce_kernel, dim3(geo.count), dim3(kReduceThreads), 0, stream, partials, geo.cells_per_volume(), sums);
    return hipGetLastError();
}

hipError_t launch_ssim3f_grad(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, const float* g_out,
                              float data_range, int which, float* coef, hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3Args ka;
    if (which < 1 || which > 3 || !fill_args(ka, geo, data_range, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.coef = coef;
    const dim3 grid((uint32_t)((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count)), block(256);
    if (which == 1)      hipLaunchKernelGGL((ssim3f_walk_kernel<1>), grid, block, 0, stream, ka);
    else if (which == 2) hipLaunchKernelGGL((ssim3f_walk_kernel<2>), grid, block, 0, stream, ka);
    else                 hipLaunchKernelGGL((ssim3f_walk_kernel<3>), grid, block, 0, stream, ka);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ssim3f_adjoint(geo, descs_dev, grads_dev, data_range, which, coef, stream, taps);
}

hipError_t launch_ssim3f_adjoint(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, float data_range, int which,
                                 const float* coef, hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3Args ka;
    if (which < 1 || which > 3 || !fill_args(ka, geo, data_range, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.coef = const_cast<float*>(coef);
    const dim3 grid((uint32_t)((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count)), block(256);
    if (which == 1)      hipLaunchKernelGGL((ssim3f_adjoint_kernel<1>), grid, block, 0, stream, ka);
    else if (which == 2) hipLaunchKernelGGL((ssim3f_adjoint_kernel<2>), grid, block, 0, stream, ka);
    else                 hipLaunchKernelGGL((ssim3f_adjoint_kernel<3>), grid, block, 0, stream, ka);
    return hipGetLastError();
}

bool ssim3f_walk_constants(const Geometry3F& geo, float data_range, Walk3FConstants& out, const float* taps)
{
    K3Args ka;
    if (!fill_args(ka, geo, data_range, taps)) return false;
    out.c1 = ka.c1; out.c2 = ka.c2;
    for (int i = 0; i < 6; ++i) out.gf[i] = ka.gf[i];
    return true;
}

} // namespace ssim_hip
