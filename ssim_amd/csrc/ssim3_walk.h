// ssim3_walk.h -- the slice walk of SSIM on VOLUMES and its adjoint, written once for the kernel files of the family
// (ssim3f / ssim3w / ssim3h / ssim3k / ssim3hk / msssim3f / msssim3h _kernels.hip).  Not installed, and included by those seven files
// only: each of them keeps its __global__ kernels -- their names, template parameters and launch bounds, which its tests count and
// budget -- as one-line calls of walk_body and adjoint_body, and its launch_* functions.  Everything here has internal linkage, so an
// instantiation and its LDS planes belong to the one kernel of the including file that calls it.  The definition the kernels implement
// is in include/rmgr/ssim-hip.h; tests/ssim3f_model.py and tests/ssim3k_model.py restate it in float64 and restate the arithmetic below
// in fp32.
//
// The bodies are templates on these things, and on nothing else:
//  * Sample: how a sample gets into a register and how a gradient voxel leaves one.  SampleF32 is a float load / store.  SampleH<TYPE>
//    is a 2-byte load and an exact widening (bfloat16 is the upper half of a float32, a shift; float16 goes through the hardware
//    convert, which keeps subnormals and maps NaN and Inf to NaN and Inf), and one rounding to nearest-even before a 2-byte store
//    (float16: the hardware convert, subnormals kept, overflow to Inf; bfloat16: integer rounding of the bit pattern, NaN kept NaN).
//    That is fetch() of the walk, centre_of, and the adjoint's re-read of a and b and its stores.  From `f2{va, vb} - cen` on every
//    instruction is the same, which is what gives the 16-bit entries the bits of the float32 ones on the widened volumes.  Loads and
//    stores are the plain per-sample form: a base pointer is only aligned to its sample, the strides are arbitrary, and the walks are
//    VALU- and LDS-bound.  The coefficient volumes, the map and the upstream gradient stay float32.
//  * R, the window's radius, 1 .. 5 (3 .. 11 taps per axis): the staged plane is the tile + R on every side, (16 + 2R)^2 positions; the x
//    pass covers 16 + 2R rows x 16 columns; the y pass reads rows y - R .. y + R; the z rings are 2R + 1 deep and their oldest entry is
//    the finished slice s - R.  A window never reads beyond its radius: a NaN sample reaches the (2R + 1)^3 map voxels around it and no
//    others.
//  * KFORM (walk_body, MODE != 0): where the weight k of a voxel's partial derivatives comes from.  kKUniform: k = float(double(gOut) /
//    (double(W) double(H) double(D))) for the whole volume.  kKPerVoxel: k(p) = gMap(p), read per voxel through the pair's GradOut3FDesc.
//    kKEither: a branch on a kernel argument between the two (g_out != NULL: uniform).  The form is a compile-time choice of each kernel
//    because the run-time branch costs registers.  The product k d is the same instruction in all three, so a constant volume gMap
//    gives the uniform form's bits.  kKScale (the multi-scale form, msssim3f_kernels.hip): k = g_out[volume] as it stands, the k_s of that
//    volume at the launch's scale, computed on the device; a volume whose k is 0 is not walked at all (its adjoint writes +0 without
//    reading a coefficient).
//  * FORM (walk_body, a defaulted parameter: the five single-scale files do not name it).  kFormSsim: SSIM.  kFormMulti: a scale of
//    MS-SSIM that is not the last -- MODE 0 keeps TWO fp64 column sums, cs = A2 / B2 and ssim, and flushes two partials per cell,
//    [cell]{cs, ssim}, the ssim one with the bits of kFormSsim; MODE 1 / 2 / 3 writes the partial derivatives of cs alone, d_ab = 2 / B2,
//    d_aa = -cs / B2, d_mu = -2 mu_a' d_aa - mu_b' d_ab (no luminance part in the centred variables).
//  * MS (adjoint_body, defaulted likewise).  kMsNone.  kMsLast: the coarsest scale of MS-SSIM -- k = g_out[volume] is read, and a volume
//    whose k is 0 gets +0 in every gradient voxel, whatever its samples are.  kMsUp: a finer scale -- the same, and every voxel adds the
//    adjoint of the clamped 2 x 2 x 2 mean, fp32(0.125 c g_{s+1}(x >> 1, y >> 1, z >> 1)), before its single store; the coarser scale's
//    dense gradient volumes come through args.up, a member only the multi-scale files' argument structs have; its type is the
//    descriptor of those volumes, float32 (Grad3FDesc) under either sample policy.
//
// walk_body<Sample, R, MODE, KFORM, FORM>.  One 256-lane workgroup owns a 16 x 16 tile of (x, y) at an absolute position and walks a chunk of
// z.  Per source slice (edge-clamped on every axis, any step / stride / sliceStride, 64-bit offsets) the workgroup loads the tile + R
// of A and B one slice ahead into registers, centres them, writes (a', b') and (a'^2 + b'^2, a'b') into LDS, runs the x pass (LDS to
// LDS) and the y pass on its own column (one lane = one column of z), and scatters the four blurred values into the register rings (the
// z pass).  No intermediate volume touches HBM.  MODE 0: the SSIM value, the optional map store and the lane's fp64 sum, flushed once
// per reduction cell (16 x 16 x 8 voxels at an absolute position) through a fixed tree.  MODE 1 / 2 / 3 (dLoss/dA, dLoss/dB, both): the
// weighted partial derivatives k d_mu, k d_aa, k d_ab (and k d_mu of B) of the voxel go to the coefficient volumes in the context's
// scratch.  The lane that owns column (qx, qy) reads a per-voxel k of output slice z = s - R at the top of the slice iteration, before
// the two barriers: its latency sits under the LDS passes.  A lane outside the volume, or a warm-up iteration (z < z0), issues no load.
//
// adjoint_body<Sample, R, WHICH, MS>.  The same walk over the coefficient volumes, zero outside the volume: adjoint x pass and y pass in
// LDS as weighted gathers, the adjoint z pass in register rings, then dLoss/da = Gt(k d_mu_a) + 2 a' Gt(k d_aa) + b' Gt(k d_ab).
//
// Chunks.  A chunk of z starts R slices early and runs R slices late (2R warm-up slices); every output voxel receives the 2R + 1 slice
// values of its window in source order, the first one multiplied into zero, whatever slice the chunk starts at, and a cell never
// straddles two chunks (chunk depths are multiples of the cell depth): value, map, sums and gradients have the same bits for every
// chunk depth.
//
// Centring.  Both walks blur a' = a - cA, b' = b - cB with ONE centre per volume: A's and B's sample at ((W - 1) / 2, (H - 1) / 2,
// (D - 1) / 2) when its magnitude is at most dataRange, else 0.  One centre for the whole volume (not one per 128 columns as in 2-D) lets
// the backward keep the coefficients of the centred variables in scratch: a coefficient and the voxel that collects it always share
// their centre.  The derivative is taken in the centred variables, as in ssimf_kernels.hip.  Centres, cells, tiles and summation orders
// are position-based: none depends on the radius or on the size of a sample.
#ifndef SSIM_AMD_SSIM3_WALK_H
#define SSIM_AMD_SSIM3_WALK_H

#include "ssim3h_kernels.h"     // Pair3HDesc, Grad3HDesc, kSHTypeF16 / BF16; Pair3FDesc, Grad3FDesc, GradOut3FDesc, Geometry3F, ssim3f_walk_constants
#include <type_traits>

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
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// A stored sample -> float32, exactly.
template <int TYPE>
__device__ __forceinline__ float widen(uint16_t s)
{
    if constexpr (TYPE == kSHTypeBF16) return __builtin_bit_cast(float, (uint32_t)s << 16);
    else                               return (float)__builtin_bit_cast(_Float16, s);
}
// float32 -> the samples' encoding, one rounding to nearest-even.
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

// The sample policies: the descriptors of a pair, and element `at` of a volume in and out of a register.
struct SampleF32 {
    typedef Pair3FDesc Pair;
    typedef Grad3FDesc Grad;
    static __device__ __forceinline__ float load(const float* p, int64_t at) { return ((gptr_cf32)p)[at]; }
    static __device__ __forceinline__ void store(float* p, int64_t at, float v) { ((gptr_f32)p)[at] = v; }
};
template <int TYPE> struct SampleH {
    typedef Pair3HDesc Pair;
    typedef Grad3HDesc Grad;
    static __device__ __forceinline__ float load(const uint16_t* p, int64_t at) { return widen<TYPE>(((gptr_cu16)p)[at]); }
    static __device__ __forceinline__ void store(uint16_t* p, int64_t at, float v) { ((gptr_u16)p)[at] = narrow<TYPE>(v); }
};

enum { T = kS3Tile, MAXR = 5 };

// The planes of radius R: the staged tile + R, the x pass's rows, loads and x-pass positions per lane, the taps of an axis.
template <int R> struct Shape {
    enum { TIN = T + 2 * R, NIN = TIN * TIN, NROW = TIN * T, NLOAD = (NIN + 255) / 256, NXP = (NROW + 255) / 256, NT = 2 * R + 1 };
};

// What every kernel of the family takes by value.
template <class PairDesc, class GradDesc>
struct Walk3Args {
    const PairDesc*      descs;
    const GradDesc*      grads;
    const float*         g_out;       // the uniform upstream form (kKUniform; kKEither: or NULL)
    const GradOut3FDesc* gouts;       // the per-voxel upstream form (kKPerVoxel; kKEither: g_out == NULL)
    uint32_t width, height, depth, tiles_x, tiles_y, chunks, chunk_slices, cells_z;
    double*  partials;            // [volume][cell_z][tile_y][tile_x]
    float*   coef;                // [volume][plane][z][y][x]
    float    c1, c2, range;
    float    gf[MAXR + 1], tail[MAXR + 1], total;
};
template <class Sample> using ArgsOf = Walk3Args<typename Sample::Pair, typename Sample::Grad>;

// The workgroup's place: volume-major, then z-chunk, then tile row, then tile column.
struct Place { uint32_t vol; int x0, y0, z0, z_end; uint32_t tx, ty; };

template <class Args>
__device__ __forceinline__ Place place_of(const Args& args)
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

// The volume's centre (top of the file).
template <class Sample>
__device__ __forceinline__ f2 centre_of(const typename Sample::Pair& pd, int W, int H, int D, float range)
{
    const int64_t cx = (W - 1) / 2, cy = (H - 1) / 2, cz = (D - 1) / 2;
    const float sa = Sample::load(pd.a, cx * pd.a_step + cy * pd.a_stride + cz * pd.a_slice);
    const float sb = Sample::load(pd.b, cx * pd.b_step + cy * pd.b_stride + cz * pd.b_slice);
    return f2{__builtin_fabsf(sa) <= range ? sa : 0.0f, __builtin_fabsf(sb) <= range ? sb : 0.0f};
}

enum { kKUniform, kKPerVoxel, kKEither, kKScale };
enum { kFormSsim, kFormMulti };
enum { kMsNone, kMsLast, kMsUp };

// MODE 0: value, map, sums.  MODE 1 / 2 / 3: the coefficient volumes of dLoss/dA, dLoss/dB, both.  The statistics are computed in the
// same order in all four.
template <class Sample, int R, int MODE, int KFORM, int FORM = kFormSsim>
__device__ __forceinline__ void walk_body(const ArgsOf<Sample>& args)
{
    typedef Shape<R> S;
    constexpr int TIN = S::TIN, NIN = S::NIN, NROW = S::NROW, NLOAD = S::NLOAD, NT = S::NT;
    constexpr int NP = MODE == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) f2 inAB[NIN];     // (a', b') of the tile + R
    __shared__ __attribute__((aligned(16))) f2 inQ[NIN];      // (a'^2 + b'^2, a'b')
    __shared__ __attribute__((aligned(16))) f2 Hab[NROW];     // x pass, 16 + 2R rows x 16 columns
    __shared__ __attribute__((aligned(16))) f2 Hq[NROW];
    __shared__ double red[MODE == 0 && FORM == kFormMulti ? 8 : 4];

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const typename Sample::Pair pd = args.descs[pl.vol];
    float gf[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) gf[i] = args.gf[i];
    const f2 cen = centre_of<Sample>(pd, W, H, D, args.range);

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
            va[t] = Sample::load(pd.a, offA[t] + zc * pd.a_slice);
            vb[t] = Sample::load(pd.b, offB[t] + zc * pd.b_slice);
        }
    };

    const int qx = pl.x0 + lx, qy = pl.y0 + ly;
    const bool inside = qx < W && qy < H;
    const uint64_t voxels = (uint64_t)W * (uint64_t)H * (uint64_t)D;
    // the weight of the voxel's partial derivatives: one float for the volume, or the lane's column of gMap
    float k_vol = 0.0f;
    gptr_cf32 pg = nullptr;
    int64_t offG = 0, g_slice = 0;
    if constexpr (MODE != 0 && KFORM == kKScale) {
        k_vol = ((gptr_cf32)args.g_out)[pl.vol];
        if (k_vol == 0.0f) return;                 // the whole workgroup: the adjoint of such a volume reads no coefficient
    } else if constexpr (MODE != 0) {
        if (KFORM == kKUniform || (KFORM == kKEither && args.g_out)) {
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
    double colsum = 0.0, colsum_cs = 0.0;

    fetch(pl.z0 - R);
#pragma unroll 1
    for (int s = pl.z0 - R; s < pl.z_end + R; ++s) {
        // 0. k of the slice this iteration finishes, z = s - R < z_end; no address is formed outside the volume or during the warm-up
        const int z = s - R;
        float k = k_vol;
        if constexpr (MODE != 0 && KFORM != kKUniform && KFORM != kKScale) {
            if ((KFORM == kKPerVoxel || pg) && inside && z >= pl.z0)
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
            if constexpr (FORM == kFormMulti) {
                const float cs = A2 * __builtin_amdgcn_rcpf(B2);
                if (inside) colsum_cs += (double)cs;
            }
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
                if constexpr (FORM == kFormMulti) {
                    double u = colsum_cs;
                    colsum_cs = 0.0;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) u += __shfl_xor(u, off, 64);
                    if ((tid & 63) == 0) red[4 + (tid >> 6)] = u;
                }
                __syncthreads();
                if (tid == 0) {
                    const uint64_t cell = (((uint64_t)pl.vol * args.cells_z + (uint32_t)z / kS3CellZ) * args.tiles_y + pl.ty) * args.tiles_x + pl.tx;
                    if constexpr (FORM == kFormMulti) {
                        ((gptr_f64)args.partials)[2 * cell] = (red[4] + red[5]) + (red[6] + red[7]);
                        ((gptr_f64)args.partials)[2 * cell + 1] = (red[0] + red[1]) + (red[2] + red[3]);
                    } else {
                        ((gptr_f64)args.partials)[cell] = (red[0] + red[1]) + (red[2] + red[3]);
                    }
                }
            }
        } else {
            float dab, daa, dmA, dmB;
            if constexpr (FORM == kFormMulti) {
                const float r2 = __builtin_amdgcn_rcpf(B2);
                const float cs = opaque(A2 * r2);
                dab = opaque(2.0f * r2);
                daa = -opaque(cs * r2);
                dmA = -opaque(opaque(2.0f * mm.x) * daa) - opaque(mm.y * dab);
                dmB = -opaque(opaque(2.0f * mm.y) * daa) - opaque(mm.x * dab);
            } else {
                const float r1 = __builtin_amdgcn_rcpf(B1), r2 = __builtin_amdgcn_rcpf(B2);
                const float r12 = opaque(r1 * r2);
                const float ssim = opaque(opaque(A1 * A2) * r12);
                dab = opaque(opaque(2.0f * A1) * r12);
                daa = -opaque(ssim * r2);
                const float f1 = opaque(A2 * r12), f2_ = opaque(ssim * r1);
                dmA = opaque(opaque(opaque(opaque(2.0f * uB) * f1) - opaque(opaque(2.0f * uA) * f2_)) - opaque(opaque(2.0f * mm.x) * daa)) - opaque(mm.y * dab);
                dmB = opaque(opaque(opaque(opaque(2.0f * uA) * f1) - opaque(opaque(2.0f * uB) * f2_)) - opaque(opaque(2.0f * mm.y) * daa)) - opaque(mm.x * dab);
            }
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

// What gradient voxel q of an axis of n voxels collects from p = q + j: the tap g|j| in the interior, and on the first (last) voxel the
// sum of the taps the forward pass clamped onto it, tail[|j|] = g|j| + ... + gR for j >= 0 (j <= 0); the sum of all taps when n == 1.
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

// The descriptor of the coarser scale's gradient volumes: what args.up points to (kMsUp); no coarser scale, no member.
template <class Args, class Sample, bool UP> struct UpDescOf { typedef typename Sample::Grad type; };
template <class Args, class Sample> struct UpDescOf<Args, Sample, true> {
    typedef std::remove_cv_t<std::remove_pointer_t<decltype(Args::up)>> type;
};

// WHICH: 1 dLoss/dA, 2 dLoss/dB, 3 both.  Every pass is a gather in the order j = -R .. R, the first product plain, the others fused; a
// coefficient outside the volume is 0 (the clamp is in the weights).  A 16-bit gradient voxel is rounded once on its way out.
template <class Sample, int R, int WHICH, int MS = kMsNone, class Args = ArgsOf<Sample>>
__device__ __forceinline__ void adjoint_body(const Args& args)
{
    typedef Shape<R> S;
    constexpr int TIN = S::TIN, NIN = S::NIN, NROW = S::NROW, NLOAD = S::NLOAD, NT = S::NT;
    constexpr int NP = WHICH == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) float P[NP][NIN];      // the slice's coefficients on the tile + R
    __shared__ __attribute__((aligned(16))) float Q[NP][NROW];     // adjoint x pass, 16 + 2R rows x 16 columns

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const typename Sample::Pair pd = args.descs[pl.vol];
    const typename Sample::Grad gd = args.grads[pl.vol];
    float gf[R + 1], tail[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) { gf[i] = args.gf[i]; tail[i] = args.tail[i]; }
    const f2 cen = centre_of<Sample>(pd, W, H, D, args.range);
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

    // The multi-scale forms: what the voxel adds from the coarser scale, and the volumes whose k is 0.
    typedef typename UpDescOf<Args, Sample, MS == kMsUp>::type UpDesc;
    UpDesc ud = UpDesc();
    float cxy = 0.125f;
    if constexpr (MS == kMsUp) {
        ud = args.up[pl.vol];
        cxy = 0.125f * ((((W & 1) && qx == W - 1) ? 2.0f : 1.0f) * (((H & 1) && qy == H - 1) ? 2.0f : 1.0f));
    }
    // fp32(0.125 c g_{s+1}(x >> 1, y >> 1, z >> 1)); 0.125 c is a power of two: the product is exact
    // the coarser volumes are dense: ceil(W / 2) x ceil(H / 2) x ceil(D / 2), x fastest
    auto upstream = [&](const float* gup, int z) -> float {
        const float c = cxy * (((D & 1) && z == D - 1) ? 2.0f : 1.0f);
        return c * ((gptr_cf32)gup)[((int64_t)(z >> 1) * ((H + 1) >> 1) + (qy >> 1)) * ((W + 1) >> 1) + (qx >> 1)];
    };
    if constexpr (MS != kMsNone) {
        if (((gptr_cf32)args.g_out)[pl.vol] == 0.0f) {       // the whole workgroup: this scale contributes +0 whatever the samples are
            if (!inside) return;
            for (int z = pl.z0; z < pl.z_end; ++z) {
                if constexpr (WHICH != 2) {
                    float g = 0.0f;
                    if constexpr (MS == kMsUp) g += upstream(ud.ga, z);
                    Sample::store(gd.ga, (int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride + (int64_t)z * gd.ga_slice, g);
                }
                if constexpr (WHICH != 1) {
                    float g = 0.0f;
                    if constexpr (MS == kMsUp) g += upstream(ud.gb, z);
                    Sample::store(gd.gb, (int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride + (int64_t)z * gd.gb_slice, g);
                }
            }
            return;
        }
    }
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
        const float a = Sample::load(pd.a, (int64_t)qx * pd.a_step + (int64_t)qy * pd.a_stride + (int64_t)z * pd.a_slice) - cen.x;
        const float b = Sample::load(pd.b, (int64_t)qx * pd.b_step + (int64_t)qy * pd.b_stride + (int64_t)z * pd.b_slice) - cen.y;
        if constexpr (WHICH != 2) {
            float g = opaque(acc[0][0] + opaque(opaque(2.0f * a) * acc[1][0])) + opaque(b * acc[2][0]);
            if constexpr (MS == kMsUp) g = opaque(g) + upstream(ud.ga, z);
            Sample::store(gd.ga, (int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride + (int64_t)z * gd.ga_slice, g);
        }
        if constexpr (WHICH != 1) {
            float g = opaque(acc[WHICH == 3 ? 3 : 0][0] + opaque(opaque(2.0f * b) * acc[1][0])) + opaque(a * acc[2][0]);
            if constexpr (MS == kMsUp) g = opaque(g) + upstream(ud.gb, z);
            Sample::store(gd.gb, (int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride + (int64_t)z * gd.gb_slice, g);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------

// What every launch takes by value, every pointer NULL.  taps: gf[0 .. radius] of the window, centre first; radius 5 (11 taps) also
// takes NULL, the engine's window.  C1, C2, the engine's taps and the refusals (data_range, geometry) are ssim3f_walk_constants'.
// tail[d] = g_d + ... + g_R and the sum of all 2R + 1 taps are sums of the float taps in double, rounded once.
template <class Args>
bool fill_args(Args& ka, const Geometry3F& geo, float data_range, uint32_t radius, const float* taps)
{
    Walk3FConstants wc;
    if (radius < 1 || radius > MAXR || (!taps && radius != MAXR) || !ssim3f_walk_constants(geo, data_range, wc, radius == MAXR ? taps : NULL)) return false;
    ka = Args();
    ka.width = geo.width; ka.height = geo.height; ka.depth = geo.depth;
    ka.tiles_x = geo.tiles_x; ka.tiles_y = geo.tiles_y; ka.chunks = geo.chunks; ka.chunk_slices = geo.chunk_slices; ka.cells_z = geo.cells_z;
    ka.c1 = wc.c1; ka.c2 = wc.c2; ka.range = data_range;
    double t = 0.0;
    for (int i = (int)radius; i >= 0; --i) {
        ka.gf[i] = taps ? taps[i] : wc.gf[i];
        t += (double)ka.gf[i];
        ka.tail[i] = (float)t;
    }
    ka.total = (float)(2.0 * t - (double)ka.gf[0]);
    return true;
}

inline dim3 grid_of(const Geometry3F& geo) { return dim3((uint32_t)((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count)); }

// A run-time `value` in LO .. HI as a compile-time constant: returns f(std::integral_constant<int, value>()), a bool; false, and no call,
// when it is outside the range.  Nested, this is the dispatch on type, radius, mode and which of every launch of the family: true when a
// kernel was launched.
template <int LO, int HI, class F>
bool with_constant(int64_t value, F&& f)
{
    if constexpr (LO <= HI) {
        if (value == LO) return f(std::integral_constant<int, LO>());
        return with_constant<LO + 1, HI>(value, f);
    } else {
        return false;
    }
}

} // namespace
} // namespace ssim_hip

#endif
