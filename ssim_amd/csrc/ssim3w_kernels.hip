// ssim3w_kernels.hip -- gfx950 kernels of the gradient of the 3-D SSIM MAP for a per-voxel upstream gradient, behind
// rmgr_ssim_hip_enqueue_ssim3f_map_grad.  The definition is in include/rmgr/ssim-hip.h; tests/ssim3w_model.py restates it in float64 and
// restates the arithmetic below in fp32.
//
// Kept apart from ssim3f_kernels.hip on purpose: that file's kernels are counted and budgeted by the tests.  ssim3w_walk_kernel<MODE> is
// ssim3f_walk_kernel<MODE> of MODE 1 / 2 / 3 (the coefficient volumes of dLoss/dA, dLoss/dB, both), copied, with ONE change: the weight k
// of the voxel's partial derivatives is not the launch-uniform float(gOut / (W H D)) but gMap(p), read per voxel through the pair's
// GradOut3FDesc.  Every instruction that produces d_mu, d_aa, d_ab is that file's, the coefficient layout is that file's, and the second
// walk is that file's ssim3f_adjoint_kernel itself (launch_ssim3f_adjoint): a volume gMap of the constant float(gOut / (W H D)) leaves the
// bits of launch_ssim3f_grad.
//
// The load of k.  The lane that owns column (qx, qy) reads k of output slice z = s - 5 at the top of the slice iteration, before the two
// barriers: its latency sits under the LDS passes.  A lane outside the volume, or a warm-up iteration (z < z0), issues no load.  The
// offset is a 64-bit sum of 64-bit products; zero and negative strides are ordinary values of it.
#include "ssim3w_kernels.h"

namespace ssim_hip {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

typedef const float __attribute__((address_space(1)))* gptr_cf32;
typedef float __attribute__((address_space(1)))*       gptr_f32;

__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float opaque(float v) { asm("" : "+v"(v)); return v; }

enum { T = kS3Tile, TIN = T + 10, NIN = TIN * TIN, NROW = TIN * T, NLOAD = (NIN + 255) / 256 };

struct K3WArgs {
    const Pair3FDesc*    descs;
    const GradOut3FDesc* gouts;
    uint32_t width, height, depth, tiles_x, tiles_y, chunks, chunk_slices;
    float*   coef;                // [volume][plane][z][y][x]
    float    c1, c2, range;
    float    gf[6];
};

// The workgroup's place: volume-major, then z-chunk, then tile row, then tile column (ssim3f_kernels.hip: place_of).
struct Place { uint32_t vol; int x0, y0, z0, z_end; };

__device__ __forceinline__ Place place_of(const K3WArgs& args)
{
    const uint32_t tiles = args.tiles_x * args.tiles_y, per_vol = tiles * args.chunks;
    Place p;
    p.vol = blockIdx.x / per_vol;
    const uint32_t rem = blockIdx.x - p.vol * per_vol, chunk = rem / tiles, lin = rem - chunk * tiles;
    const uint32_t ty = lin / args.tiles_x, tx = lin - ty * args.tiles_x;
    p.x0 = (int)(tx * T); p.y0 = (int)(ty * T);
    const uint64_t z0 = (uint64_t)chunk * args.chunk_slices, z1 = z0 + args.chunk_slices;
    p.z0 = (int)z0;
    p.z_end = (int)(z1 < args.depth ? z1 : args.depth);
    return p;
}

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// The volume's centre (ssim3f_kernels.hip: centre_of).
__device__ __forceinline__ f2 centre_of(const Pair3FDesc& pd, int W, int H, int D, float range)
{
    const int64_t cx = (W - 1) / 2, cy = (H - 1) / 2, cz = (D - 1) / 2;
    const float sa = ((gptr_cf32)pd.a)[cx * pd.a_step + cy * pd.a_stride + cz * pd.a_slice];
    const float sb = ((gptr_cf32)pd.b)[cx * pd.b_step + cy * pd.b_stride + cz * pd.b_slice];
    return f2{__builtin_fabsf(sa) <= range ? sa : 0.0f, __builtin_fabsf(sb) <= range ? sb : 0.0f};
}

// MODE 1 / 2 / 3: the coefficient volumes of dLoss/dA, dLoss/dB, both.  Steps 1 to 4 and the derivative of step 5 are
// ssim3f_walk_kernel's, operation by operation.
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3w_walk_kernel(const K3WArgs args)
{
    static_assert(MODE >= 1 && MODE <= 3, "the value walk stays in ssim3f_kernels.hip");
    constexpr int NP = MODE == 3 ? 4 : 3;
    __shared__ __attribute__((aligned(16))) f2 inAB[NIN];     // (a', b') of the tile + 5
    __shared__ __attribute__((aligned(16))) f2 inQ[NIN];      // (a'^2 + b'^2, a'b')
    __shared__ __attribute__((aligned(16))) f2 Hab[NROW];     // x pass, 26 rows x 16 columns
    __shared__ __attribute__((aligned(16))) f2 Hq[NROW];

    const int tid = threadIdx.x, lx = tid & (T - 1), ly = tid >> 4;
    const int W = (int)args.width, H = (int)args.height, D = (int)args.depth;
    const Place pl = place_of(args);
    const Pair3FDesc pd = args.descs[pl.vol];
    const GradOut3FDesc go = args.gouts[pl.vol];
    const gptr_cf32 pa = (gptr_cf32)pd.a, pb = (gptr_cf32)pd.b, pg = (gptr_cf32)go.g;
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
    const int64_t offG = inside ? (int64_t)qx * go.g_step + (int64_t)qy * go.g_stride : 0;      // the lane's column of gMap

    f2 accAB[11], accQ[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) accAB[i] = accQ[i] = f2{0.0f, 0.0f};

    fetch(pl.z0 - 5);
#pragma unroll 1
    for (int s = pl.z0 - 5; s < pl.z_end + 5; ++s) {
        // 0. k of the slice this iteration finishes, z = s - 5 < z_end; no address is formed outside the volume or during the warm-up
        const int z = s - 5;
        float k = 0.0f;
        if (inside && z >= pl.z0)
            k = pg[offG + (int64_t)z * go.g_slice];
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

} // namespace

hipError_t launch_ssim3w_grad(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, const GradOut3FDesc* gouts_dev,
                              float data_range, int which, float* coef, hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    Walk3FConstants wc;
    if (which < 1 || which > 3 || !ssim3f_walk_constants(geo, data_range, wc, taps)) return hipErrorInvalidValue;
    K3WArgs ka;
    ka.descs = descs_dev; ka.gouts = gouts_dev; ka.coef = coef;
    ka.width = geo.width; ka.height = geo.height; ka.depth = geo.depth;
    ka.tiles_x = geo.tiles_x; ka.tiles_y = geo.tiles_y; ka.chunks = geo.chunks; ka.chunk_slices = geo.chunk_slices;
    ka.c1 = wc.c1; ka.c2 = wc.c2; ka.range = data_range;
    for (int i = 0; i < 6; ++i) ka.gf[i] = wc.gf[i];
    const dim3 grid((uint32_t)((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count)), block(256);
    if (which == 1)      hipLaunchKernelGGL((ssim3w_walk_kernel<1>), grid, block, 0, stream, ka);
    else if (which == 2) hipLaunchKernelGGL((ssim3w_walk_kernel<2>), grid, block, 0, stream, ka);
    else                 hipLaunchKernelGGL((ssim3w_walk_kernel<3>), grid, block, 0, stream, ka);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ssim3f_adjoint(geo, descs_dev, grads_dev, data_range, which, coef, stream, taps);
}

} // namespace ssim_hip
