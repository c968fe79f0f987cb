// ssim3f_kernels.hip -- gfx950 kernels of SSIM on float32 VOLUMES (a three-dimensional window) and of its gradient, behind
// rmgr_ssim_hip_enqueue_ssim3f, rmgr_ssim_hip_compute_ssim3f_device / _host and rmgr_ssim_hip_enqueue_ssim3f_grad.  The definition they
// implement is in include/rmgr/ssim-hip.h; tests/ssim3f_model.py restates it in float64 and restates the arithmetic in fp32.
//
// The walk and its adjoint are ssim3_walk.h's (tiles, chunks, centring, rings and adjoint weights are described there), instantiated
// here with SampleF32 at R = 5, the 11-tap window:
//  * ssim3f_walk_kernel<MODE>: MODE 0 (value, map, sums) and 1 / 2 / 3 (coefficient volumes, kKUniform).
//  * ssim3f_adjoint_kernel<WHICH>.  Its launch is a host function of its own (launch_ssim3f_adjoint): the backward for a per-voxel
//    upstream gradient (ssim3w_kernels.hip) fills the coefficient volumes with a walk of its own and runs this one unchanged.
// What the whole family shares and this file owns: ssim3f_reduce_kernel (each volume's cell partials summed in a fixed order), the
// planner (plan3f, ssim3f_max_count) and the constants of a walk (ssim3f_walk_constants: C1, C2, the engine's taps, the refusals).
#include "ssim3f_kernels.h"
#include "ssim3_walk.h"
#include <algorithm>
#include <cmath>

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleF32> K3Args;

template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3f_walk_kernel(const K3Args args)
{
    walk_body<SampleF32, 5, MODE, kKUniform>(args);
}

template <int WHICH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3f_adjoint_kernel(const K3Args args)
{
    adjoint_body<SampleF32, 5, WHICH>(args);
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

bool ssim3f_walk_constants(const Geometry3F& geo, float data_range, Walk3FConstants& out, const float* taps)
{
    if (!(data_range > 0.0f) || !std::isfinite(data_range) || geo.count == 0 || geo.count > ssim3f_max_count(geo.width, geo.height, geo.depth)) return false;
    if ((uint64_t)geo.tiles_x * geo.tiles_y * geo.chunks * geo.count > kMaxBlocks || geo.chunk_slices % kS3CellZ != 0) return false;
    constants3f(data_range, out.c1, out.c2);
    if (taps) { for (int i = 0; i < 6; ++i) out.gf[i] = taps[i]; }       // an 11-tap window of the caller's
    else engine_taps(out.gf);
    return true;
}

hipError_t launch_ssim3f(const Geometry3F& geo, const Pair3FDesc* descs_dev, float data_range, double* partials, double* sums, hipStream_t stream,
                         const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3Args ka;
    if (!fill_args(ka, geo, data_range, 5, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.partials = partials;
    hipLaunchKernelGGL((ssim3f_walk_kernel<0>), grid_of(geo), dim3(256), 0, stream, ka);
    const hipError_t e = hipGetLastError();
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
    if (!fill_args(ka, geo, data_range, 5, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.coef = coef;
    if (!with_constant<1, 3>(which, [&](auto MODE) {
            hipLaunchKernelGGL((ssim3f_walk_kernel<MODE()>), grid_of(geo), dim3(256), 0, stream, ka);
            return true; }))
        return hipErrorInvalidValue;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ssim3f_adjoint(geo, descs_dev, grads_dev, data_range, which, coef, stream, taps);
}

hipError_t launch_ssim3f_adjoint(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, float data_range, int which,
                                 const float* coef, hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3Args ka;
    if (!fill_args(ka, geo, data_range, 5, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.coef = const_cast<float*>(coef);
    return with_constant<1, 3>(which, [&](auto WHICH) {
        hipLaunchKernelGGL((ssim3f_adjoint_kernel<WHICH()>), grid_of(geo), dim3(256), 0, stream, ka);
        return true; }) ? hipGetLastError() : hipErrorInvalidValue;
}

} // namespace ssim_hip
