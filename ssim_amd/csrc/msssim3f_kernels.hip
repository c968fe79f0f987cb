// msssim3f_kernels.hip -- gfx950 kernels of multi-scale SSIM on float32 VOLUMES and of its gradient, behind
// rmgr_ssim_hip_enqueue_msssim3f, rmgr_ssim_hip_compute_msssim3f_device / _host and rmgr_ssim_hip_enqueue_msssim3f_grad.  The definition
// they implement is in include/rmgr/ssim-hip.h; tests/msssim3f_model.py restates it in float64 and restates the arithmetic in fp32.
//
// The walk and its adjoint are ssim3_walk.h's (tiles, chunks, centring, rings and adjoint weights are described there), instantiated
// here with SampleF32 at R = 5, the 11-tap window, in the multi-scale forms of that file:
//  * msssim3f_walk_kernel<0, kFormMulti>: one scale's value walk with TWO fp64 column sums (cs and ssim) and two partials per cell; the
//    ssim partial has the bits of ssim3f_walk_kernel<0>'s on the same volume.
//  * msssim3f_walk_kernel<MODE, FORM>, MODE 1 / 2 / 3: the coefficient volumes of one scale, k_s read as one float per volume (kKScale);
//    FORM kFormMulti (the cs form) on every scale but the coarsest, kFormSsim on the coarsest.
//  * msssim3f_adjoint_kernel<WHICH, MS>: the adjoint walk; kMsUp adds 0.125 c g_{s+1}(x >> 1, y >> 1, z >> 1) before its single store,
//    kMsLast (the coarsest scale) has nothing to add.  A volume whose k_s is 0 gets +0 from this scale without a coefficient being read.
// Its own kernels: the pyramid step (msssim3f_down_kernel), the reduction of every (pair, scale, kind) in ssim3f_reduce_kernel's order,
// the weighted product (msssim3f_finalise_kernel) and the coefficients k_s (msssim3f_coef_kernel: ms_product as msssimf_kernels.hip has it).
#include "msssim3f_kernels.h"
#include "ssim3_walk.h"
#include <algorithm>
#include <cmath>

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleF32> K3Args;

// What the adjoint of a scale that is not the coarsest takes besides: the coarser scale's gradient volumes, one Grad3FDesc per pair.
struct KM3Args : K3Args {
    const Grad3FDesc* up;
};

template <int MODE, int FORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void msssim3f_walk_kernel(const K3Args args)
{
    walk_body<SampleF32, 5, MODE, MODE == 0 ? kKUniform : kKScale, FORM>(args);
}

// Three waves per SIMD for both gradients, four for one: the occupancy of ssim3f_adjoint_kernel<WHICH>, asked for here because the
// coarser scale's gradient would otherwise cost the both-gradients form its third wave (173 VGPRs against 168).
template <int WHICH, int MS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WHICH == 3 ? 3 : 4)))
void msssim3f_adjoint_kernel(const KM3Args args)
{
    static_assert(MS == kMsLast || MS == kMsUp, "the single-scale adjoint stays in ssim3f_kernels.hip");
    adjoint_body<SampleF32, 5, WHICH, MS>(args);
}

// ---- pyramid, reduction, product, coefficients ------------------------------------------------------------------------------------------

// One step of the pyramid: work-item = one voxel of scale s + 1 of one pair, x fastest, A and B.  src is read through its descriptor
// (scale 0: the caller's strides), coordinates clamped to scale s; dst volumes are dense.
__device__ __forceinline__ float down8(const float* base, int64_t step, int64_t stride, int64_t slice, int64_t x0, int64_t x1, int64_t y0,
                                       int64_t y1, int64_t z0, int64_t z1)
{
    const gptr_cf32 p = (gptr_cf32)base;
    const float n00 = p[x0 * step + y0 * stride + z0 * slice] + p[x1 * step + y0 * stride + z0 * slice];
    const float n10 = p[x0 * step + y1 * stride + z0 * slice] + p[x1 * step + y1 * stride + z0 * slice];
    const float n01 = p[x0 * step + y0 * stride + z1 * slice] + p[x1 * step + y0 * stride + z1 * slice];
    const float n11 = p[x0 * step + y1 * stride + z1 * slice] + p[x1 * step + y1 * stride + z1 * slice];
    return ((n00 + n10) + (n01 + n11)) * 0.125f;
}

__global__ __launch_bounds__(256)
void msssim3f_down_kernel(const Pair3FDesc* __restrict__ src, const Pair3FDesc* __restrict__ dst, uint32_t src_w, uint32_t src_h, uint32_t src_d,
                          uint32_t dst_w, uint32_t dst_h, uint32_t dst_d, uint32_t blocks_per_volume)
{
    const uint32_t vol = blockIdx.x / blocks_per_volume, blk = blockIdx.x - vol * blocks_per_volume;
    const uint64_t idx = (uint64_t)blk * 256 + threadIdx.x, plane = (uint64_t)dst_w * dst_h;
    if (idx >= plane * dst_d) return;
    const uint32_t z = (uint32_t)(idx / plane);
    const uint64_t rem = idx - (uint64_t)z * plane;
    const uint32_t y = (uint32_t)(rem / dst_w), x = (uint32_t)(rem - (uint64_t)y * dst_w);
    const Pair3FDesc s = src[vol];
    const Pair3FDesc d = dst[vol];
    const int64_t x0 = 2 * (int64_t)x, x1 = x0 + 1 < (int64_t)src_w ? x0 + 1 : (int64_t)src_w - 1;
    const int64_t y0 = 2 * (int64_t)y, y1 = y0 + 1 < (int64_t)src_h ? y0 + 1 : (int64_t)src_h - 1;
    const int64_t z0 = 2 * (int64_t)z, z1 = z0 + 1 < (int64_t)src_d ? z0 + 1 : (int64_t)src_d - 1;
    ((gptr_f32)const_cast<float*>(d.a))[idx] = down8(s.a, s.a_step, s.a_stride, s.a_slice, x0, x1, y0, y1, z0, z1);
    ((gptr_f32)const_cast<float*>(d.b))[idx] = down8(s.b, s.b_step, s.b_stride, s.b_slice, x0, x1, y0, y1, z0, z1);
}

struct KR3Args {
    const double* partials;
    double*       means;                      // [pair][scale]{mcs, mssim}
    uint32_t      count, scales;
    uint64_t      offset[kMS3MaxScales];      // of a scale's partials, in doubles
    uint64_t      cells[kMS3MaxScales];       // per volume
    double        voxels[kMS3MaxScales];      // double(W_s) * double(H_s) * double(D_s)
};

// Workgroup (pair, scale, kind), in ssim3f_reduce_kernel's order: thread t of 1024 adds cells t, t + 1024, ... in that order, each wave
// runs a fixed xor butterfly, and the 16 wave totals are added in wave order.  The ssim sum has the bits of that kernel's.
constexpr int kReduceThreads = 1024;

__global__ __launch_bounds__(kReduceThreads) void msssim3f_reduce_kernel(const KR3Args args)
{
    __shared__ double sh[kReduceThreads / 64];
    const uint32_t kind = blockIdx.x & 1u, rest = blockIdx.x >> 1;
    const uint32_t s = rest % args.scales, vol = rest / args.scales;
    const uint64_t cells = args.cells[s];
    const double* p = args.partials + args.offset[s] + (uint64_t)vol * cells * 2 + kind;
    double acc = 0.0;
    for (uint64_t i = threadIdx.x; i < cells; i += kReduceThreads)
        acc += p[2 * i];
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
        args.means[((size_t)vol * args.scales + s) * 2 + kind] = t / args.voxels[s];
    }
}

struct KW3Args {
    uint32_t count, scales;
    double   weights[kMS3MaxScales];
    double   voxels[kMS3MaxScales];
};

// The mean scale s contributes: mcs_s, or mssim_s for the last scale.
__device__ __forceinline__ double scale_mean(const double* means, uint32_t s, uint32_t scales) { return means[2 * s + (s + 1 == scales ? 1 : 0)]; }

// prod max(m_s, 0)^w_s with x^0 = 1; a NaN mean stays a NaN.
__device__ __forceinline__ double ms_product(const double* means, const KW3Args& a)
{
    double r = 1.0;
    for (uint32_t s = 0; s < a.scales; ++s) {
        if (a.weights[s] == 0.0) continue;
        const double m = scale_mean(means, s, a.scales);
        r *= pow(m <= 0.0 ? 0.0 : m, a.weights[s]);
    }
    return r;
}

__global__ __launch_bounds__(64) void msssim3f_finalise_kernel(const KW3Args args, const double* __restrict__ means, double* __restrict__ values)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= args.count) return;
    values[i] = ms_product(means + (size_t)i * args.scales * 2, args);
}

// k_s of every pair and scale as [scale][pair], rounded to float once; all 0 when MS = 0 (the ReLU's subgradient), when gOut = 0 (whatever
// the means are, NaN included) and where w_s = 0.
__global__ __launch_bounds__(64) void msssim3f_coef_kernel(const KW3Args args, const double* __restrict__ means, const float* __restrict__ g_out,
                                                           float* __restrict__ ks)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= args.count) return;
    const double* m = means + (size_t)i * args.scales * 2;
    const double ms = ms_product(m, args);
    const double g = (double)g_out[i];
    for (uint32_t s = 0; s < args.scales; ++s) {
        double k = 0.0;
        if (ms != 0.0 && g != 0.0 && args.weights[s] != 0.0)
            k = g * args.weights[s] * ms / scale_mean(m, s, args.scales) / args.voxels[s];
        ks[(size_t)s * args.count + i] = (float)k;
    }
}

const uint64_t kMaxBlocks = (uint64_t(1) << 24) - 1;      // x 256 work-items stays below 2^32

bool valid_call(uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, float data_range, const double* weights)
{
    if (!(data_range > 0.0f) || !std::isfinite(data_range) || scales < 1 || scales > kMS3MaxScales || weights == nullptr) return false;
    for (uint32_t s = 0; s < scales; ++s)
        if (!std::isfinite(weights[s]) || weights[s] < 0.0) return false;
    return count <= msssim3f_max_count(width, height, depth);
}

KW3Args weight_args(uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, const double* weights)
{
    KW3Args a;
    a.count = count; a.scales = scales;
    for (uint32_t s = 0; s < kMS3MaxScales; ++s) {
        a.weights[s] = s < scales ? weights[s] : 0.0;
        a.voxels[s] = (double)ms3_dim(width, s) * (double)ms3_dim(height, s) * (double)ms3_dim(depth, s);
    }
    return a;
}

// The pyramid of `count` pairs from scale `first` down: one launch per step, finest first.
hipError_t launch_pyramid(uint32_t first, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales,
                          hipStream_t stream)
{
    for (uint32_t s = first; s + 1 < scales; ++s) {
        const uint32_t sw = ms3_dim(width, s), sh = ms3_dim(height, s), sd = ms3_dim(depth, s);
        const uint32_t dw = ms3_dim(width, s + 1), dh = ms3_dim(height, s + 1), dd = ms3_dim(depth, s + 1);
        const uint64_t per = ((uint64_t)dw * dh * dd + 255) / 256;
        if (per * count > kMaxBlocks) return hipErrorInvalidValue;
        hipLaunchKernelGGL(msssim3f_down_kernel, dim3((uint32_t)(per * count)), dim3(256), 0, stream, descs_dev + (size_t)s * count,
                           descs_dev + (size_t)(s + 1) * count, sw, sh, sd, dw, dh, dd, (uint32_t)per);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

uint32_t msssim3f_max_count(uint32_t width, uint32_t height, uint32_t depth)
{
    const uint32_t walk = ssim3f_max_count(width, height, depth);
    if (walk == 0) return 0;
    // the pyramid step into scale 1 has the most work-items of all steps; the walks of scales >= 1 have fewer tiles than scale 0's
    const uint64_t per = (ms3_voxels(width, height, depth, 1) + 255) / 256;
    return (uint32_t)std::min<uint64_t>(walk, kMaxBlocks / per);
}

uint64_t msssim3f_scratch_bytes(uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int grad_planes)
{
    const uint64_t pyr = ms3_pyramid_floats(width, height, depth, scales);
    if (grad_planes == 0)
        return 2 * pyr * sizeof(float) + ms3_partials(width, height, depth, 1, scales) * sizeof(double);
    return (2 + (uint64_t)grad_planes) * pyr * sizeof(float) + (uint64_t)ssim3f_coef_planes(grad_planes == 2 ? 3 : 1) * ms3_voxels(width, height, depth, 0) * sizeof(float) +
           scales * sizeof(float);
}

uint32_t msssim3f_per_sub_batch(uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int grad_planes, uint64_t cap)
{
    const uint64_t fit = cap / msssim3f_scratch_bytes(width, height, depth, scales, grad_planes);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(fit, msssim3f_max_count(width, height, depth)));
}

// ---- the steps that do not depend on the window, for this file's launchers and for msssim3k_kernels.hip's ---------------------------------

hipError_t launch_msssim3f_pyramid(uint32_t first_scale, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth,
                                   uint32_t scales, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (first_scale > 1 || scales < 1 || scales > kMS3MaxScales || count > msssim3f_max_count(width, height, depth)) return hipErrorInvalidValue;
    return launch_pyramid(first_scale, descs_dev, count, width, height, depth, scales, stream);
}

hipError_t launch_msssim3f_means(uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, const double* weights,
                                 const double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(count, width, height, depth, scales, 1.0f, weights)) return hipErrorInvalidValue;
    KR3Args kr;
    kr.partials = partials; kr.means = means; kr.count = count; kr.scales = scales;
    for (uint32_t s = 0; s < kMS3MaxScales; ++s) { kr.offset[s] = 0; kr.cells[s] = 0; kr.voxels[s] = 1.0; }
    uint64_t offset = 0;
    for (uint32_t s = 0; s < scales; ++s) {
        kr.offset[s] = offset; kr.cells[s] = ms3_cells(width, height, depth, s);
        kr.voxels[s] = (double)ms3_dim(width, s) * (double)ms3_dim(height, s) * (double)ms3_dim(depth, s);
        offset += kr.cells[s] * 2 * count;
    }
    hipLaunchKernelGGL(msssim3f_reduce_kernel, dim3(count * scales * 2), dim3(kReduceThreads), 0, stream, kr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(msssim3f_finalise_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, weight_args(count, width, height, depth, scales, weights),
                       means, values);
    return hipGetLastError();
}

hipError_t launch_msssim3f_coef(uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, const double* weights,
                                const double* means, const float* g_out, float* ks, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(count, width, height, depth, scales, 1.0f, weights)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(msssim3f_coef_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, weight_args(count, width, height, depth, scales, weights),
                       means, g_out, ks);
    return hipGetLastError();
}

// ---- the launchers of the 11-tap window -----------------------------------------------------------------------------------------------------

// first_scale 1 (msssim3h_kernels.hip): scale 0 is the caller's -- its pyramid step and its walk, whose partials lie first -- and row 0
// of descs_dev is not read.  The layout of the partials, the reduction and the product are the same.
hipError_t launch_msssim3f_from(uint32_t first_scale, uint32_t radius, const float* taps, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width,
                                uint32_t height, uint32_t depth, uint32_t scales, float data_range, const double* weights, int cu_count,
                                double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (first_scale > 1 || radius != 5 || !valid_call(count, width, height, depth, scales, data_range, weights)) return hipErrorInvalidValue;
    hipError_t e = launch_pyramid(first_scale, descs_dev, count, width, height, depth, scales, stream);
    if (e != hipSuccess) return e;
    uint64_t offset = 0;
    for (uint32_t s = 0; s < scales; ++s) {
        const uint32_t w = ms3_dim(width, s), h = ms3_dim(height, s), d = ms3_dim(depth, s);
        const Geometry3F geo = plan3f(w, h, d, count, cu_count);
        K3Args ka;
        if (!fill_args(ka, geo, data_range, radius, taps)) return hipErrorInvalidValue;
        ka.descs = descs_dev + (size_t)s * count;
        ka.partials = partials + offset;
        offset += geo.cells_per_volume() * 2 * count;
        if (s < first_scale) continue;
        hipLaunchKernelGGL((msssim3f_walk_kernel<0, kFormMulti>), grid_of(geo), dim3(256), 0, stream, ka);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_msssim3f_means(count, width, height, depth, scales, weights, partials, means, values, stream);
}

hipError_t launch_msssim3f(const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales,
                           float data_range, const double* weights, int cu_count, double* partials, double* means, double* values,
                           hipStream_t stream)
{
    return launch_msssim3f_from(0, 5, NULL, descs_dev, count, width, height, depth, scales, data_range, weights, cu_count, partials, means, values, stream);
}

// first_scale 1: the k_s of every scale, the pyramid from scale 1 down, the walks from the coarsest scale down to scale 1; rows 0 of
// descs_dev and grads_dev are not read.
hipError_t launch_msssim3f_grad_from(uint32_t first_scale, uint32_t radius, const float* taps, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev,
                                     uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, float data_range,
                                     const double* weights, int cu_count, const double* means, const float* g_out, float* ks, float* coef, int which,
                                     hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (first_scale > 1 || radius != 5 || !valid_call(count, width, height, depth, scales, data_range, weights) || which < 1 || which > 3)
        return hipErrorInvalidValue;
    hipError_t e = launch_msssim3f_coef(count, width, height, depth, scales, weights, means, g_out, ks, stream);
    if (e != hipSuccess) return e;
    if ((e = launch_pyramid(first_scale, descs_dev, count, width, height, depth, scales, stream)) != hipSuccess) return e;
    for (uint32_t s = scales; s-- > first_scale;) {
        const bool last = s + 1 == scales;
        const Geometry3F geo = plan3f(ms3_dim(width, s), ms3_dim(height, s), ms3_dim(depth, s), count, cu_count);
        KM3Args ka;
        if (!fill_args(ka, geo, data_range, radius, taps)) return hipErrorInvalidValue;
        ka.descs = descs_dev + (size_t)s * count;
        ka.grads = grads_dev + (size_t)s * count;
        ka.up = last ? nullptr : grads_dev + (size_t)(s + 1) * count;
        ka.g_out = ks + (size_t)s * count;
        ka.coef = coef;
        const K3Args& kw = ka;
        with_constant<1, 3>(which, [&](auto MODE) {
            if (last) hipLaunchKernelGGL((msssim3f_walk_kernel<MODE(), kFormSsim>), grid_of(geo), dim3(256), 0, stream, kw);
            else      hipLaunchKernelGGL((msssim3f_walk_kernel<MODE(), kFormMulti>), grid_of(geo), dim3(256), 0, stream, kw);
            return true; });
        if ((e = hipGetLastError()) != hipSuccess) return e;
        with_constant<1, 3>(which, [&](auto WHICH) {
            if (last) hipLaunchKernelGGL((msssim3f_adjoint_kernel<WHICH(), kMsLast>), grid_of(geo), dim3(256), 0, stream, ka);
            else      hipLaunchKernelGGL((msssim3f_adjoint_kernel<WHICH(), kMsUp>), grid_of(geo), dim3(256), 0, stream, ka);
            return true; });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_msssim3f_grad(const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height,
                                uint32_t depth, uint32_t scales, float data_range, const double* weights, int cu_count, const double* means,
                                const float* g_out, float* ks, float* coef, int which, hipStream_t stream)
{
    return launch_msssim3f_grad_from(0, 5, NULL, descs_dev, grads_dev, count, width, height, depth, scales, data_range, weights, cu_count, means, g_out, ks,
                                     coef, which, stream);
}

} // namespace ssim_hip
