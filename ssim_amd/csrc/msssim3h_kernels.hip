// msssim3h_kernels.hip -- gfx950 kernels of multi-scale SSIM on float16 / bfloat16 VOLUMES and of its gradient, behind
// rmgr_ssim_hip_enqueue_msssim3h, rmgr_ssim_hip_compute_msssim3h_device / _host and rmgr_ssim_hip_enqueue_msssim3h_grad.  The definition
// they implement is in include/rmgr/ssim-hip.h: msssim3f's, applied to the samples widened to float32, with the gradient rounded once
// into the samples' encoding.
//
// Only scale 0 touches 16-bit memory -- the pyramid is float32 from scale 1 on -- so only scale 0 has kernels here, all of them
// ssim3_walk.h's bodies under the sample policy SampleH<TYPE> at R = 5, msssim3f_kernels.hip's instantiations with another policy:
//  * msssim3h_walk_kernel<TYPE, 0, kFormMulti>: scale 0's value walk, two fp64 column sums and two partials per cell.
//  * msssim3h_walk_kernel<TYPE, MODE, FORM>, MODE 1 / 2 / 3: scale 0's coefficient volumes under k_0 (kKScale); the cs form, and the ssim
//    form when scale 0 is the only scale.
//  * msssim3h_adjoint_kernel<TYPE, WHICH, MS>: kMsUp adds scale 1's float32 gradient (args.up: Grad3FDesc) before the single rounding and
//    store; kMsLast when scale 0 is the only scale.
//  * msssim3h_down_kernel<TYPE>: msssim3f_down_kernel with widened loads; from the eight widened samples on every instruction is
//    msssim3f's, and the scale-1 volume has the bits of msssim3f on the widened volumes.
// Scales >= 1, the reduction, the product and the coefficients k_s run on msssim3f_kernels.hip's kernels (launch_msssim3f_from,
// launch_msssim3f_grad_from) over the same partials layout, pyramid and coarse gradient volumes.
#include "msssim3h_kernels.h"
#include "ssim3_walk.h"
#include <cmath>

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleH<kSHTypeF16>> K3HArgs;      // the same struct for both encodings

// What the adjoint takes besides when a coarser scale exists: scale 1's gradient volumes, float32, one Grad3FDesc per pair.
struct KM3HArgs : K3HArgs {
    const Grad3FDesc* up;
};

template <int TYPE, int MODE, int FORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void msssim3h_walk_kernel(const K3HArgs args)
{
    walk_body<SampleH<TYPE>, 5, MODE, MODE == 0 ? kKUniform : kKScale, FORM>(args);
}

// The occupancies of msssim3f_adjoint_kernel<WHICH, MS>: three waves per SIMD for both gradients, four for one.
template <int TYPE, int WHICH, int MS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WHICH == 3 ? 3 : 4)))
void msssim3h_adjoint_kernel(const KM3HArgs args)
{
    static_assert(MS == kMsLast || MS == kMsUp, "the single-scale adjoint stays in ssim3h_kernels.hip");
    adjoint_body<SampleH<TYPE>, 5, WHICH, MS>(args);
}

// ---- the pyramid step ------------------------------------------------------------------------------------------------------------------

// Eight widened samples of one image at the caller's three strides, added in msssim3f's order.
template <int TYPE>
__device__ __forceinline__ float down8h(const uint16_t* base, int64_t step, int64_t stride, int64_t slice, int64_t x0, int64_t x1, int64_t y0,
                                        int64_t y1, int64_t z0, int64_t z1)
{
    const gptr_cu16 p = (gptr_cu16)base;
    const float n00 = widen<TYPE>(p[x0 * step + y0 * stride + z0 * slice]) + widen<TYPE>(p[x1 * step + y0 * stride + z0 * slice]);
    const float n10 = widen<TYPE>(p[x0 * step + y1 * stride + z0 * slice]) + widen<TYPE>(p[x1 * step + y1 * stride + z0 * slice]);
    const float n01 = widen<TYPE>(p[x0 * step + y0 * stride + z1 * slice]) + widen<TYPE>(p[x1 * step + y0 * stride + z1 * slice]);
    const float n11 = widen<TYPE>(p[x0 * step + y1 * stride + z1 * slice]) + widen<TYPE>(p[x1 * step + y1 * stride + z1 * slice]);
    return ((n00 + n10) + (n01 + n11)) * 0.125f;
}

// The pyramid step from scale 0 to scale 1: work-item = one voxel of scale 1 of one pair, x fastest, A and B; coordinates clamped to
// scale 0; dst volumes are dense float32.
template <int TYPE>
__global__ __launch_bounds__(256)
void msssim3h_down_kernel(const Pair3HDesc* __restrict__ src, const Pair3FDesc* __restrict__ dst, uint32_t src_w, uint32_t src_h, uint32_t src_d,
                          uint32_t dst_w, uint32_t dst_h, uint32_t dst_d, uint32_t blocks_per_volume)
{
    const uint32_t vol = blockIdx.x / blocks_per_volume, blk = blockIdx.x - vol * blocks_per_volume;
    const uint64_t idx = (uint64_t)blk * 256 + threadIdx.x, plane = (uint64_t)dst_w * dst_h;
    if (idx >= plane * dst_d) return;
    const uint32_t z = (uint32_t)(idx / plane);
    const uint64_t rem = idx - (uint64_t)z * plane;
    const uint32_t y = (uint32_t)(rem / dst_w), x = (uint32_t)(rem - (uint64_t)y * dst_w);
    const Pair3HDesc s = src[vol];
    const Pair3FDesc d = dst[vol];
    const int64_t x0 = 2 * (int64_t)x, x1 = x0 + 1 < (int64_t)src_w ? x0 + 1 : (int64_t)src_w - 1;
    const int64_t y0 = 2 * (int64_t)y, y1 = y0 + 1 < (int64_t)src_h ? y0 + 1 : (int64_t)src_h - 1;
    const int64_t z0 = 2 * (int64_t)z, z1 = z0 + 1 < (int64_t)src_d ? z0 + 1 : (int64_t)src_d - 1;
    ((gptr_f32)const_cast<float*>(d.a))[idx] = down8h<TYPE>(s.a, s.a_step, s.a_stride, s.a_slice, x0, x1, y0, y1, z0, z1);
    ((gptr_f32)const_cast<float*>(d.b))[idx] = down8h<TYPE>(s.b, s.b_step, s.b_stride, s.b_slice, x0, x1, y0, y1, z0, z1);
}

static_assert(kSHTypeF16 == 0 && kSHTypeBF16 == 1, "the dispatch on the encoding");

// What launch_msssim3f_from checks as well; here before scale 0's own launches.
bool valid_call(uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int type, float data_range, const double* weights)
{
    if (type != kSHTypeF16 && type != kSHTypeBF16) return false;
    if (!(data_range > 0.0f) || !std::isfinite(data_range) || scales < 1 || scales > kMS3MaxScales || weights == nullptr) return false;
    for (uint32_t s = 0; s < scales; ++s)
        if (!std::isfinite(weights[s]) || weights[s] < 0.0) return false;
    return count <= msssim3f_max_count(width, height, depth);
}

// The pyramid step from the caller's volumes into row 1 of descs_dev; count <= msssim3f_max_count keeps the grid below 2^24 blocks.
hipError_t launch_down(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth,
                       int type, hipStream_t stream)
{
    const uint32_t dw = ms3_dim(width, 1), dh = ms3_dim(height, 1), dd = ms3_dim(depth, 1);
    const uint64_t per = ((uint64_t)dw * dh * dd + 255) / 256;
    return with_constant<0, 1>(type, [&](auto TYPE) {
        hipLaunchKernelGGL((msssim3h_down_kernel<TYPE()>), dim3((uint32_t)(per * count)), dim3(256), 0, stream, descs0_dev, descs_dev + (size_t)count,
                           width, height, depth, dw, dh, dd, (uint32_t)per);
        return true; }) ? hipGetLastError() : hipErrorInvalidValue;
}

} // namespace

hipError_t launch_msssim3h_down(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                                uint32_t depth, int type, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (count > msssim3f_max_count(width, height, depth)) return hipErrorInvalidValue;
    return launch_down(descs0_dev, descs_dev, count, width, height, depth, type, stream);
}

hipError_t launch_msssim3h(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                           uint32_t depth, uint32_t scales, int type, float data_range, uint32_t radius, const float* taps, const double* weights,
                           int cu_count, double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (radius != 5 || !valid_call(count, width, height, depth, scales, type, data_range, weights)) return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1 && (e = launch_down(descs0_dev, descs_dev, count, width, height, depth, type, stream)) != hipSuccess) return e;
    // scale 0's tiles and cells, as launch_msssim3f_from lays them out: its partials come first
    const Geometry3F geo = plan3f(width, height, depth, count, cu_count);
    K3HArgs ka;
    if (!fill_args(ka, geo, data_range, radius, taps)) return hipErrorInvalidValue;
    ka.descs = descs0_dev;
    ka.partials = partials;
    if (!with_constant<0, 1>(type, [&](auto TYPE) {
            hipLaunchKernelGGL((msssim3h_walk_kernel<TYPE(), 0, kFormMulti>), grid_of(geo), dim3(256), 0, stream, ka);
            return true; }))
        return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_msssim3f_from(1, radius, taps, descs_dev, count, width, height, depth, scales, data_range, weights, cu_count, partials, means, values,
                                stream);
}

hipError_t launch_msssim3h_grad(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, const Grad3HDesc* grads0_dev, const Grad3FDesc* grads_dev,
                                uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int type, float data_range,
                                uint32_t radius, const float* taps, const double* weights, int cu_count, const double* means, const float* g_out,
                                float* ks, float* coef, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (radius != 5 || !valid_call(count, width, height, depth, scales, type, data_range, weights) || which < 1 || which > 3)
        return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1 && (e = launch_down(descs0_dev, descs_dev, count, width, height, depth, type, stream)) != hipSuccess) return e;
    // the k_s of every scale, the rest of the pyramid, the float32 gradients from the coarsest scale down to scale 1
    if ((e = launch_msssim3f_grad_from(1, radius, taps, descs_dev, grads_dev, count, width, height, depth, scales, data_range, weights, cu_count, means,
                                       g_out, ks, coef, which, stream)) != hipSuccess)
        return e;
    const bool last = scales == 1;
    const Geometry3F geo = plan3f(width, height, depth, count, cu_count);
    KM3HArgs ka;
    if (!fill_args(ka, geo, data_range, radius, taps)) return hipErrorInvalidValue;
    ka.descs = descs0_dev;
    ka.grads = grads0_dev;
    ka.up = last ? nullptr : grads_dev + (size_t)count;
    ka.g_out = ks;                                          // k_0 of pair i at ks[i]
    ka.coef = coef;
    const K3HArgs& kw = ka;
    if (!with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 3>(which, [&](auto MODE) {
            if (last) hipLaunchKernelGGL((msssim3h_walk_kernel<TYPE(), MODE(), kFormSsim>), grid_of(geo), dim3(256), 0, stream, kw);
            else      hipLaunchKernelGGL((msssim3h_walk_kernel<TYPE(), MODE(), kFormMulti>), grid_of(geo), dim3(256), 0, stream, kw);
            return true; }); }))
        return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 3>(which, [&](auto WHICH) {
            if (last) hipLaunchKernelGGL((msssim3h_adjoint_kernel<TYPE(), WHICH(), kMsLast>), grid_of(geo), dim3(256), 0, stream, ka);
            else      hipLaunchKernelGGL((msssim3h_adjoint_kernel<TYPE(), WHICH(), kMsUp>), grid_of(geo), dim3(256), 0, stream, ka);
            return true; }); }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace ssim_hip
