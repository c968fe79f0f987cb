// msssim3k_kernels.hip -- gfx950 kernels of one scale of multi-scale SSIM on float32 VOLUMES, and of its gradient, under a window of 3, 5,
// 7 or 9 taps per axis (radius R = 1 .. 4), behind rmgr_ssim_hip_enqueue_msssim3f_win, rmgr_ssim_hip_compute_msssim3f_win_device / _host
// and rmgr_ssim_hip_enqueue_msssim3f_win_grad, and behind the msssim3h_win entries from scale 1 on.  The definition they implement is in
// include/rmgr/ssim-hip.h; tests/msssim3k_model.py restates it in float64 and restates the arithmetic in fp32.  Windows of 11 taps run on
// msssim3f_kernels.hip with the window's taps.
//
// These are the walks and the adjoint walks of msssim3f_kernels.hip at another radius: the bodies of ssim3_walk.h in their multi-scale
// forms with SampleF32 at R = 1 .. 4; no line of a body is written here.  That file's kernels are counted by its tests, hence a file of
// its own.  The pyramid, the reduction, the product and the coefficients k_s do not depend on the window and stay in
// msssim3f_kernels.hip, whose launch_msssim3f_pyramid / _means / _coef the launchers below call.
//  * msssim3k_walk_kernel<R, 0, kFormMulti>: one scale's value walk with two fp64 column sums and two partials per cell.
//  * msssim3k_walk_kernel<R, MODE, FORM>, MODE 1 / 2 / 3: the coefficient volumes of one scale under k_s (kKScale); FORM kFormMulti (the
//    cs form) on every scale but the coarsest, kFormSsim on the coarsest.
//  * msssim3k_adjoint_kernel<R, WHICH, MS>: the adjoint walk; kMsUp adds the coarser scale's gradient before its single store, kMsLast
//    (the coarsest scale) has nothing to add.
// Tiles, chunks, cells, centring and summation orders: see the top of ssim3_walk.h; they are position-based and do not depend on the
// radius.
#include "msssim3k_kernels.h"
#include "ssim3_walk.h"
#include <cmath>

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleF32> K3Args;

// What the adjoint of a scale that is not the coarsest takes besides: the coarser scale's gradient volumes, one Grad3FDesc per pair.
struct KM3Args : K3Args {
    const Grad3FDesc* up;
};

template <int R, int MODE, int FORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void msssim3k_walk_kernel(const K3Args args)
{
    walk_body<SampleF32, R, MODE, MODE == 0 ? kKUniform : kKScale, FORM>(args);
}

// The occupancies of msssim3f_adjoint_kernel<WHICH, MS>: three waves per SIMD for both gradients, four for one.
template <int R, int WHICH, int MS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WHICH == 3 ? 3 : 4)))
void msssim3k_adjoint_kernel(const KM3Args args)
{
    static_assert(MS == kMsLast || MS == kMsUp, "the single-scale adjoint stays in ssim3k_kernels.hip");
    adjoint_body<SampleF32, R, WHICH, MS>(args);
}

bool valid_call(uint32_t first_scale, uint32_t radius, uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, float data_range,
                const double* weights)
{
    return first_scale <= 1 && radius >= 1 && radius <= 4 && data_range > 0.0f && std::isfinite(data_range) && scales >= 1 &&
           scales <= kMS3MaxScales && weights != nullptr && count <= msssim3f_max_count(width, height, depth);
}

} // namespace

hipError_t launch_msssim3k_from(uint32_t first_scale, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Pair3FDesc* descs_dev, uint32_t count,
                                uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, float data_range, const double* weights, int cu_count,
                                double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(first_scale, radius, count, width, height, depth, scales, data_range, weights)) return hipErrorInvalidValue;
    hipError_t e = launch_msssim3f_pyramid(first_scale, descs_dev, count, width, height, depth, scales, stream);
    if (e != hipSuccess) return e;
    uint64_t offset = 0;
    for (uint32_t s = 0; s < scales; ++s) {
        // the cells, and with them the partials, are plan3f()'s; a smaller window re-plans its chunks, which pay fewer warm-up slices
        const Geometry3F geo = plan3k(radius, ms3_dim(width, s), ms3_dim(height, s), ms3_dim(depth, s), count, cu_count);
        K3Args ka;
        if (!fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
        ka.descs = descs_dev + (size_t)s * count;
        ka.partials = partials + offset;
        offset += geo.cells_per_volume() * 2 * count;
        if (s < first_scale) continue;              // the caller's own walk fills this scale's partials
        if (!with_constant<1, 4>(radius, [&](auto R) {
                hipLaunchKernelGGL((msssim3k_walk_kernel<R(), 0, kFormMulti>), grid_of(geo), dim3(256), 0, stream, ka);
                return true; }))
            return hipErrorInvalidValue;
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_msssim3f_means(count, width, height, depth, scales, weights, partials, means, values, stream);
}

hipError_t launch_msssim3k_grad_from(uint32_t first_scale, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Pair3FDesc* descs_dev,
                                     const Grad3FDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales,
                                     float data_range, const double* weights, int cu_count, const double* means, const float* g_out, float* ks,
                                     float* coef, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(first_scale, radius, count, width, height, depth, scales, data_range, weights) || which < 1 || which > 3) return hipErrorInvalidValue;
    hipError_t e = launch_msssim3f_coef(count, width, height, depth, scales, weights, means, g_out, ks, stream);
    if (e != hipSuccess) return e;
    if ((e = launch_msssim3f_pyramid(first_scale, descs_dev, count, width, height, depth, scales, stream)) != hipSuccess) return e;
    for (uint32_t s = scales; s-- > first_scale;) {
        const bool last = s + 1 == scales;
        const Geometry3F geo = plan3k(radius, ms3_dim(width, s), ms3_dim(height, s), ms3_dim(depth, s), count, cu_count);
        KM3Args ka;
        if (!fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
        ka.descs = descs_dev + (size_t)s * count;
        ka.grads = grads_dev + (size_t)s * count;
        ka.up = last ? nullptr : grads_dev + (size_t)(s + 1) * count;
        ka.g_out = ks + (size_t)s * count;
        ka.coef = coef;
        const K3Args& kw = ka;
        if (!with_constant<1, 4>(radius, [&](auto R) { return with_constant<1, 3>(which, [&](auto MODE) {
                if (last) hipLaunchKernelGGL((msssim3k_walk_kernel<R(), MODE(), kFormSsim>), grid_of(geo), dim3(256), 0, stream, kw);
                else      hipLaunchKernelGGL((msssim3k_walk_kernel<R(), MODE(), kFormMulti>), grid_of(geo), dim3(256), 0, stream, kw);
                return true; }); }))
            return hipErrorInvalidValue;
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (!with_constant<1, 4>(radius, [&](auto R) { return with_constant<1, 3>(which, [&](auto WHICH) {
                if (last) hipLaunchKernelGGL((msssim3k_adjoint_kernel<R(), WHICH(), kMsLast>), grid_of(geo), dim3(256), 0, stream, ka);
                else      hipLaunchKernelGGL((msssim3k_adjoint_kernel<R(), WHICH(), kMsUp>), grid_of(geo), dim3(256), 0, stream, ka);
                return true; }); }))
            return hipErrorInvalidValue;
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace ssim_hip
