// msssim3hk_kernels.hip -- gfx950 kernels of scale 0 of multi-scale SSIM on float16 / bfloat16 VOLUMES, and of its gradient, under a
// window of 3, 5, 7 or 9 taps per axis (radius R = 1 .. 4), behind rmgr_ssim_hip_enqueue_msssim3h_win,
// rmgr_ssim_hip_compute_msssim3h_win_device / _host and rmgr_ssim_hip_enqueue_msssim3h_win_grad.  The definition they implement is in
// include/rmgr/ssim-hip.h: msssim3f_win's, applied to the samples widened to float32, with the gradient rounded once into the samples'
// encoding.  Windows of 11 taps run on msssim3h_kernels.hip with the window's taps.
//
// Only scale 0 touches 16-bit memory, so only scale 0 has kernels here; scales >= 1 run on msssim3k_kernels.hip.  These are that file's
// walk and adjoint walk under the sample policy of msssim3h_kernels.hip: the bodies of ssim3_walk.h in their multi-scale forms with
// R = 1 .. 4 and SampleH<TYPE>.  Both template axes are those files'; no line of a body is written here.  Those files' kernels are counted
// by their tests, hence a file of its own.  The pyramid step from scale 0 is msssim3h_kernels.hip's (launch_msssim3h_down).
//  * msssim3hk_walk_kernel<TYPE, R, 0, kFormMulti>: scale 0's value walk, two fp64 column sums and two partials per cell.
//  * msssim3hk_walk_kernel<TYPE, R, MODE, FORM>, MODE 1 / 2 / 3: scale 0's coefficient volumes under k_0 (kKScale); the cs form, and the
//    ssim form when scale 0 is the only scale.
//  * msssim3hk_adjoint_kernel<TYPE, R, WHICH, MS>: kMsUp adds scale 1's float32 gradient (args.up: Grad3FDesc) before the single rounding
//    and store; kMsLast when scale 0 is the only scale.
#include "msssim3hk_kernels.h"
#include "ssim3_walk.h"
#include <cmath>

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleH<kSHTypeF16>> K3HArgs;      // the same struct for both encodings

// What the adjoint takes besides when a coarser scale exists: scale 1's gradient volumes, float32, one Grad3FDesc per pair.
struct KM3HArgs : K3HArgs {
    const Grad3FDesc* up;
};

// TYPE: kSHTypeF16 or kSHTypeBF16, the encoding of the samples.
template <int TYPE, int R, int MODE, int FORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void msssim3hk_walk_kernel(const K3HArgs args)
{
    walk_body<SampleH<TYPE>, R, MODE, MODE == 0 ? kKUniform : kKScale, FORM>(args);
}

// The occupancies of msssim3k_adjoint_kernel<R, WHICH, MS>: three waves per SIMD for both gradients, four for one.
template <int TYPE, int R, int WHICH, int MS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WHICH == 3 ? 3 : 4)))
void msssim3hk_adjoint_kernel(const KM3HArgs args)
{
    static_assert(MS == kMsLast || MS == kMsUp, "the single-scale adjoint stays in ssim3hk_kernels.hip");
    adjoint_body<SampleH<TYPE>, R, WHICH, MS>(args);
}

static_assert(kSHTypeF16 == 0 && kSHTypeBF16 == 1, "the dispatch on the encoding");

bool valid_call(int type, uint32_t radius, uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, float data_range,
                const double* weights)
{
    return (type == kSHTypeF16 || type == kSHTypeBF16) && radius >= 1 && radius <= 4 && data_range > 0.0f && std::isfinite(data_range) &&
           scales >= 1 && scales <= kMS3MaxScales && weights != nullptr && count <= msssim3f_max_count(width, height, depth);
}

} // namespace

hipError_t launch_msssim3hk(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                            uint32_t depth, uint32_t scales, int type, float data_range, uint32_t radius, const float (&gf)[kSKMaxRadius + 1],
                            const double* weights, int cu_count, double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(type, radius, count, width, height, depth, scales, data_range, weights)) return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1 && (e = launch_msssim3h_down(descs0_dev, descs_dev, count, width, height, depth, type, stream)) != hipSuccess) return e;
    // scale 0's tiles and cells, as launch_msssim3k_from lays them out: its partials come first
    const Geometry3F geo = plan3k(radius, width, height, depth, count, cu_count);
    K3HArgs ka;
    if (!fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
    ka.descs = descs0_dev;
    ka.partials = partials;
    if (!with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 4>(radius, [&](auto R) {
            hipLaunchKernelGGL((msssim3hk_walk_kernel<TYPE(), R(), 0, kFormMulti>), grid_of(geo), dim3(256), 0, stream, ka);
            return true; }); }))
        return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_msssim3k_from(1, radius, gf, descs_dev, count, width, height, depth, scales, data_range, weights, cu_count, partials, means, values,
                                stream);
}

hipError_t launch_msssim3hk_grad(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, const Grad3HDesc* grads0_dev, const Grad3FDesc* grads_dev,
                                 uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int type, float data_range,
                                 uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const double* weights, int cu_count, const double* means,
                                 const float* g_out, float* ks, float* coef, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(type, radius, count, width, height, depth, scales, data_range, weights) || which < 1 || which > 3) return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1 && (e = launch_msssim3h_down(descs0_dev, descs_dev, count, width, height, depth, type, stream)) != hipSuccess) return e;
    // the k_s of every scale, the rest of the pyramid, the float32 gradients from the coarsest scale down to scale 1
    if ((e = launch_msssim3k_grad_from(1, radius, gf, descs_dev, grads_dev, count, width, height, depth, scales, data_range, weights, cu_count, means,
                                       g_out, ks, coef, which, stream)) != hipSuccess)
        return e;
    const bool last = scales == 1;
    const Geometry3F geo = plan3k(radius, width, height, depth, count, cu_count);
    KM3HArgs ka;
    if (!fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
    ka.descs = descs0_dev;
    ka.grads = grads0_dev;
    ka.up = last ? nullptr : grads_dev + (size_t)count;
    ka.g_out = ks;                                          // k_0 of pair i at ks[i]
    ka.coef = coef;
    const K3HArgs& kw = ka;
    if (!with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 4>(radius, [&](auto R) { return with_constant<1, 3>(which, [&](auto MODE) {
            if (last) hipLaunchKernelGGL((msssim3hk_walk_kernel<TYPE(), R(), MODE(), kFormSsim>), grid_of(geo), dim3(256), 0, stream, kw);
            else      hipLaunchKernelGGL((msssim3hk_walk_kernel<TYPE(), R(), MODE(), kFormMulti>), grid_of(geo), dim3(256), 0, stream, kw);
            return true; }); }); }))
        return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 4>(radius, [&](auto R) { return with_constant<1, 3>(which, [&](auto WHICH) {
            if (last) hipLaunchKernelGGL((msssim3hk_adjoint_kernel<TYPE(), R(), WHICH(), kMsLast>), grid_of(geo), dim3(256), 0, stream, ka);
            else      hipLaunchKernelGGL((msssim3hk_adjoint_kernel<TYPE(), R(), WHICH(), kMsUp>), grid_of(geo), dim3(256), 0, stream, ka);
            return true; }); }); }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace ssim_hip
