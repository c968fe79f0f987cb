// msssimhk_kernels.hip -- gfx950 kernels of scale 0 of multi-scale SSIM on float16 / bfloat16 samples, and of its gradient, under a
// window of 3, 5, 7 or 9 taps (radius R = 1 .. 4), behind rmgr_ssim_hip_enqueue_msssimh_win, rmgr_ssim_hip_compute_msssimh_win_device /
// _host and rmgr_ssim_hip_enqueue_msssimh_win_grad.  The definition they implement is in include/rmgr/ssim-hip.h: msssimf_win's, applied
// to the samples widened to float32, with the gradient rounded once into the samples' encoding.  Windows of 11 taps run on
// msssimh_kernels.hip with the window's taps.
//
// Only scale 0 touches 16-bit memory, so only scale 0 has kernels here; scales >= 1 run on msssimk_kernels.hip.  This is the strip kernel
// and the gradient kernel of msssimk_kernels.hip under the sample policy of msssimh_kernels.hip: the bodies of ssim2_walk.h in their
// multi-scale forms with R = 1 .. 4 and SampleH<TYPE>.  Both template axes are those files'; no line of a body is written here.  Those
// files' kernels are counted by their tests, hence a file of its own.  The pyramid step from scale 0 is msssimh_kernels.hip's (launch_msssimh_down).
//  * msssimhk_strip_kernel<TYPE, R, WIDE>: strip_body in the form kFormMulti.
//  * msssimhk_grad_kernel<TYPE, R, WHICH, LAST>: grad_body with kKCoef, kMsUp or -- LAST: scales == 1 -- kMsLast.
#include "ssim2_walk.h"
#include "msssimk_kernels.h"

namespace ssim_hip {
namespace {

// TYPE: kSHTypeF16 or kSHTypeBF16, the encoding of the samples.
template <int TYPE, int R, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void msssimhk_strip_kernel(const Strip2Args<PairHDesc> args) { strip_body<SampleH<TYPE>, R, kFormMulti, 0, WIDE>(args); }

template <int TYPE, int R, int WHICH, bool LAST>
__global__ __launch_bounds__(256)
void msssimhk_grad_kernel(const Grad2Args<PairHDesc, GradHDesc> args) { grad_body<SampleH<TYPE>, R, WHICH, kKCoef, LAST ? kMsLast : kMsUp>(args); }

bool valid_type(int type) { return type == kSHTypeF16 || type == kSHTypeBF16; }

} // namespace

hipError_t launch_msssimhk(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                           uint32_t scales, int type, bool wide, float data_range, uint32_t radius, const float (&gf)[kSKMaxRadius + 1],
                           const double* weights, int cu_count, int xcd_count, double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_type(type) || !valid_range(data_range) || radius < 1 || radius > 4 || scales < 1 || scales > kMSFMaxScales ||
        count > msssimf_max_count(width, height))
        return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1 && (e = launch_msssimh_down(descs0_dev, descs_dev, count, width, height, type, stream)) != hipSuccess) return e;
    // scale 0's strips and cells, as launch_msssimk_from lays them out: its partials come first
    const GeometryF geo = plank(radius, width, height, count, cu_count);
    const Strip2Args<PairHDesc> ka = fill_strip(geo, descs0_dev, data_range, gf, xcd_count, partials);
    pick_type(type, [&](auto t) {
        pick_radius4(radius, [&](auto r) {
            pick_bool(wide, [&](auto w) {
                hipLaunchKernelGGL((msssimhk_strip_kernel<decltype(t)::value, decltype(r)::value, decltype(w)::value>), strip_grid(geo), dim3(64), 0,
                                   stream, ka);
            });
        });
    });
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_msssimk_from(1, radius, gf, descs_dev, count, width, height, scales, false, data_range, weights, cu_count, xcd_count, partials, means,
                               values, stream);
}

hipError_t launch_msssimhk_grad(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, const GradHDesc* grads0_dev, const GradFDesc* grads_dev,
                                uint32_t count, uint32_t width, uint32_t height, uint32_t scales, int type, float data_range, uint32_t radius,
                                const float (&gf)[kSKMaxRadius + 1], const double* weights, const double* means, const float* g_out, float* coef,
                                int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_type(type) || !valid_range(data_range) || radius < 1 || radius > 4 || scales < 1 || scales > kMSFMaxScales || which < 1 || which > 3 ||
        count > msssimf_max_count(width, height))
        return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1 && (e = launch_msssimh_down(descs0_dev, descs_dev, count, width, height, type, stream)) != hipSuccess) return e;
    // the coefficients of every scale, the rest of the pyramid, the float32 gradients from the coarsest scale down to scale 1
    if ((e = launch_msssimk_grad_from(1, radius, gf, descs_dev, grads_dev, count, width, height, scales, data_range, weights, means, g_out, coef, which,
                                      stream)) != hipSuccess)
        return e;
    const bool last = scales == 1;
    Grad2Args<PairHDesc, GradHDesc> ka = fill_grad(width, height, descs0_dev, grads0_dev, data_range, radius, gf);
    ka.up = last ? nullptr : grads_dev + (size_t)count;
    ka.g_out = coef; ka.g_out_stride = scales;              // k_0 of pair i at coef[i * scales]
    pick_type(type, [&](auto t) {
        pick_radius4(radius, [&](auto r) {
            pick_bool(last, [&](auto l) {
                pick_which(which, [&](auto wh) {
                    hipLaunchKernelGGL((msssimhk_grad_kernel<decltype(t)::value, decltype(r)::value, decltype(wh)::value, decltype(l)::value>),
                                       grad_grid(ka, count), dim3(256), 0, stream, ka);
                });
            });
        });
    });
    return hipGetLastError();
}

} // namespace ssim_hip
