// msssimk_kernels.hip -- gfx950 kernels of one scale of multi-scale SSIM on float32 samples, and of its gradient, under a window of 3,
// 5, 7 or 9 taps (radius R = 1 .. 4), behind rmgr_ssim_hip_enqueue_msssimf_win, rmgr_ssim_hip_compute_msssimf_win_device / _host and
// rmgr_ssim_hip_enqueue_msssimf_win_grad, and behind the msssimh_win entries from scale 1 on.  The definition they implement is in
// include/rmgr/ssim-hip.h; tests/msssimk_model.py restates it in float64 and restates the arithmetic in fp32.  Windows of 11 taps run on
// msssimf_kernels.hip with the window's taps.
//
// This is the strip kernel and the gradient kernel of msssimf_kernels.hip at another radius: the bodies of ssim2_walk.h in their
// multi-scale forms with R = 1 .. 4; no line of a body is written here.  That file's kernels are counted by its tests, hence a file of
// its own.  The pyramid, the reduction, the product and the coefficients do not depend on the window and stay in msssimf_kernels.hip,
// whose launch_msssimf_pyramid / _means / _coef the launchers below call.
//  * msssimk_strip_kernel<R, WIDE>: strip_body in the form kFormMulti: no map, two fp64 sums per cell.
//  * msssimk_grad_kernel<R, WHICH, LAST>: grad_body with k_s read from device memory (kKCoef), the cs form (kMsUp) or -- LAST -- the
//    ssim form (kMsLast).
// Centring, cells, tiles and summation orders: see the top of ssim2_walk.h; they are position-based and do not depend on the radius.
#include "ssim2_walk.h"
#include "msssimk_kernels.h"

namespace ssim_hip {
namespace {

template <int R, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void msssimk_strip_kernel(const Strip2Args<PairFDesc> args) { strip_body<SampleF32, R, kFormMulti, 0, WIDE>(args); }

template <int R, int WHICH, bool LAST>
__global__ __launch_bounds__(256)
void msssimk_grad_kernel(const Grad2Args<PairFDesc, GradFDesc> args) { grad_body<SampleF32, R, WHICH, kKCoef, LAST ? kMsLast : kMsUp>(args); }

bool valid_call(uint32_t radius, uint32_t first, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, float data_range, const double* weights)
{
    return radius >= 1 && radius <= 4 && first <= 1 && valid_range(data_range) && scales >= 1 && scales <= kMSFMaxScales && weights != nullptr &&
           count <= msssimf_max_count(width, height);
}

} // namespace

hipError_t launch_msssimk_from(uint32_t first, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const PairFDesc* descs_dev, uint32_t count,
                               uint32_t width, uint32_t height, uint32_t scales, bool wide, float data_range, const double* weights, int cu_count,
                               int xcd_count, double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(radius, first, count, width, height, scales, data_range, weights)) return hipErrorInvalidValue;
    hipError_t e = launch_msssimf_pyramid(first, descs_dev, count, width, height, scales, stream);
    if (e != hipSuccess) return e;
    uint64_t offset = 0;
    for (uint32_t s = 0; s < scales; ++s) {
        // the cells, and with them the partials, are planf()'s; a smaller window re-plans its strips, which pay fewer warm-up rows
        const GeometryF geo = plank(radius, msf_dim(width, s), msf_dim(height, s), count, cu_count);
        const Strip2Args<PairFDesc> ka = fill_strip(geo, descs_dev + (size_t)s * count, data_range, gf, xcd_count, partials + offset);
        offset += geo.cells_per_image() * 2 * count;
        if (s < first) continue;                  // the caller's own strip kernel fills this scale's partials
        pick_radius4(radius, [&](auto r) {
            pick_bool(wide && s == 0, [&](auto w) {
                hipLaunchKernelGGL((msssimk_strip_kernel<decltype(r)::value, decltype(w)::value>), strip_grid(geo), dim3(64), 0, stream, ka);
            });
        });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_msssimf_means(count, width, height, scales, weights, partials, means, values, stream);
}

hipError_t launch_msssimk_grad_from(uint32_t first, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const PairFDesc* descs_dev,
                                    const GradFDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, float data_range,
                                    const double* weights, const double* means, const float* g_out, float* coef, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(radius, first, count, width, height, scales, data_range, weights) || which < 1 || which > 3) return hipErrorInvalidValue;
    hipError_t e = launch_msssimf_coef(count, width, height, scales, weights, means, g_out, coef, stream);
    if (e != hipSuccess) return e;
    if ((e = launch_msssimf_pyramid(first, descs_dev, count, width, height, scales, stream)) != hipSuccess) return e;
    for (uint32_t s = scales; s-- > first;) {
        const bool last = s + 1 == scales;
        Grad2Args<PairFDesc, GradFDesc> ka = fill_grad(msf_dim(width, s), msf_dim(height, s), descs_dev + (size_t)s * count, grads_dev + (size_t)s * count,
                                                       data_range, radius, gf);
        ka.up = last ? nullptr : grads_dev + (size_t)(s + 1) * count;
        ka.g_out = coef + s; ka.g_out_stride = scales;      // k_s of pair i at coef[i * scales + s]
        pick_radius4(radius, [&](auto r) {
            pick_bool(last, [&](auto l) {
                pick_which(which, [&](auto wh) {
                    hipLaunchKernelGGL((msssimk_grad_kernel<decltype(r)::value, decltype(wh)::value, decltype(l)::value>), grad_grid(ka, count), dim3(256),
                                       0, stream, ka);
                });
            });
        });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace ssim_hip
