// ssimhk_kernels.hip -- gfx950 kernels of SSIM on float16 / bfloat16 samples, and of its gradient, under a window of 3, 5, 7 or 9 taps
// (radius R = 1 .. 4), behind rmgr_ssim_hip_enqueue_ssimh_win, rmgr_ssim_hip_compute_ssimh_win_device / _host,
// rmgr_ssim_hip_enqueue_ssimh_win_grad and rmgr_ssim_hip_enqueue_ssimh_win_map_grad.  The definition they implement is in
// include/rmgr/ssim-hip.h: ssimf_win's, applied to the samples widened to float32, with the gradient rounded once into the samples'
// encoding.  Windows of 11 taps run on ssimh_kernels.hip and ssimw_kernels.hip with the window's taps; the taps of every window are
// ssimk_kernels.hip's (window_taps), the strips are planned by its plank.
//
// This is the flow of ssimk_kernels.hip under the sample policy of ssimh_kernels.hip: the bodies of ssim2_walk.h with R = 1 .. 4 and
// SampleH<TYPE>.  Both template axes are those files'; no line of a body is written here.  Those files' kernels are counted by their
// tests, hence a file of its own.
//  * ssimhk_strip_kernel<TYPE, R, MAP, WIDE>: MAP 0 no map; 1 a map of any ssimStep (one 4-byte store per column).
//  * ssimhk_grad_kernel<TYPE, R, WHICH>: one kernel serves both upstream forms (kKEither): k = float(double(gOut) / (double(W) double(H)))
//    for the whole launch, or k(p) = gMap(p) read per pixel -- a branch on a kernel argument.
//  * ssimhk_reduce_kernel: each image's cell partials summed in a fixed order.
// Centring, cells, tiles and summation orders: see the top of ssim2_walk.h; they are position-based and depend neither on the radius
// nor on the encoding.
#include "ssim2_walk.h"
#include "ssimhk_kernels.h"

namespace ssim_hip {
namespace {

// TYPE: kSHTypeF16 or kSHTypeBF16, the encoding of the samples.
template <int TYPE, int R, int MAP, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void ssimhk_strip_kernel(const Strip2Args<PairHDesc> args) { strip_body<SampleH<TYPE>, R, kFormSsim, MAP, WIDE>(args); }

__global__ __launch_bounds__(kStripReduceThreads)
void ssimhk_reduce_kernel(const double* __restrict__ partials, uint64_t per_image, double* __restrict__ sums) { reduce_body(partials, per_image, sums); }

template <int TYPE, int R, int WHICH>
__global__ __launch_bounds__(256)
void ssimhk_grad_kernel(const Grad2Args<PairHDesc, GradHDesc> args) { grad_body<SampleH<TYPE>, R, WHICH, kKEither>(args); }

bool valid_type(int type) { return type == kSHTypeF16 || type == kSHTypeBF16; }

} // namespace

hipError_t launch_ssimhk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const GeometryH& geo, const PairHDesc* descs_dev, int type, bool map,
                         bool wide, float data_range, int xcd_count, double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    if (radius < 1 || radius > 4 || !valid_range(data_range) || geo.count > ssimh_max_count(geo.width, geo.height) || !valid_type(type))
        return hipErrorInvalidValue;
    const Strip2Args<PairHDesc> ka = fill_strip(geo, descs_dev, data_range, gf, xcd_count, partials);
    pick_type(type, [&](auto t) {
        pick_radius4(radius, [&](auto r) {
            pick_bool(map, [&](auto m) {
                pick_bool(wide, [&](auto w) {
                    hipLaunchKernelGGL((ssimhk_strip_kernel<decltype(t)::value, decltype(r)::value, decltype(m)::value ? 1 : 0, decltype(w)::value>),
                                       strip_grid(geo), dim3(64), 0, stream, ka);
                });
            });
        });
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssimhk_reduce_kernel, dim3(geo.count), dim3(kStripReduceThreads), 0, stream, partials, geo.cells_per_image(), sums);
    return hipGetLastError();
}

hipError_t launch_ssimhk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], uint32_t width, uint32_t height, uint32_t count,
                              const PairHDesc* descs_dev, const GradHDesc* grads_dev, int type, const float* g_out, const GradOutFDesc* gouts_dev,
                              float data_range, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (radius < 1 || radius > 4 || !valid_range(data_range) || which < 1 || which > 3 || !valid_type(type) ||
        (g_out == NULL) == (gouts_dev == NULL) || count > ssimh_max_count(width, height))
        return hipErrorInvalidValue;
    Grad2Args<PairHDesc, GradHDesc> ka = fill_grad(width, height, descs_dev, grads_dev, data_range, radius, gf);
    ka.g_out = g_out; ka.gouts = g_out ? NULL : gouts_dev;
    pick_type(type, [&](auto t) {
        pick_radius4(radius, [&](auto r) {
            pick_which(which, [&](auto wh) {
                hipLaunchKernelGGL((ssimhk_grad_kernel<decltype(t)::value, decltype(r)::value, decltype(wh)::value>), grad_grid(ka, count), dim3(256), 0,
                                   stream, ka);
            });
        });
    });
    return hipGetLastError();
}

} // namespace ssim_hip
