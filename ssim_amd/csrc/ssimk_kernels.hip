// ssimk_kernels.hip -- gfx950 kernels of SSIM on float32 samples, and of its gradient, under a window of 3, 5, 7 or 9 taps (radius
// R = 1 .. 4), behind rmgr_ssim_hip_enqueue_ssimf_win, rmgr_ssim_hip_compute_ssimf_win_device / _host, rmgr_ssim_hip_enqueue_ssimf_win_grad
// and rmgr_ssim_hip_enqueue_ssimf_win_map_grad.  The definition they implement is in include/rmgr/ssim-hip.h (rmgr_ssim_hip_Window);
// tests/ssimk_model.py restates it in float64 and restates the arithmetic in fp32.  Windows of 11 taps run on ssimf_kernels.hip and
// ssimw_kernels.hip with the window's taps; this file also holds the taps rule of every window (window_taps).
//
// This is the flow of ssimf_kernels.hip at another radius: the bodies of ssim2_walk.h with R = 1 .. 4; see ssim2_walk.h for what the
// radius changes (rings, warm-up rows, the LDS slot, the gradient's planes and weights).
//  * ssimk_strip_kernel<R, MAP, WIDE>: MAP 0 no map; 1 a map of any ssimStep (one 4-byte store per column).
//  * ssimk_grad_kernel<R, WHICH>: one kernel serves both upstream forms (kKEither): k = float(double(gOut) / (double(W) double(H))) for
//    the whole launch, or k(p) = gMap(p) read per pixel -- a branch on a kernel argument.
//  * ssimk_reduce_kernel: each image's cell partials summed in a fixed order.
// Centring, cells, tiles and summation orders: see the top of ssim2_walk.h; they are position-based and do not depend on the radius.
#include "ssim2_walk.h"

namespace ssim_hip {
namespace {

template <int R, int MAP, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void ssimk_strip_kernel(const Strip2Args<PairFDesc> args) { strip_body<SampleF32, R, kFormSsim, MAP, WIDE>(args); }

__global__ __launch_bounds__(kStripReduceThreads)
void ssimk_reduce_kernel(const double* __restrict__ partials, uint64_t per_image, double* __restrict__ sums) { reduce_body(partials, per_image, sums); }

template <int R, int WHICH>
__global__ __launch_bounds__(256)
void ssimk_grad_kernel(const Grad2Args<PairFDesc, GradFDesc> args) { grad_body<SampleF32, R, WHICH, kKEither>(args); }

} // namespace

bool window_taps(uint32_t radius, uint32_t kind, float sigma, float (&gf)[kSKMaxRadius + 1])
{
    if (radius < 1 || radius > kSKMaxRadius) return false;
    for (int i = 0; i <= kSKMaxRadius; ++i) gf[i] = 0.0f;
    if (kind == kSKUniform) {
        for (uint32_t i = 0; i <= radius; ++i) gf[i] = (float)(1.0 / (double)(2 * radius + 1));
        return true;
    }
    if (kind != kSKGaussian || !(sigma > 0.0f) || !std::isfinite(sigma)) return false;
    const double s = (double)sigma;
    double g[kSKMaxRadius + 1], norm = 0.0;
    for (int i = 0; i <= (int)radius; ++i) {
        g[i] = exp(-(double)(i * i) / (2.0 * s * s));
        norm += (i == 0) ? g[i] : 2.0 * g[i];
    }
    for (int i = 0; i <= (int)radius; ++i) gf[i] = (float)(g[i] / norm);
    return true;
}

void window_tails(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], float (&tail)[kSKMaxRadius + 1], float& total)
{
    for (int i = 0; i <= kSKMaxRadius; ++i) tail[i] = 0.0f;
    double t = 0.0;
    for (int i = (int)radius; i >= 0; --i) { t += (double)gf[i]; tail[i] = (float)t; }
    total = (float)(2.0 * t - (double)gf[0]);
}

GeometryF plank(uint32_t radius, uint32_t width, uint32_t height, uint32_t count, int cu_count)
{
    return plan_strips(width, height, count, cu_count, 2 * radius);
}

hipError_t launch_ssimk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const GeometryF& geo, const PairFDesc* descs_dev, bool map, bool wide,
                        float data_range, int xcd_count, double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    if (radius < 1 || radius > 4 || !valid_range(data_range) || geo.count > ssimf_max_count(geo.width, geo.height)) return hipErrorInvalidValue;
    const Strip2Args<PairFDesc> ka = fill_strip(geo, descs_dev, data_range, gf, xcd_count, partials);
    pick_radius4(radius, [&](auto r) {
        pick_bool(map, [&](auto m) {
            pick_bool(wide, [&](auto w) {
                hipLaunchKernelGGL((ssimk_strip_kernel<decltype(r)::value, decltype(m)::value ? 1 : 0, decltype(w)::value>), strip_grid(geo), dim3(64), 0, stream, ka);
            });
        });
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssimk_reduce_kernel, dim3(geo.count), dim3(kStripReduceThreads), 0, stream, partials, geo.cells_per_image(), sums);
    return hipGetLastError();
}

hipError_t launch_ssimk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], uint32_t width, uint32_t height, uint32_t count,
                             const PairFDesc* descs_dev, const GradFDesc* grads_dev, const float* g_out, const GradOutFDesc* gouts_dev,
                             float data_range, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (radius < 1 || radius > 4 || !valid_range(data_range) || which < 1 || which > 3 ||
        (g_out == NULL) == (gouts_dev == NULL) || count > ssimf_max_count(width, height))
        return hipErrorInvalidValue;
    Grad2Args<PairFDesc, GradFDesc> ka = fill_grad(width, height, descs_dev, grads_dev, data_range, radius, gf);
    ka.g_out = g_out; ka.gouts = g_out ? NULL : gouts_dev;
    pick_radius4(radius, [&](auto r) {
        pick_which(which, [&](auto wh) {
            hipLaunchKernelGGL((ssimk_grad_kernel<decltype(r)::value, decltype(wh)::value>), grad_grid(ka, count), dim3(256), 0, stream, ka);
        });
    });
    return hipGetLastError();
}

} // namespace ssim_hip
