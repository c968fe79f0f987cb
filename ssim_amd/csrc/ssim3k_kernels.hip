// ssim3k_kernels.hip -- gfx950 kernels of SSIM on float32 VOLUMES under a window of 3, 5, 7 or 9 taps per axis (radius R = 1 .. 4) and of
// its gradient for both upstream forms, behind the rmgr_ssim_hip_*_ssim3f_win* entries.  The definition is in include/rmgr/ssim-hip.h;
// tests/ssim3k_model.py restates it in float64 and restates the arithmetic in fp32.  Windows of 11 taps run on the kernels of
// ssim3f_kernels.hip / ssim3w_kernels.hip with the window's taps.
//
// The walk and its adjoint are ssim3_walk.h's, instantiated here with SampleF32 at R = 1 .. 4; the weight k of the coefficient walk is
// kKEither, a branch on a kernel argument that serves both upstream forms.  The per-volume reduction is ssim3f_kernels.hip's
// (launch_ssim3f_reduce): the cells do not depend on the radius.
#include "ssim3k_kernels.h"
#include "ssim3_walk.h"

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleF32> K3KArgs;

template <int R, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3k_walk_kernel(const K3KArgs args)
{
    walk_body<SampleF32, R, MODE, kKEither>(args);
}

template <int R, int WHICH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3k_adjoint_kernel(const K3KArgs args)
{
    adjoint_body<SampleF32, R, WHICH>(args);
}

hipError_t launch_walk(const K3KArgs& ka, uint32_t radius, int mode, const Geometry3F& geo, hipStream_t stream)
{
    return with_constant<1, 4>(radius, [&](auto R) { return with_constant<0, 3>(mode, [&](auto MODE) {
        hipLaunchKernelGGL((ssim3k_walk_kernel<R(), MODE()>), grid_of(geo), dim3(256), 0, stream, ka);
        return true; }); }) ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_adjoint(const K3KArgs& ka, uint32_t radius, int which, const Geometry3F& geo, hipStream_t stream)
{
    return with_constant<1, 4>(radius, [&](auto R) { return with_constant<1, 3>(which, [&](auto WHICH) {
        hipLaunchKernelGGL((ssim3k_adjoint_kernel<R(), WHICH()>), grid_of(geo), dim3(256), 0, stream, ka);
        return true; }); }) ? hipGetLastError() : hipErrorInvalidValue;
}

} // namespace

hipError_t launch_ssim3k(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3FDesc* descs_dev, float data_range,
                         double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3KArgs ka;
    if (!fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.partials = partials;
    const hipError_t e = launch_walk(ka, radius, 0, geo, stream);
    if (e != hipSuccess) return e;
    return launch_ssim3f_reduce(geo, partials, sums, stream);
}

hipError_t launch_ssim3k_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3FDesc* descs_dev,
                              const Grad3FDesc* grads_dev, const float* g_out, const GradOut3FDesc* gouts_dev, float data_range, int which,
                              float* coef, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3KArgs ka;
    if (which < 1 || which > 3 || (g_out == NULL) == (gouts_dev == NULL) || !fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.gouts = gouts_dev; ka.coef = coef;
    const hipError_t e = launch_walk(ka, radius, which, geo, stream);
    if (e != hipSuccess) return e;
    return launch_adjoint(ka, radius, which, geo, stream);
}

} // namespace ssim_hip
