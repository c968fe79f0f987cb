// ssim3hk_kernels.hip -- gfx950 kernels of SSIM on float16 / bfloat16 VOLUMES under a window of 3, 5, 7 or 9 taps per axis (radius R = 1
// .. 4) and of its gradient for both upstream forms, behind the rmgr_ssim_hip_*_ssim3h_win* entries.  The definition is in
// include/rmgr/ssim-hip.h: ssim3f_win's, applied to the samples widened to float32, with the gradient rounded once into the samples'
// encoding.  Windows of 11 taps run on the kernels of ssim3h_kernels.hip with the window's taps.
//
// The walk and its adjoint are ssim3_walk.h's, instantiated here with SampleH<TYPE> at R = 1 .. 4; the weight k of the coefficient
// walk is kKEither, a branch on a kernel argument that serves both upstream forms.  These are ssim3k_kernels.hip's instantiations
// with another sample policy, which is what gives value, map, sums, coefficient volumes and the float32 gradient the bits of ssim3k on
// the widened volumes.  The per-volume reduction is ssim3f_kernels.hip's own kernel (launch_ssim3f_reduce).
#include "ssim3hk_kernels.h"
#include "ssim3_walk.h"

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleH<kSHTypeF16>> K3HKArgs;      // the same struct for both encodings

template <int TYPE, int R, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3hk_walk_kernel(const K3HKArgs args)
{
    walk_body<SampleH<TYPE>, R, MODE, kKEither>(args);
}

template <int TYPE, int R, int WHICH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3hk_adjoint_kernel(const K3HKArgs args)
{
    adjoint_body<SampleH<TYPE>, R, WHICH>(args);
}

static_assert(kSHTypeF16 == 0 && kSHTypeBF16 == 1, "the dispatch on the encoding");

hipError_t launch_walk(const K3HKArgs& ka, int type, uint32_t radius, int mode, const Geometry3F& geo, hipStream_t stream)
{
    return with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 4>(radius, [&](auto R) { return with_constant<0, 3>(mode, [&](auto MODE) {
        hipLaunchKernelGGL((ssim3hk_walk_kernel<TYPE(), R(), MODE()>), grid_of(geo), dim3(256), 0, stream, ka);
        return true; }); }); }) ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_adjoint(const K3HKArgs& ka, int type, uint32_t radius, int which, const Geometry3F& geo, hipStream_t stream)
{
    return with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 4>(radius, [&](auto R) { return with_constant<1, 3>(which, [&](auto WHICH) {
        hipLaunchKernelGGL((ssim3hk_adjoint_kernel<TYPE(), R(), WHICH()>), grid_of(geo), dim3(256), 0, stream, ka);
        return true; }); }); }) ? hipGetLastError() : hipErrorInvalidValue;
}

} // namespace

hipError_t launch_ssim3hk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3HDesc* descs_dev, int type,
                          float data_range, double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3HKArgs ka;
    if (!fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.partials = partials;
    const hipError_t e = launch_walk(ka, type, radius, 0, geo, stream);
    if (e != hipSuccess) return e;
    return launch_ssim3f_reduce(geo, partials, sums, stream);
}

hipError_t launch_ssim3hk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3HDesc* descs_dev,
                               const Grad3HDesc* grads_dev, int type, const float* g_out, const GradOut3FDesc* gouts_dev, float data_range,
                               int which, float* coef, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    K3HKArgs ka;
    if (which < 1 || which > 3 || (g_out == NULL) == (gouts_dev == NULL) || !fill_args(ka, geo, data_range, radius, gf)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.gouts = gouts_dev; ka.coef = coef;
    const hipError_t e = launch_walk(ka, type, radius, which, geo, stream);
    if (e != hipSuccess) return e;
    return launch_adjoint(ka, type, radius, which, geo, stream);
}

} // namespace ssim_hip
