// ssim3h_kernels.hip -- gfx950 kernels of SSIM on float16 / bfloat16 VOLUMES (a three-dimensional window), of its gradient and of the
// gradient of its map for a per-voxel upstream gradient, behind rmgr_ssim_hip_enqueue_ssim3h, rmgr_ssim_hip_compute_ssim3h_device / _host,
// rmgr_ssim_hip_enqueue_ssim3h_grad and rmgr_ssim_hip_enqueue_ssim3h_map_grad.  The definition they implement is in
// include/rmgr/ssim-hip.h: ssim3f's, applied to the samples widened to float32, with the gradient rounded once into the samples' encoding.
//
// The walk and its adjoint are ssim3_walk.h's, instantiated here with SampleH<TYPE> at R = 5: ssim3f_kernels.hip's and
// ssim3w_kernels.hip's instantiations with another sample policy, which is what gives value, map, sums, coefficient volumes and the
// float32 gradient the bits of ssim3f on the widened volumes.  The per-volume reduction is ssim3f_kernels.hip's own kernel
// (launch_ssim3f_reduce).
//  * ssim3h_walk_kernel<TYPE, MODE>: MODE 0 (value, map, sums) and 1 / 2 / 3 (coefficient volumes, kKUniform).
//  * ssim3h_mapwalk_kernel<TYPE, MODE>: MODE 1 / 2 / 3 with k = gMap(p) read per voxel (kKPerVoxel).
//  * ssim3h_adjoint_kernel<TYPE, WHICH>.
// The launches take the six taps of any 11-tap window (the _win entries: another sigma, or the box); NULL is the engine's window.  Windows
// of 3, 5, 7 and 9 taps have kernels of their own radius in ssim3hk_kernels.hip.
#include "ssim3h_kernels.h"
#include "ssim3_walk.h"

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleH<kSHTypeF16>> K3HArgs;      // the same struct for both encodings

template <int TYPE, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3h_walk_kernel(const K3HArgs args)
{
    walk_body<SampleH<TYPE>, 5, MODE, kKUniform>(args);
}

template <int TYPE, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3h_mapwalk_kernel(const K3HArgs args)
{
    static_assert(MODE >= 1 && MODE <= 3, "the value walk has no upstream gradient");
    walk_body<SampleH<TYPE>, 5, MODE, kKPerVoxel>(args);
}

template <int TYPE, int WHICH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3h_adjoint_kernel(const K3HArgs args)
{
    adjoint_body<SampleH<TYPE>, 5, WHICH>(args);
}

static_assert(kSHTypeF16 == 0 && kSHTypeBF16 == 1, "the dispatch on the encoding");

// MODE 1 / 2 / 3: the coefficient walk of the upstream form the arguments carry (gouts: per voxel).
hipError_t launch_walk(const K3HArgs& ka, int type, int mode, const Geometry3F& geo, hipStream_t stream)
{
    return with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<0, 3>(mode, [&](auto MODE) {
        if constexpr (MODE() != 0) {
            if (ka.gouts) {
                hipLaunchKernelGGL((ssim3h_mapwalk_kernel<TYPE(), MODE()>), grid_of(geo), dim3(256), 0, stream, ka);
                return true;
            }
        }
        hipLaunchKernelGGL((ssim3h_walk_kernel<TYPE(), MODE()>), grid_of(geo), dim3(256), 0, stream, ka);
        return true; }); }) ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_adjoint(const K3HArgs& ka, int type, int which, const Geometry3F& geo, hipStream_t stream)
{
    return with_constant<0, 1>(type, [&](auto TYPE) { return with_constant<1, 3>(which, [&](auto WHICH) {
        hipLaunchKernelGGL((ssim3h_adjoint_kernel<TYPE(), WHICH()>), grid_of(geo), dim3(256), 0, stream, ka);
        return true; }); }) ? hipGetLastError() : hipErrorInvalidValue;
}

} // namespace

hipError_t launch_ssim3h(const Geometry3F& geo, const Pair3HDesc* descs_dev, int type, float data_range, double* partials, double* sums,
                         hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3HArgs ka;
    if (!fill_args(ka, geo, data_range, 5, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.partials = partials;
    const hipError_t e = launch_walk(ka, type, 0, geo, stream);
    if (e != hipSuccess) return e;
    return launch_ssim3f_reduce(geo, partials, sums, stream);
}

hipError_t launch_ssim3h_grad(const Geometry3F& geo, const Pair3HDesc* descs_dev, const Grad3HDesc* grads_dev, int type, const float* g_out,
                              float data_range, int which, float* coef, hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3HArgs ka;
    if (which < 1 || which > 3 || g_out == NULL || !fill_args(ka, geo, data_range, 5, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.coef = coef;
    const hipError_t e = launch_walk(ka, type, which, geo, stream);
    if (e != hipSuccess) return e;
    return launch_adjoint(ka, type, which, geo, stream);
}

hipError_t launch_ssim3h_map_grad(const Geometry3F& geo, const Pair3HDesc* descs_dev, const Grad3HDesc* grads_dev, const GradOut3FDesc* gouts_dev,
                                  int type, float data_range, int which, float* coef, hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3HArgs ka;
    if (which < 1 || which > 3 || gouts_dev == NULL || !fill_args(ka, geo, data_range, 5, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.gouts = gouts_dev; ka.coef = coef;
    const hipError_t e = launch_walk(ka, type, which, geo, stream);
    if (e != hipSuccess) return e;
    return launch_adjoint(ka, type, which, geo, stream);
}

} // namespace ssim_hip
