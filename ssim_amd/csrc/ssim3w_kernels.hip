// ssim3w_kernels.hip -- gfx950 kernels of the gradient of the 3-D SSIM MAP for a per-voxel upstream gradient, behind
// rmgr_ssim_hip_enqueue_ssim3f_map_grad.  The definition is in include/rmgr/ssim-hip.h; tests/ssim3w_model.py restates it in float64 and
// restates the arithmetic in fp32.
//
// ssim3w_walk_kernel<MODE> is ssim3_walk.h's walk with SampleF32 at R = 5, as ssim3f_walk_kernel<MODE> of MODE 1 / 2 / 3 (the
// coefficient volumes of dLoss/dA, dLoss/dB, both) is, with ONE change: the weight k of the voxel's partial derivatives is not the
// launch-uniform float(gOut / (W H D)) but gMap(p), read per voxel through the pair's GradOut3FDesc (kKPerVoxel).  The second walk is
// ssim3f_kernels.hip's adjoint kernel itself (launch_ssim3f_adjoint): a volume gMap of the constant float(gOut / (W H D)) leaves the bits
// of launch_ssim3f_grad.
#include "ssim3w_kernels.h"
#include "ssim3_walk.h"

namespace ssim_hip {
namespace {

typedef ArgsOf<SampleF32> K3WArgs;

template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void ssim3w_walk_kernel(const K3WArgs args)
{
    static_assert(MODE >= 1 && MODE <= 3, "the value walk stays in ssim3f_kernels.hip");
    walk_body<SampleF32, 5, MODE, kKPerVoxel>(args);
}

} // namespace

hipError_t launch_ssim3w_grad(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, const GradOut3FDesc* gouts_dev,
                              float data_range, int which, float* coef, hipStream_t stream, const float* taps)
{
    if (geo.count == 0) return hipSuccess;
    K3WArgs ka;
    if (!fill_args(ka, geo, data_range, 5, taps)) return hipErrorInvalidValue;
    ka.descs = descs_dev; ka.gouts = gouts_dev; ka.coef = coef;
    if (!with_constant<1, 3>(which, [&](auto MODE) {
            hipLaunchKernelGGL((ssim3w_walk_kernel<MODE()>), grid_of(geo), dim3(256), 0, stream, ka);
            return true; }))
        return hipErrorInvalidValue;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ssim3f_adjoint(geo, descs_dev, grads_dev, data_range, which, coef, stream, taps);
}

} // namespace ssim_hip
