// ssimf_kernels.hip -- gfx950 kernels of SSIM on float32 samples and of its gradient, behind rmgr_ssim_hip_enqueue_ssimf,
// rmgr_ssim_hip_compute_ssimf_device / _host and rmgr_ssim_hip_enqueue_ssimf_grad.  The definition they implement is in
// include/rmgr/ssim-hip.h; tests/ssimf_model.py restates it in float64 and restates the arithmetic in fp32.
//
// Kept apart from ssim_kernels.hip on purpose: that file's sha256 is the kernel source id measurements are tied to
// (Makefile, profiles/traffic.json).  The strip walk, the reduction and the gradient tile are those of ssim2_walk.h, whose top has the
// arithmetic contract (centring, per-pixel order, cells); see ssim2_walk.h.  This file holds the instantiations for float32 samples
// under the 11-tap window (radius 5), the constants rule, the planner and the launch bound of the family.
//
//  * ssimf_strip_kernel<MAP, WIDE>: strip_body, the SSIM form.
//  * ssimf_reduce_kernel: each image's cell partials summed in a fixed order.
//  * ssimf_grad_kernel<WHICH>: grad_body with the launch-uniform k.
#include "ssim2_walk.h"

namespace ssim_hip {
namespace {

template <int MAP, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void ssimf_strip_kernel(const Strip2Args<PairFDesc> args) { strip_body<SampleF32, 5, kFormSsim, MAP, WIDE>(args); }

__global__ __launch_bounds__(kStripReduceThreads)
void ssimf_reduce_kernel(const double* __restrict__ partials, uint64_t per_image, double* __restrict__ sums) { reduce_body(partials, per_image, sums); }

template <int WHICH>
__global__ __launch_bounds__(256)
void ssimf_grad_kernel(const Grad2Args<PairFDesc, GradFDesc> args) { grad_body<SampleF32, 5, WHICH>(args); }

} // namespace

void ssimf_constants(float data_range, float& c1, float& c2)
{
    const double R = (double)data_range;
    c1 = (float)((0.01 * R) * (0.01 * R));
    c2 = (float)((0.03 * R) * (0.03 * R));
}

uint32_t ssimf_max_count(uint32_t width, uint32_t height)
{
    if (width == 0 || height == 0 || width > kSFMaxDim || height > kSFMaxDim) return 0;
    // the worst case: strips of the smallest height
    const uint64_t cr = cell_rows_of(height);
    const uint64_t per = (uint64_t)((width + kSFStripW - 1) / kSFStripW) * ((height + cr - 1) / cr);
    const uint64_t tiles = (uint64_t)((width + kSFTile - 1) / kSFTile) * ((height + kSFTile - 1) / kSFTile);
    return (uint32_t)std::min<uint64_t>(std::min(kMaxBlocks / per, kMaxGradBlocks / tiles), 65535);
}

GeometryF planf(uint32_t width, uint32_t height, uint32_t count, int cu_count) { return plan_strips(width, height, count, cu_count, 10); }

hipError_t launch_ssimf(const GeometryF& geo, const PairFDesc* descs_dev, bool map, bool map_unit, bool wide, float data_range,
                        const float (&taps)[6], int xcd_count, double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    if (!valid_range(data_range) || geo.count > ssimf_max_count(geo.width, geo.height)) return hipErrorInvalidValue;
    const Strip2Args<PairFDesc> ka = fill_strip(geo, descs_dev, data_range, taps, xcd_count, partials);
    pick_map(map, map_unit, wide, [&](auto m, auto w) {
        hipLaunchKernelGGL((ssimf_strip_kernel<decltype(m)::value, decltype(w)::value>), strip_grid(geo), dim3(64), 0, stream, ka);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssimf_reduce_kernel, dim3(geo.count), dim3(kStripReduceThreads), 0, stream, partials, geo.cells_per_image(), sums);
    return hipGetLastError();
}

hipError_t launch_ssimf_grad(uint32_t width, uint32_t height, uint32_t count, const PairFDesc* descs_dev, const GradFDesc* grads_dev,
                             const float* g_out, float data_range, const float (&taps)[6], int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_range(data_range) || which < 1 || which > 3 || count > ssimf_max_count(width, height)) return hipErrorInvalidValue;
    Grad2Args<PairFDesc, GradFDesc> ka = fill_grad(width, height, descs_dev, grads_dev, data_range, 5, taps);
    ka.g_out = g_out;
    pick_which(which, [&](auto wh) { hipLaunchKernelGGL((ssimf_grad_kernel<decltype(wh)::value>), grad_grid(ka, count), dim3(256), 0, stream, ka); });
    return hipGetLastError();
}

} // namespace ssim_hip
