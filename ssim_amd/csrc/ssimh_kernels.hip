// ssimh_kernels.hip -- gfx950 kernels of SSIM on float16 / bfloat16 samples and of its gradient, behind rmgr_ssim_hip_enqueue_ssimh,
// rmgr_ssim_hip_compute_ssimh_device / _host and rmgr_ssim_hip_enqueue_ssimh_grad.  The definition they implement is in
// include/rmgr/ssim-hip.h: ssimf's, applied to the samples widened to float32, with the gradient rounded once into the samples' encoding.
//
// This is the flow of ssimf_kernels.hip (DESIGN.md sections 12 to 14): the same strips, LDS ring, row and column passes, cells,
// reduction order and gradient tiles -- the bodies of ssim2_walk.h under the sample policy SampleH<TYPE>, which says how a sample gets
// into a register and how a gradient pixel leaves one; see ssim2_walk.h.
//
// Centring, per-pixel values and cells: see the top of ssim2_walk.h; the rules are the same, on the widened samples.
#include "ssim2_walk.h"

namespace ssim_hip {
namespace {

// TYPE: kSHTypeF16 or kSHTypeBF16, the encoding of the samples.
template <int TYPE, int MAP, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void ssimh_strip_kernel(const Strip2Args<PairHDesc> args) { strip_body<SampleH<TYPE>, 5, kFormSsim, MAP, WIDE>(args); }

__global__ __launch_bounds__(kStripReduceThreads)
void ssimh_reduce_kernel(const double* __restrict__ partials, uint64_t per_image, double* __restrict__ sums) { reduce_body(partials, per_image, sums); }

template <int TYPE, int WHICH>
__global__ __launch_bounds__(256)
void ssimh_grad_kernel(const Grad2Args<PairHDesc, GradHDesc> args) { grad_body<SampleH<TYPE>, 5, WHICH>(args); }

bool valid_type(int type) { return type == kSHTypeF16 || type == kSHTypeBF16; }

} // namespace

uint32_t ssimh_max_count(uint32_t width, uint32_t height) { return ssimf_max_count(width, height); }

GeometryH planh(uint32_t width, uint32_t height, uint32_t count, int cu_count) { return plan_strips(width, height, count, cu_count, 10); }

hipError_t launch_ssimh(const GeometryH& geo, const PairHDesc* descs_dev, int type, bool map, bool map_unit, bool wide, float data_range,
                        const float (&taps)[6], int xcd_count, double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    if (!valid_range(data_range) || geo.count > ssimh_max_count(geo.width, geo.height) || !valid_type(type)) return hipErrorInvalidValue;
    const Strip2Args<PairHDesc> ka = fill_strip(geo, descs_dev, data_range, taps, xcd_count, partials);
    pick_type(type, [&](auto t) {
        pick_map(map, map_unit, wide, [&](auto m, auto w) {
            hipLaunchKernelGGL((ssimh_strip_kernel<decltype(t)::value, decltype(m)::value, decltype(w)::value>), strip_grid(geo), dim3(64), 0, stream, ka);
        });
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssimh_reduce_kernel, dim3(geo.count), dim3(kStripReduceThreads), 0, stream, partials, geo.cells_per_image(), sums);
    return hipGetLastError();
}

hipError_t launch_ssimh_grad(uint32_t width, uint32_t height, uint32_t count, const PairHDesc* descs_dev, const GradHDesc* grads_dev,
                             int type, const float* g_out, float data_range, const float (&taps)[6], int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_range(data_range) || which < 1 || which > 3 || count > ssimh_max_count(width, height) || !valid_type(type)) return hipErrorInvalidValue;
    Grad2Args<PairHDesc, GradHDesc> ka = fill_grad(width, height, descs_dev, grads_dev, data_range, 5, taps);
    ka.g_out = g_out;
    pick_type(type, [&](auto t) {
        pick_which(which, [&](auto wh) {
            hipLaunchKernelGGL((ssimh_grad_kernel<decltype(t)::value, decltype(wh)::value>), grad_grid(ka, count), dim3(256), 0, stream, ka);
        });
    });
    return hipGetLastError();
}

} // namespace ssim_hip
