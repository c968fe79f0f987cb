// ssimw_kernels.hip -- gfx950 kernels of the gradient of the SSIM MAP, for an upstream gradient given per pixel, behind
// rmgr_ssim_hip_enqueue_ssimf_map_grad (float32 samples) and rmgr_ssim_hip_enqueue_ssimh_map_grad (float16 / bfloat16 samples).  The
// definition they implement is in include/rmgr/ssim-hip.h; tests/ssimw_model.py restates it in float64 and restates the arithmetic
// in fp32.
//
// This is the gradient tile of ssimf_kernels.hip and ssimh_kernels.hip -- grad_body of ssim2_walk.h -- in its per-pixel form
// (kKPerPixel): in step 3 the factor k that multiplies the partials is not the launch-uniform gOut / (W H) but the pixel's own gMap(p),
// read through the plane's descriptor.  Every other instruction is the same, so a plane whose every element is float(gOut / (W H))
// gives the bits of ssimf_grad_kernel / ssimh_grad_kernel.  Those files' kernels are counted by their tests, hence a file of its own.
//
// Centring, tiles, summation orders: see the top of ssim2_walk.h and the comment above grad_body.
#include "ssim2_walk.h"

namespace ssim_hip {
namespace {

// TYPE: the samples' (and the gradient planes') encoding.
enum { kSWTypeF32 = 0, kSWTypeF16 = 1, kSWTypeBF16 = 2 };

template <int TYPE> struct Sample       { typedef SampleH<TYPE == kSWTypeBF16 ? kSHTypeBF16 : kSHTypeF16> S; };
template <> struct Sample<kSWTypeF32>   { typedef SampleF32 S; };

template <int TYPE> using KWArgs = Grad2Args<typename Sample<TYPE>::S::Pair, typename Sample<TYPE>::S::Grad>;

template <int TYPE, int WHICH>
__global__ __launch_bounds__(256)
void ssimw_grad_kernel(const KWArgs<TYPE> args) { grad_body<typename Sample<TYPE>::S, 5, WHICH, kKPerPixel>(args); }

template <int TYPE>
hipError_t launch(uint32_t width, uint32_t height, uint32_t count, const typename Sample<TYPE>::S::Pair* descs_dev,
                  const typename Sample<TYPE>::S::Grad* grads_dev, const GradOutFDesc* gouts_dev, float data_range, const float (&taps)[6], int which,
                  hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_range(data_range) || which < 1 || which > 3 || count > ssimf_max_count(width, height)) return hipErrorInvalidValue;
    KWArgs<TYPE> ka = fill_grad(width, height, descs_dev, grads_dev, data_range, 5, taps);
    ka.gouts = gouts_dev;
    pick_which(which, [&](auto wh) { hipLaunchKernelGGL((ssimw_grad_kernel<TYPE, decltype(wh)::value>), grad_grid(ka, count), dim3(256), 0, stream, ka); });
    return hipGetLastError();
}

} // namespace

hipError_t launch_ssimw_grad_f(uint32_t width, uint32_t height, uint32_t count, const PairFDesc* descs_dev, const GradFDesc* grads_dev,
                               const GradOutFDesc* gouts_dev, float data_range, const float (&taps)[6], int which, hipStream_t stream)
{
    return launch<kSWTypeF32>(width, height, count, descs_dev, grads_dev, gouts_dev, data_range, taps, which, stream);
}

hipError_t launch_ssimw_grad_h(uint32_t width, uint32_t height, uint32_t count, const PairHDesc* descs_dev, const GradHDesc* grads_dev,
                               int type, const GradOutFDesc* gouts_dev, float data_range, const float (&taps)[6], int which, hipStream_t stream)
{
    if (type == kSHTypeBF16) return launch<kSWTypeBF16>(width, height, count, descs_dev, grads_dev, gouts_dev, data_range, taps, which, stream);
    if (type == kSHTypeF16)  return launch<kSWTypeF16>(width, height, count, descs_dev, grads_dev, gouts_dev, data_range, taps, which, stream);
    return hipErrorInvalidValue;
}

} // namespace ssim_hip
