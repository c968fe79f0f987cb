// msssimh_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, multi-scale SSIM of float16 / bfloat16 samples and its
// gradient) and the kernels (msssimh_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssimh, rmgr_ssim_hip_enqueue_msssimh_grad).
//
// Only scale 0 holds 16-bit samples: its strip kernel, its pyramid step and its gradient kernel are msssimh_kernels.hip's; scales >= 1,
// the reduction, the product and the coefficients are the float32 kernels of msssimf_kernels.hip, run by launch_msssimf_from /
// launch_msssimf_grad_from over the same partials, pyramid and coarse gradient planes.
#ifndef SSIM_AMD_MSSSIMH_KERNELS_H
#define SSIM_AMD_MSSSIMH_KERNELS_H

#include "msssimf_kernels.h"    // PairFDesc, GradFDesc, msf_*, launch_msssimf_from, launch_msssimf_grad_from
#include "ssimh_kernels.h"      // PairHDesc, GradHDesc, kSHType*, fitsh_narrow

namespace ssim_hip {

// Enqueues the forward of `count` pairs on `stream`: the pyramid step from the 16-bit scale 0 to the float32 scale 1, the strip kernel
// of scale 0, then launch_msssimf_from(1, ...): the rest of the pyramid, the strip kernels of scales >= 1, the reduction and the product.
//   descs0_dev   count PairHDesc in device memory: the caller's planes (map ignored)
//   descs_dev    scales x count PairFDesc in device memory, [scale][pair]: rows >= 1 dense scratch planes that this call writes; row 0
//                is not read
//   type         kSHTypeF16 or kSHTypeBF16
//   wide         some pair fails fitsh_narrow()
//   radius, taps the window, the same at every scale, as launch_msssimf_from takes it: the radius must be 5 (windows of 11 taps run on these
//                kernels with the window's taps); radius 1 .. 4: launch_msssimhk / launch_msssimhk_grad of msssimk_kernels.h
//   the rest     as launch_msssimf
hipError_t launch_msssimh(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                          uint32_t scales, int type, bool wide, float data_range, uint32_t radius, const float (&taps)[kSKMaxRadius + 1],
                          const double* weights, int cu_count, int xcd_count, double* partials, double* means, double* values, hipStream_t stream);

// Enqueues the gradient of `count` pairs on `stream`: the pyramid step from scale 0 to scale 1, launch_msssimf_grad_from(1, ...) -- the
// coefficients, the rest of the pyramid, the float32 gradient kernels from the coarsest scale down to scale 1 --, then the gradient
// kernel of scale 0, which rounds each pixel once, to nearest-even, into the samples' encoding.
//   descs0_dev, descs_dev   as above
//   grads0_dev   count GradHDesc in device memory: the caller's gradient planes
//   grads_dev    scales x count GradFDesc in device memory, [scale][pair]: rows >= 1 dense float32 scratch planes; row 0 is not read
//   radius, taps as above
//   the rest     as launch_msssimf_grad
hipError_t launch_msssimh_grad(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, const GradHDesc* grads0_dev, const GradFDesc* grads_dev,
                               uint32_t count, uint32_t width, uint32_t height, uint32_t scales, int type, float data_range, uint32_t radius,
                               const float (&taps)[kSKMaxRadius + 1], const double* weights, const double* means, const float* g_out, float* coef,
                               int which, hipStream_t stream);

// The pyramid step from the 16-bit scale 0 into row 1 of descs_dev, as the two launchers above enqueue it -- for them and for
// msssimhk_kernels.hip; it does not depend on the window.
hipError_t launch_msssimh_down(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, int type,
                               hipStream_t stream);

} // namespace ssim_hip

#endif
