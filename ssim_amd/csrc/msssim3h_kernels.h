// msssim3h_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, multi-scale SSIM of float16 / bfloat16 VOLUMES and its
// gradient) and the kernels (msssim3h_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssim3h, rmgr_ssim_hip_enqueue_msssim3h_grad).
//
// Only scale 0 holds 16-bit samples: its walks, its pyramid step and its adjoint are msssim3h_kernels.hip's; scales >= 1, the reduction,
// the product and the coefficients k_s are the float32 kernels of msssim3f_kernels.hip, run by launch_msssim3f_from /
// launch_msssim3f_grad_from over the same partials, pyramid and coarse gradient volumes.
#ifndef SSIM_AMD_MSSSIM3H_KERNELS_H
#define SSIM_AMD_MSSSIM3H_KERNELS_H

#include "msssim3f_kernels.h"   // Pair3FDesc, Grad3FDesc, ms3_*, launch_msssim3f_from, launch_msssim3f_grad_from
#include "ssim3h_kernels.h"     // Pair3HDesc, Grad3HDesc, kSHType*

namespace ssim_hip {

// Enqueues the forward of `count` pairs on `stream`: the pyramid step from the 16-bit scale 0 to the float32 scale 1, the value walk of
// scale 0, then launch_msssim3f_from(1, ...): the rest of the pyramid, the walks of scales >= 1, the reduction and the product.
//   descs0_dev   count Pair3HDesc in device memory: the caller's volumes; map must be NULL
//   descs_dev    scales x count Pair3FDesc in device memory, [scale][pair]: rows >= 1 dense scratch volumes that this call writes; row 0
//                is not read
//   type         kSHTypeF16 or kSHTypeBF16
//   radius, taps the window, the same at every scale, as launch_msssim3f_from takes it: the radius must be 5 (windows of 11 taps run on these
//                kernels with the window's taps; NULL: the engine's); radius 1 .. 4: launch_msssim3hk / launch_msssim3hk_grad of
//                msssim3k_kernels.h
//   the rest     as launch_msssim3f
hipError_t launch_msssim3h(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                           uint32_t depth, uint32_t scales, int type, float data_range, uint32_t radius, const float* taps, const double* weights,
                           int cu_count, double* partials, double* means, double* values, hipStream_t stream);

// Enqueues the gradient of `count` pairs on `stream`: the pyramid step from scale 0 to scale 1, launch_msssim3f_grad_from(1, ...) -- the
// coefficients k_s, the rest of the pyramid, the float32 walks from the coarsest scale down to scale 1 --, then the coefficient walk and
// the adjoint walk of scale 0; the adjoint rounds each voxel once, to nearest-even, into the samples' encoding.
//   descs0_dev, descs_dev   as above
//   grads0_dev   count Grad3HDesc in device memory: the caller's gradient volumes
//   grads_dev    scales x count Grad3FDesc in device memory, [scale][pair]: rows >= 1 dense float32 scratch volumes; row 0 is not read
//   radius, taps as above
//   the rest     as launch_msssim3f_grad
hipError_t launch_msssim3h_grad(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, const Grad3HDesc* grads0_dev, const Grad3FDesc* grads_dev,
                                uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int type, float data_range,
                                uint32_t radius, const float* taps, const double* weights, int cu_count, const double* means, const float* g_out,
                                float* ks, float* coef, int which, hipStream_t stream);

// The pyramid step from the 16-bit scale 0 into row 1 of descs_dev, as the two launchers above enqueue it -- for them and for
// msssim3hk_kernels.hip; it does not depend on the window.
hipError_t launch_msssim3h_down(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                                uint32_t depth, int type, hipStream_t stream);

} // namespace ssim_hip

#endif
