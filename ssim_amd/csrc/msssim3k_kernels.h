// msssim3k_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, multi-scale SSIM of float32 VOLUMES under a
// caller-chosen window) and the kernels of one scale of 3-D MS-SSIM under a window of 3, 5, 7 or 9 taps per axis (msssim3k_kernels.hip).
// Not installed.  The definition the kernels implement is written out in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssim3f_win and
// its siblings).  Windows of 11 taps run on the kernels of msssim3f_kernels.hip with the window's taps.
//
// The pyramid, the reduction, the product and the coefficients k_s do not depend on the window: they are msssim3f_kernels.hip's, on its
// kernels, enqueued through launch_msssim3f_pyramid / _means / _coef.  The cells of a scale, and with them the layout of the partials, do
// not depend on the radius either.
#ifndef SSIM_AMD_MSSSIM3K_KERNELS_H
#define SSIM_AMD_MSSSIM3K_KERNELS_H

#include "msssim3f_kernels.h"   // Pair3FDesc, Grad3FDesc, ms3_*, launch_msssim3f_pyramid / _means / _coef
#include "ssim3k_kernels.h"     // plan3k, kSKMaxRadius

namespace ssim_hip {

// launch_msssim3f_from() / launch_msssim3f_grad_from() for a window of `radius` (1 .. 4) with the taps gf[0 .. radius], the same at every
// scale: the walk and the adjoint walk of that radius, each scale's chunks planned by plan3k.  Arguments and layouts as there.
hipError_t launch_msssim3k_from(uint32_t first_scale, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Pair3FDesc* descs_dev, uint32_t count,
                                uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, float data_range, const double* weights, int cu_count,
                                double* partials, double* means, double* values, hipStream_t stream);
hipError_t launch_msssim3k_grad_from(uint32_t first_scale, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Pair3FDesc* descs_dev,
                                     const Grad3FDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales,
                                     float data_range, const double* weights, int cu_count, const double* means, const float* g_out, float* ks,
                                     float* coef, int which, hipStream_t stream);

} // namespace ssim_hip

#endif
