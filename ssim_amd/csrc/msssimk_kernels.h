// msssimk_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, multi-scale SSIM under a caller-chosen window) and the
// kernels of one scale of MS-SSIM under a window of 3, 5, 7 or 9 taps: msssimk_kernels.hip (float32 samples, every scale) and
// msssimhk_kernels.hip (float16 / bfloat16 samples, scale 0).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssimf_win and its siblings).  Windows of 11 taps run on the kernels of
// msssimf_kernels.hip / msssimh_kernels.hip with the window's taps.
//
// The pyramid, the reduction, the product and the coefficients do not depend on the window: they are msssimf_kernels.hip's (and, from a
// 16-bit scale 0, msssimh_kernels.hip's pyramid step), on its kernels, enqueued through launch_msssimf_pyramid / _means / _coef and
// launch_msssimh_down.  The cells of a scale, and with them the layout of the partials, do not depend on the radius either.
#ifndef SSIM_AMD_MSSSIMK_KERNELS_H
#define SSIM_AMD_MSSSIMK_KERNELS_H

#include "msssimh_kernels.h"    // PairFDesc, GradFDesc, PairHDesc, GradHDesc, kSHType*, msf_*
#include "ssimk_kernels.h"      // plank, kSKMaxRadius

namespace ssim_hip {

// launch_msssimf_from() / launch_msssimf_grad_from() for a window of `radius` (1 .. 4) with the taps gf[0 .. radius], the same at every
// scale: the strip and gradient kernels of that radius, each scale's strips planned by plank.  Arguments and layouts as there.
hipError_t launch_msssimk_from(uint32_t first, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const PairFDesc* descs_dev, uint32_t count,
                               uint32_t width, uint32_t height, uint32_t scales, bool wide, float data_range, const double* weights, int cu_count,
                               int xcd_count, double* partials, double* means, double* values, hipStream_t stream);
hipError_t launch_msssimk_grad_from(uint32_t first, uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const PairFDesc* descs_dev,
                                    const GradFDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, float data_range,
                                    const double* weights, const double* means, const float* g_out, float* coef, int which, hipStream_t stream);

// launch_msssimh() / launch_msssimh_grad() for such a window: scale 0 on the 16-bit kernels of that radius, scales >= 1 through the two
// launchers above with first == 1.  Arguments and layouts as there.
hipError_t launch_msssimhk(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                           uint32_t scales, int type, bool wide, float data_range, uint32_t radius, const float (&gf)[kSKMaxRadius + 1],
                           const double* weights, int cu_count, int xcd_count, double* partials, double* means, double* values, hipStream_t stream);
hipError_t launch_msssimhk_grad(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, const GradHDesc* grads0_dev, const GradFDesc* grads_dev,
                                uint32_t count, uint32_t width, uint32_t height, uint32_t scales, int type, float data_range, uint32_t radius,
                                const float (&gf)[kSKMaxRadius + 1], const double* weights, const double* means, const float* g_out, float* coef,
                                int which, hipStream_t stream);

} // namespace ssim_hip

#endif
