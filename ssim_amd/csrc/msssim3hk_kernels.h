// msssim3hk_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, multi-scale SSIM of float16 / bfloat16 VOLUMES under a
// caller-chosen window) and the kernels of scale 0 of 3-D MS-SSIM under a window of 3, 5, 7 or 9 taps per axis (msssim3hk_kernels.hip).
// Not installed.  The definition the kernels implement is written out in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssim3h_win and
// its siblings).  Windows of 11 taps run on the kernels of msssim3h_kernels.hip with the window's taps.
//
// Only scale 0 holds 16-bit samples: its walks and its adjoint are msssim3hk_kernels.hip's, its pyramid step is msssim3h_kernels.hip's
// (launch_msssim3h_down); scales >= 1 are msssim3k_kernels.hip's, run by launch_msssim3k_from / launch_msssim3k_grad_from with
// first_scale == 1 over the same partials, pyramid and coarse gradient volumes.
#ifndef SSIM_AMD_MSSSIM3HK_KERNELS_H
#define SSIM_AMD_MSSSIM3HK_KERNELS_H

#include "msssim3h_kernels.h"   // Pair3HDesc, Grad3HDesc, kSHType*, launch_msssim3h_down
#include "msssim3k_kernels.h"   // launch_msssim3k_from, launch_msssim3k_grad_from, plan3k, kSKMaxRadius

namespace ssim_hip {

// launch_msssim3h() / launch_msssim3h_grad() for a window of `radius` (1 .. 4) with the taps gf[0 .. radius]: scale 0 on the 16-bit
// kernels of that radius, scales >= 1 through launch_msssim3k_from / launch_msssim3k_grad_from.  Arguments and layouts as there.
hipError_t launch_msssim3hk(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                            uint32_t depth, uint32_t scales, int type, float data_range, uint32_t radius, const float (&gf)[kSKMaxRadius + 1],
                            const double* weights, int cu_count, double* partials, double* means, double* values, hipStream_t stream);
hipError_t launch_msssim3hk_grad(const Pair3HDesc* descs0_dev, const Pair3FDesc* descs_dev, const Grad3HDesc* grads0_dev, const Grad3FDesc* grads_dev,
                                 uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int type, float data_range,
                                 uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const double* weights, int cu_count, const double* means,
                                 const float* g_out, float* ks, float* coef, int which, hipStream_t stream);

} // namespace ssim_hip

#endif
