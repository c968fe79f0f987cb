// ssim3hk_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, SSIM of float16 / bfloat16 VOLUMES under a caller-chosen
// window) and the kernels of the windows of 3, 5, 7 and 9 taps (ssim3hk_kernels.hip).  Not installed.  The definition the kernels
// implement is written out in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssim3h_win and its siblings).  Windows of 11 taps run on the
// kernels of ssim3h_kernels.hip with the window's taps; the taps of every window are ssimk_kernels.h's (window_taps), the chunks are
// planned by ssim3k_kernels.h's plan3k.
#ifndef SSIM_AMD_SSIM3HK_KERNELS_H
#define SSIM_AMD_SSIM3HK_KERNELS_H

#include "ssim3h_kernels.h"     // Pair3HDesc, Grad3HDesc, GradOut3FDesc, Geometry3F, kSHTypeF16, kSHTypeBF16
#include "ssim3k_kernels.h"     // plan3k, kSKMaxRadius, window_taps, window_tails, launch_ssim3f_reduce, ssim3f_walk_constants

namespace ssim_hip {

// launch_ssim3k() for 16-bit samples: the walk of `radius` (1 .. 4) with the taps gf[0 .. radius] on the samples widened to float32, then
// launch_ssim3f_reduce.  Value, map and sums have the bits of launch_ssim3k on the widened volumes.
//   type   kSHTypeF16 or kSHTypeBF16
hipError_t launch_ssim3hk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3HDesc* descs_dev, int type,
                          float data_range, double* partials, double* sums, hipStream_t stream);

// launch_ssim3k_grad() for 16-bit samples: one coefficient walk serves both upstream forms (exactly one of g_out and gouts_dev is given),
// then the adjoint walk of that radius, which rounds each float32 gradient voxel once, to nearest-even, into the samples' encoding.  The
// coefficient volumes in `coef` stay float32.
hipError_t launch_ssim3hk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3HDesc* descs_dev,
                               const Grad3HDesc* grads_dev, int type, const float* g_out, const GradOut3FDesc* gouts_dev, float data_range,
                               int which, float* coef, hipStream_t stream);

} // namespace ssim_hip

#endif
