// ssimhk_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, SSIM of float16 / bfloat16 samples under a caller-chosen
// window) and the kernels of the windows of 3, 5, 7 and 9 taps (ssimhk_kernels.hip).  Not installed.  The definition the kernels
// implement is written out in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssimh_win and its siblings).  Windows of 11 taps run on the
// kernels of ssimh_kernels.hip / ssimw_kernels.hip with the window's taps; the taps of every window are ssimk_kernels.h's (window_taps),
// the strips are planned by its plank.
#ifndef SSIM_AMD_SSIMHK_KERNELS_H
#define SSIM_AMD_SSIMHK_KERNELS_H

#include "ssimk_kernels.h"      // plank, kSKMaxRadius, window_taps; PairHDesc, GradHDesc, GradOutFDesc, GeometryH, kSHTypeF16, kSHTypeBF16

namespace ssim_hip {

// launch_ssimk() for 16-bit samples: the strip kernel of `radius` (1 .. 4) with the taps gf[0 .. radius] on the samples widened to
// float32, and the per-image reduction.  `geo` is plank()'s.  Value, map and sums have the bits of launch_ssimk on the widened planes.
//   type   kSHTypeF16 or kSHTypeBF16
hipError_t launch_ssimhk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const GeometryH& geo, const PairHDesc* descs_dev, int type, bool map,
                         bool wide, float data_range, int xcd_count, double* partials, double* sums, hipStream_t stream);

// launch_ssimk_grad() for 16-bit samples: one kernel serves both upstream forms (exactly one of g_out and gouts_dev is given) and rounds
// each float32 gradient pixel once, to nearest-even, into the samples' encoding.
hipError_t launch_ssimhk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], uint32_t width, uint32_t height, uint32_t count,
                              const PairHDesc* descs_dev, const GradHDesc* grads_dev, int type, const float* g_out, const GradOutFDesc* gouts_dev,
                              float data_range, int which, hipStream_t stream);

} // namespace ssim_hip

#endif
