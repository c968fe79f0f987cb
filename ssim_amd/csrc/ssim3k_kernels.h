// ssim3k_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, SSIM of float32 VOLUMES under a caller-chosen window) and the
// kernels of the windows of 3, 5, 7 and 9 taps (ssim3k_kernels.hip).  Not installed.  The definition the kernels implement is written out
// in include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssim3f_win and its siblings).  Windows of 11 taps run on the kernels of
// ssim3f_kernels.hip / ssim3w_kernels.hip with the window's taps; the taps of every window are ssimk_kernels.h's (window_taps).
#ifndef SSIM_AMD_SSIM3K_KERNELS_H
#define SSIM_AMD_SSIM3K_KERNELS_H

#include "ssim3w_kernels.h"     // Pair3FDesc, Grad3FDesc, GradOut3FDesc, Geometry3F, plan3f, launch_ssim3f_reduce, ssim3f_walk_constants
#include "ssimk_kernels.h"      // kSKMaxRadius, window_taps, window_tails

namespace ssim_hip {

// plan3f() for a window of `radius` (1 .. 5): the same tiles and cells; a chunk pays 2 * radius warm-up slices.
inline Geometry3F plan3k(uint32_t radius, uint32_t width, uint32_t height, uint32_t depth, uint32_t count, int cu_count)
{
    return plan3f(width, height, depth, count, cu_count, 2 * radius);
}

// launch_ssim3f() for a window of `radius` (1 .. 4) with the taps gf[0 .. radius]: the walk of that radius, then launch_ssim3f_reduce.
// Arguments as launch_ssim3f.
hipError_t launch_ssim3k(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3FDesc* descs_dev, float data_range,
                         double* partials, double* sums, hipStream_t stream);

// launch_ssim3f_grad() / launch_ssim3w_grad() for a window of `radius` (1 .. 4): one coefficient walk serves both upstream forms, then the
// adjoint walk of that radius.
//   g_out      geo.count floats in device memory, dLoss/dS_i: k = float(double(g_out[i]) / (double(W) double(H) double(D))) for every voxel; or NULL
//   gouts_dev  (g_out == NULL) geo.count GradOut3FDesc in device memory: k(p) = gMap(p)
// Exactly one of the two is given.  A volume whose every element is the scalar form's k gives that form's bits.
hipError_t launch_ssim3k_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const Geometry3F& geo, const Pair3FDesc* descs_dev,
                              const Grad3FDesc* grads_dev, const float* g_out, const GradOut3FDesc* gouts_dev, float data_range, int which,
                              float* coef, hipStream_t stream);

} // namespace ssim_hip

#endif
