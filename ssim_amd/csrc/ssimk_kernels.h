// ssimk_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, SSIM of float32 samples under a caller-chosen window)
// and the kernels of the windows of 3, 5, 7 and 9 taps (ssimk_kernels.hip).  Not installed.  The definition the kernels implement is
// written out in include/rmgr/ssim-hip.h (rmgr_ssim_hip_Window, rmgr_ssim_hip_enqueue_ssimf_win and its siblings).  Windows of 11 taps
// run on the kernels of ssimf_kernels.hip / ssimw_kernels.hip with the window's taps.
#ifndef SSIM_AMD_SSIMK_KERNELS_H
#define SSIM_AMD_SSIMK_KERNELS_H

#include "ssimw_kernels.h"      // PairFDesc, GradFDesc, GradOutFDesc, GeometryF, fitsf_narrow, ssimf_max_count, ssimf_constants

namespace ssim_hip {

// Window kinds, as RMGR_SSIM_HIP_WINDOW_* of the public header.
enum { kSKGaussian = 0, kSKUniform = 1 };
// Largest radius any float kernel serves (11 taps).
enum { kSKMaxRadius = 5 };

// The taps of a window of 2 * radius + 1 taps, centre first: gf[0 .. radius]; gf[radius + 1 .. 5] = 0.
//   Gaussian  g_i = exp(-(i i) / (2 s s)), s = double(sigma); the norm accumulated in double in the order i = 0 .. radius, g_0 once and
//             the others twice; tap i = float(g_i / norm).  radius 5, sigma 1.5f: the engine's taps, bit for bit.
//   uniform   every tap float(1.0 / (2 radius + 1)); sigma is not read.
// false: a radius outside 1 .. 5, an unknown kind, or a Gaussian sigma that is not finite or not > 0.
bool window_taps(uint32_t radius, uint32_t kind, float sigma, float (&gf)[kSKMaxRadius + 1]);

// tail[d] = g_d + ... + g_radius (0 beyond the radius) and the sum of all taps: sums of the float taps in double, rounded once.
void window_tails(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], float (&tail)[kSKMaxRadius + 1], float& total);

// planf() for a window of `radius` (1 .. 4): the same cells and strip columns; a strip pays 2 * radius warm-up rows.
GeometryF plank(uint32_t radius, uint32_t width, uint32_t height, uint32_t count, int cu_count);

// launch_ssimf() for a window of `radius` (1 .. 4) with the taps gf[0 .. radius]: the strip kernel of that radius and the per-image
// reduction of `geo.count` pairs on `stream`.  Arguments as launch_ssimf (no 8-byte-store form: `map` alone selects the map kernels).
hipError_t launch_ssimk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const GeometryF& geo, const PairFDesc* descs_dev, bool map, bool wide,
                        float data_range, int xcd_count, double* partials, double* sums, hipStream_t stream);

// launch_ssimf_grad() / launch_ssimw_grad_f() for a window of `radius` (1 .. 4): one kernel serves both upstream forms.
//   g_out      count floats in device memory, dLoss/dS_i: k = float(double(g_out[i]) / (double(W) double(H))) for every pixel; or NULL
//   gouts_dev  (g_out == NULL) count GradOutFDesc in device memory: k(p) = gMap(p)
// Exactly one of the two is given.  A plane whose every element is the scalar form's k gives that form's bits.
hipError_t launch_ssimk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], uint32_t width, uint32_t height, uint32_t count,
                             const PairFDesc* descs_dev, const GradFDesc* grads_dev, const float* g_out, const GradOutFDesc* gouts_dev,
                             float data_range, int which, hipStream_t stream);

} // namespace ssim_hip

#endif
