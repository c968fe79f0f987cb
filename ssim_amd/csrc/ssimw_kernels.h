// ssimw_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, gradient of the SSIM map for a per-pixel upstream
// gradient) and the kernels (ssimw_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssimf_map_grad, rmgr_ssim_hip_enqueue_ssimh_map_grad).
#ifndef SSIM_AMD_SSIMW_KERNELS_H
#define SSIM_AMD_SSIMW_KERNELS_H

#include "ssimf_kernels.h"      // PairFDesc, GradFDesc, kSFStripW, kSFTile, ssimf_max_count, ssimf_constants
#include "ssimh_kernels.h"      // PairHDesc, GradHDesc, kSHTypeF16, kSHTypeBF16

namespace ssim_hip {

// The upstream gradient plane of one pair: gMap(x,y) = g[x*g_step + y*g_stride] (floats, signed; 0 allowed: with both 0 one float
// stands for the whole plane).
struct GradOutFDesc {
    const float* g; int64_t g_step, g_stride;
};

// Enqueues the map-gradient kernel of `count` pairs of width x height on `stream`: ssimf's / ssimh's fused gradient launch with the
// uniform k = gOut / (W H) replaced by k(p) = gMap(p), read per pixel.  Tiles, centres and summation orders are those of
// launch_ssimf_grad, so a constant plane of float(gOut / (W H)) gives that launch's bits.
//   descs_dev   count PairFDesc / PairHDesc in device memory (map ignored)
//   grads_dev   count GradFDesc / GradHDesc in device memory
//   gouts_dev   count GradOutFDesc in device memory
//   type        (16-bit samples) kSHTypeF16 or kSHTypeBF16
//   taps        the window's six taps, centre first, as launch_ssimf
//   which       1: dLoss/dA into ga; 2: dLoss/dB into gb; 3: both, in one pass, each with the bits it has alone
// count <= ssimf_max_count(width, height).  Gradient planes are written, not accumulated; every pixel by exactly one work-item.
hipError_t launch_ssimw_grad_f(uint32_t width, uint32_t height, uint32_t count, const PairFDesc* descs_dev, const GradFDesc* grads_dev,
                               const GradOutFDesc* gouts_dev, float data_range, const float (&taps)[6], int which, hipStream_t stream);
hipError_t launch_ssimw_grad_h(uint32_t width, uint32_t height, uint32_t count, const PairHDesc* descs_dev, const GradHDesc* grads_dev,
                               int type, const GradOutFDesc* gouts_dev, float data_range, const float (&taps)[6], int which, hipStream_t stream);

} // namespace ssim_hip

#endif
