// ssim3w_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, gradient of the 3-D SSIM map for a per-voxel upstream
// gradient) and the kernels (ssim3w_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssim3f_map_grad).
#ifndef SSIM_AMD_SSIM3W_KERNELS_H
#define SSIM_AMD_SSIM3W_KERNELS_H

#include "ssim3f_kernels.h"     // Pair3FDesc, Grad3FDesc, Geometry3F, launch_ssim3f_adjoint, ssim3f_walk_constants

namespace ssim_hip {

// The upstream gradient volume of one pair: gMap(x,y,z) = g[x*g_step + y*g_stride + z*g_slice] (floats, signed; 0 allowed: with all
// three 0 one float stands for the whole volume).  Every offset is a 64-bit product.
struct GradOut3FDesc {
    const float* g; int64_t g_step, g_stride, g_slice;
};

// Enqueues the backward of geo.count pairs for a per-voxel upstream gradient on `stream`: launch_ssim3f_grad with the uniform
// k = gOut / (W H D) of its first walk replaced by k(p) = gMap(p), read per voxel; the adjoint walk is launch_ssim3f_adjoint.  Tiles,
// chunks, centres and summation orders are those of launch_ssim3f_grad, so a constant volume of float(gOut / (W H D)) gives that
// launch's bits.
//   descs_dev   geo.count Pair3FDesc in device memory (map ignored)
//   grads_dev   geo.count Grad3FDesc in device memory
//   gouts_dev   geo.count GradOut3FDesc in device memory
//   which       1: dLoss/dA into ga; 2: dLoss/dB into gb; 3: both, each with the bits it has alone
//   coef        geo.count * ssim3f_coef_planes(which) * geo.voxels() floats of device scratch
//   taps        NULL: the engine's window; else the six taps of an 11-tap window, centre first (launch_ssim3f)
// Gradient volumes are written, not accumulated; every voxel by exactly one work-item.
hipError_t launch_ssim3w_grad(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, const GradOut3FDesc* gouts_dev,
                              float data_range, int which, float* coef, hipStream_t stream, const float* taps = NULL);

} // namespace ssim_hip

#endif
