// ssim3h_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, SSIM of float16 / bfloat16 VOLUMES, its gradient and the
// gradient of its map) and the kernels (ssim3h_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssim3h, _ssim3h_grad, _ssim3h_map_grad).
#ifndef SSIM_AMD_SSIM3H_KERNELS_H
#define SSIM_AMD_SSIM3H_KERNELS_H

#include "ssim3w_kernels.h"     // Geometry3F, plan3f, ssim3f_max_count, ssim3f_coef_planes, ssim3f_walk_constants, GradOut3FDesc
#include "ssimh_kernels.h"      // kSHTypeF16, kSHTypeBF16

namespace ssim_hip {

// One pair of 16-bit float volumes as the kernels address it: voxel (x,y,z) of A is a[x*a_step + y*a_stride + z*a_slice] (16-bit
// samples, signed), map element (x,y,z) is map[x*map_step + y*map_stride + z*map_slice] (floats, signed; map == NULL: no map).  Every
// offset is a 64-bit product.
struct Pair3HDesc {
    const uint16_t* a;  int64_t a_step, a_stride, a_slice;
    const uint16_t* b;  int64_t b_step, b_stride, b_slice;
    float*          map; int64_t map_step, map_stride, map_slice;
};

// The gradient volumes of one pair, in the samples' encoding; ga == NULL or gb == NULL: that gradient is not wanted.
struct Grad3HDesc {
    uint16_t* ga; int64_t ga_step, ga_stride, ga_slice;
    uint16_t* gb; int64_t gb_step, gb_stride, gb_slice;
};

// Tiles, cells, chunks, the launch limit and the coefficient layout are those of ssim3f_kernels.h (Geometry3F, plan3f,
// ssim3f_max_count, ssim3f_coef_planes): sums and gradients have the bits of the float32 path on the widened volumes.

// Enqueues the forward walk and the per-volume reduction of geo.count pairs on `stream` (launch_ssim3f for 16-bit samples).
//   type   kSHTypeF16 or kSHTypeBF16
//   taps   NULL: the engine's 11-tap Gaussian of sigma 1.5; else the six taps of an 11-tap window, centre first (here and below)
hipError_t launch_ssim3h(const Geometry3F& geo, const Pair3HDesc* descs_dev, int type, float data_range, double* partials, double* sums,
                         hipStream_t stream, const float* taps = NULL);

// Enqueues the backward of geo.count pairs on `stream` (launch_ssim3f_grad for 16-bit samples): the walk that writes the float32
// coefficient volumes into `coef`, then the adjoint walk, which rounds each gradient voxel once, to nearest-even, into the samples'
// encoding.  g_out, which, coef: as for launch_ssim3f_grad.
hipError_t launch_ssim3h_grad(const Geometry3F& geo, const Pair3HDesc* descs_dev, const Grad3HDesc* grads_dev, int type, const float* g_out,
                              float data_range, int which, float* coef, hipStream_t stream, const float* taps = NULL);

// The same for a per-voxel upstream gradient (launch_ssim3w_grad for 16-bit samples): k(p) = gMap(p), float32, read per voxel through
// gouts_dev.  A constant volume of float(gOut / (W H D)) gives the bits of launch_ssim3h_grad.
hipError_t launch_ssim3h_map_grad(const Geometry3F& geo, const Pair3HDesc* descs_dev, const Grad3HDesc* grads_dev, const GradOut3FDesc* gouts_dev,
                                  int type, float data_range, int which, float* coef, hipStream_t stream, const float* taps = NULL);

} // namespace ssim_hip

#endif
