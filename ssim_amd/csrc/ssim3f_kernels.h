// ssim3f_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, SSIM of float32 VOLUMES and its gradient) and the kernels
// (ssim3f_kernels.hip).  Not installed.  The definition the kernels implement is written out in include/rmgr/ssim-hip.h
// (rmgr_ssim_hip_enqueue_ssim3f, rmgr_ssim_hip_enqueue_ssim3f_grad).
#ifndef SSIM_AMD_SSIM3F_KERNELS_H
#define SSIM_AMD_SSIM3F_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssim_hip {

// One pair of float32 volumes as the kernels address it: voxel (x,y,z) of A is a[x*a_step + y*a_stride + z*a_slice] (floats, signed),
// map element (x,y,z) is map[x*map_step + y*map_stride + z*map_slice] (map == NULL: no map).  Every offset is a 64-bit product.
struct Pair3FDesc {
    const float* a;  int64_t a_step, a_stride, a_slice;
    const float* b;  int64_t b_step, b_stride, b_slice;
    float*       map; int64_t map_step, map_stride, map_slice;
};

// The gradient volumes of one pair; ga == NULL or gb == NULL: that gradient is not wanted.
struct Grad3FDesc {
    float* ga; int64_t ga_step, ga_stride, ga_slice;
    float* gb; int64_t gb_step, gb_stride, gb_slice;
};

// A workgroup's (x, y) tile, the depth of an fp64 reduction cell (slices, at absolute positions), the column group of one centre.
enum { kS3Tile = 16, kS3CellZ = 8, kS3GroupW = 128 };

// Largest width / height / depth (the 2-D float family's limit).
enum : uint32_t { kS3MaxDim = 0x7FFF0000u };

// The walk of one launch: every (x, y) tile of every volume is cut into z-chunks of chunk_slices slices (a multiple of kS3CellZ), one
// workgroup each; the fp64 cells are kS3Tile x kS3Tile x kS3CellZ voxels at absolute positions.
struct Geometry3F {
    uint32_t width, height, depth, count;
    uint32_t tiles_x, tiles_y, cells_z;
    uint32_t chunk_slices, chunks;
    uint64_t cells_per_volume() const { return (uint64_t)tiles_x * tiles_y * cells_z; }
    uint64_t voxels() const { return (uint64_t)width * height * depth; }
};

// Most volumes of this size one launch may take (its grid stays below 2^32 work-items); 0 when one volume is already too large.
uint32_t ssim3f_max_count(uint32_t width, uint32_t height, uint32_t depth);

// The walk of `count` volumes: chunk_slices chosen so that the workgroups fill the chip's wave slots (cu_count CUs; <= 0: 256) in as
// few slice-times as possible, `warmup` warm-up slices per chunk included (twice the window's radius: 10 for the 11-tap window).  Results
// do not depend on it.
Geometry3F plan3f(uint32_t width, uint32_t height, uint32_t depth, uint32_t count, int cu_count, uint32_t warmup = 10);

// Floats of coefficient scratch per voxel of the backward: k d_mu, k d_aa, k d_ab, and k d_mu of B when both gradients are wanted.
inline uint32_t ssim3f_coef_planes(int which) { return which == 3 ? 4u : 3u; }

// Enqueues the forward walk and the per-volume reduction of geo.count pairs on `stream`.
//   descs_dev   geo.count descriptors in device memory (map NULL: that pair has no map)
//   partials    geo.count * geo.cells_per_volume() doubles of device scratch
//   sums        geo.count doubles: each volume's fp64 sum of its per-voxel values, in a fixed order
//   taps        NULL: the engine's 11-tap Gaussian of sigma 1.5; else the six taps of an 11-tap window, centre first (here and below)
hipError_t launch_ssim3f(const Geometry3F& geo, const Pair3FDesc* descs_dev, float data_range, double* partials, double* sums, hipStream_t stream,
                         const float* taps = NULL);

// The second half of launch_ssim3f alone: each volume's cell partials summed in a fixed order into sums[0 .. geo.count-1].  The walk that
// fills `partials` is the caller's (ssim3h_kernels.hip: 16-bit samples).
hipError_t launch_ssim3f_reduce(const Geometry3F& geo, const double* partials, double* sums, hipStream_t stream);

// Enqueues the backward of geo.count pairs on `stream`: the forward walk that writes the coefficient volumes into `coef`
// (geo.count * ssim3f_coef_planes(which) * geo.voxels() floats, dense, [pair][plane][z][y][x]), then the adjoint walk.
//   g_out   geo.count floats in device memory: dLoss/dS_i
//   which   1: dLoss/dA into ga; 2: dLoss/dB into gb; 3: both, each with the bits it has alone
// Gradient volumes are written, not accumulated; every voxel by exactly one work-item.
hipError_t launch_ssim3f_grad(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, const float* g_out,
                              float data_range, int which, float* coef, hipStream_t stream, const float* taps = NULL);

// The second half of launch_ssim3f_grad alone: the adjoint walk that reads the coefficient volumes in `coef` and writes the gradient
// volumes.  The walk that fills `coef` is the caller's (ssim3w_kernels.hip: the per-voxel upstream gradient).
hipError_t launch_ssim3f_adjoint(const Geometry3F& geo, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, float data_range, int which,
                                 const float* coef, hipStream_t stream, const float* taps = NULL);

// What a walk of this file's shape takes by value besides its geometry: C1, C2 and the six taps (centre first) launch_ssim3f and
// launch_ssim3f_grad run with.  false: a data_range or a geometry those launches refuse.
struct Walk3FConstants { float c1, c2, gf[6]; };
bool ssim3f_walk_constants(const Geometry3F& geo, float data_range, Walk3FConstants& out, const float* taps = NULL);

} // namespace ssim_hip

#endif
