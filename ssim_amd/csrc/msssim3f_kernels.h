// msssim3f_kernels.h -- internal interface between the C ABI (ssim_volumes_abi.cpp, multi-scale SSIM of float32 VOLUMES and its gradient)
// and the kernels (msssim3f_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssim3f, rmgr_ssim_hip_enqueue_msssim3f_grad).
#ifndef SSIM_AMD_MSSSIM3F_KERNELS_H
#define SSIM_AMD_MSSSIM3F_KERNELS_H

#include "ssim3f_kernels.h"     // Pair3FDesc, Grad3FDesc, Geometry3F, plan3f, ssim3f_max_count, ssim3f_coef_planes

namespace ssim_hip {

enum { kMS3MaxScales = 8 };

// Width, height or depth of scale s: ceil(n / 2^s); an axis that has reached 1 stays 1.
inline uint32_t ms3_dim(uint32_t n, uint32_t s) { return (uint32_t)(((uint64_t)n + ((uint64_t(1) << s) - 1)) >> s); }

// Floats of one dense volume of scale s.
inline uint64_t ms3_voxels(uint32_t W, uint32_t H, uint32_t D, uint32_t s) { return (uint64_t)ms3_dim(W, s) * ms3_dim(H, s) * ms3_dim(D, s); }

// Floats of the dense volumes of scales 1 .. scales-1 of ONE volume (the pyramid of a pair is two of these; so are its coarse gradients).
inline uint64_t ms3_pyramid_floats(uint32_t W, uint32_t H, uint32_t D, uint32_t scales)
{
    uint64_t t = 0;
    for (uint32_t s = 1; s < scales; ++s) t += ms3_voxels(W, H, D, s);
    return t;
}

// Reduction cells of one volume at scale s (16 x 16 x 8 voxels at absolute positions; two fp64 sums each: cs, ssim).
inline uint64_t ms3_cells(uint32_t W, uint32_t H, uint32_t D, uint32_t s)
{
    const uint64_t w = ms3_dim(W, s), h = ms3_dim(H, s), d = ms3_dim(D, s);
    return ((w + kS3Tile - 1) / kS3Tile) * ((h + kS3Tile - 1) / kS3Tile) * ((d + kS3CellZ - 1) / kS3CellZ);
}

// Doubles of cell partials `count` pairs need over all their scales.
inline uint64_t ms3_partials(uint32_t W, uint32_t H, uint32_t D, uint32_t count, uint32_t scales)
{
    uint64_t t = 0;
    for (uint32_t s = 0; s < scales; ++s) t += ms3_cells(W, H, D, s) * 2 * count;
    return t;
}

// Most pairs of this size one call to the launchers below may take (every grid stays below 2^32 work-items: the walks of every scale,
// and the pyramid step into scale 1, one work-item per voxel); 0 when one pair is already too large.
uint32_t msssim3f_max_count(uint32_t width, uint32_t height, uint32_t depth);

// Bytes of device scratch ONE pair needs.  grad_planes 0, the forward: the pyramid of both volumes (scales >= 1; 8/7 bytes per scale-0
// voxel of the pair at most) and its cell partials.  grad_planes 1 or 2, the backward: the pyramid, grad_planes coarse gradient pyramids
// (4/7 or 8/7 bytes more), the coefficient volumes of the LARGEST scale (3 floats per voxel for one gradient, 4 for both: 12 / 16 bytes),
// which every scale reuses, and `scales` floats of k_s.
uint64_t msssim3f_scratch_bytes(uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int grad_planes);

// The sub-batch rule for device-resident volumes: pairs of every sub-batch but the last -- as many as `cap` bytes of scratch hold, at most
// msssim3f_max_count, at least one.  The host flow passes it to take3f as the launch limit, which adds a host call's staged volumes.
uint32_t msssim3f_per_sub_batch(uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, int grad_planes, uint64_t cap);

// Enqueues the forward of `count` pairs on `stream`: the pyramid (one launch per step), the walk of every scale, one reduction and the
// finalise kernel.
//   descs_dev    scales x count Pair3FDesc in device memory, [scale][pair]: scale 0 the caller's volumes, scales >= 1 dense scratch
//                volumes (step 1, stride W_s, slice W_s H_s) that this call writes; map must be NULL in all of them
//   weights      `scales` weights (host), finite and >= 0
//   partials     ms3_partials(width, height, depth, count, scales) doubles of device scratch
//   means        count x scales x 2 doubles (device): [pair][scale]{mcs, mssim}
//   values       count doubles (device): the ReLU'd weighted product
hipError_t launch_msssim3f(const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales,
                           float data_range, const double* weights, int cu_count, double* partials, double* means, double* values,
                           hipStream_t stream);

// Enqueues the gradient of `count` pairs on `stream`: the coefficients k_s, the pyramid again, then from the coarsest scale down the walk
// that writes the coefficient volumes and the adjoint walk that reads them and adds the coarser scale's gradient.
//   descs_dev    as above
//   grads_dev    scales x count Grad3FDesc in device memory, [scale][pair]: scale 0 the caller's gradient volumes, scales >= 1 dense
//                scratch volumes; ga == NULL or gb == NULL in all of them when that gradient is not wanted (which)
//   means        the forward's count x scales x 2 doubles (device)
//   g_out        count floats (device): dLoss/dMS_i
//   ks           scales x count floats of device scratch: k_s, [scale][pair]
//   coef         count * ssim3f_coef_planes(which) * width * height * depth floats of device scratch, reused by every scale
hipError_t launch_msssim3f_grad(const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height,
                                uint32_t depth, uint32_t scales, float data_range, const double* weights, int cu_count, const double* means,
                                const float* g_out, float* ks, float* coef, int which, hipStream_t stream);

// The two launchers above are the first_scale = 0 form of these under the engine's window.  first_scale = 1 is for a caller that runs
// scale 0 itself (msssim3h_kernels.hip: only scale 0 holds 16-bit samples): the pyramid steps from scale 1 down, the walks of scales >= 1,
// the reduction over ALL scales -- scale 0's cell partials first, at offset 0, laid out by plan3f(width, height, depth, count, cu_count) --,
// the product and k_s; in the backward the coefficient and adjoint walks from the coarsest scale down to scale 1.  Row 0 of descs_dev and of
// grads_dev is not read; the caller has written scale 1's volumes (forward: and scale 0's partials) earlier on `stream`.
//
// They also take the window, the same at every scale: its radius, which must be 5 here, and its taps, centre first (NULL: the engine's,
// as launch_ssim3f takes them).  Windows of 11 taps run on the kernels of this file with the window's taps -- the engine's taps: the two
// launchers above, bit for bit.  Radius 1 .. 4: launch_msssim3k_from / launch_msssim3k_grad_from of msssim3k_kernels.h, on kernels of
// that radius.
hipError_t launch_msssim3f_from(uint32_t first_scale, uint32_t radius, const float* taps, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width,
                                uint32_t height, uint32_t depth, uint32_t scales, float data_range, const double* weights, int cu_count,
                                double* partials, double* means, double* values, hipStream_t stream);
hipError_t launch_msssim3f_grad_from(uint32_t first_scale, uint32_t radius, const float* taps, const Pair3FDesc* descs_dev, const Grad3FDesc* grads_dev,
                                     uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, float data_range,
                                     const double* weights, int cu_count, const double* means, const float* g_out, float* ks, float* coef, int which,
                                     hipStream_t stream);

// What does not depend on the window, as the launchers above enqueue it -- for them and for msssim3k_kernels.hip, whose launchers differ
// in the walk and the adjoint walk of each scale alone:
//   _pyramid  the pyramid of `count` pairs from scale `first_scale` (0 or 1) on, one launch per step, finest first: row s + 1 of descs_dev
//             from row s
//   _means    the reduction of every (pair, scale, kind) over `partials` as laid out above ([scale][pair][cell]{cs, ssim}, the cells of a
//             scale ms3_cells()) into `means`, then the ReLU'd weighted product into `values`
//   _coef     k_s of every pair and scale into `ks` (scales x count floats, [scale][pair]), from the forward's means and g_out
hipError_t launch_msssim3f_pyramid(uint32_t first_scale, const Pair3FDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t depth,
                                   uint32_t scales, hipStream_t stream);
hipError_t launch_msssim3f_means(uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, const double* weights,
                                 const double* partials, double* means, double* values, hipStream_t stream);
hipError_t launch_msssim3f_coef(uint32_t count, uint32_t width, uint32_t height, uint32_t depth, uint32_t scales, const double* weights,
                                const double* means, const float* g_out, float* ks, hipStream_t stream);

} // namespace ssim_hip

#endif
