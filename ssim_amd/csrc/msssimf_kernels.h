// msssimf_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, multi-scale SSIM of float32 samples and its
// gradient) and the kernels (msssimf_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_msssimf, rmgr_ssim_hip_enqueue_msssimf_grad).
#ifndef SSIM_AMD_MSSSIMF_KERNELS_H
#define SSIM_AMD_MSSSIMF_KERNELS_H

#include "ssimf_kernels.h"      // PairFDesc, GradFDesc, kSFStripW, kSFTile, kSFMaxDim
#include "ssimk_kernels.h"      // kSKMaxRadius

namespace ssim_hip {

enum { kMSFMaxScales = 8 };

// Width or height of scale s: ceil(n / 2^s).
inline uint32_t msf_dim(uint32_t n, uint32_t s) { return (uint32_t)(((uint64_t)n + ((uint64_t(1) << s) - 1)) >> s); }

// Floats of one dense plane of scale s.
inline uint64_t msf_plane(uint32_t W, uint32_t H, uint32_t s) { return (uint64_t)msf_dim(W, s) * msf_dim(H, s); }

// Floats of the dense planes of scales 1 .. scales-1 of ONE image (the pyramid of a pair is two of these; so are its coarse gradients).
inline uint64_t msf_pyramid_floats(uint32_t W, uint32_t H, uint32_t scales)
{
    uint64_t t = 0;
    for (uint32_t s = 1; s < scales; ++s) t += msf_plane(W, H, s);
    return t;
}

// Reduction cells of one image at scale s (64 columns x cell_rows rows at absolute positions; two fp64 sums each: cs, ssim).
uint64_t msf_cells(uint32_t W, uint32_t H, uint32_t s);

// Doubles of cell partials `count` pairs need over all their scales.
inline uint64_t msf_partials(uint32_t W, uint32_t H, uint32_t count, uint32_t scales)
{
    uint64_t t = 0;
    for (uint32_t s = 0; s < scales; ++s) t += msf_cells(W, H, s) * 2 * count;
    return t;
}

// Strip height launch_msssimf gives the strips of one scale of `count` pairs, `width` x `height` that scale's size: chosen as
// ssimf_kernels.h's planf chooses it.  Results do not depend on the strip height.
uint32_t strip_rows_of(uint32_t width, uint32_t height, uint32_t count, int cu_count);

// Most pairs of this size one call to the launchers below may take (every grid stays below 2^32 work-items); 0 when one pair is
// already too large.
uint32_t msssimf_max_count(uint32_t width, uint32_t height);

// Enqueues the forward of `count` pairs on `stream`: the pyramid (one launch per step), the strip kernel of every scale, one
// reduction and the finalise kernel.
//   descs_dev    scales x count PairFDesc in device memory, [scale][pair]: scale 0 the caller's planes, scales >= 1 dense scratch
//                planes (step 1, stride W_s) that this call writes; map is ignored
//   wide         some scale-0 pair fails fitsf_narrow()
//   weights      `scales` weights (host), finite and >= 0
//   partials     msf_partials(width, height, count, scales) doubles of device scratch
//   means        count x scales x 2 doubles (device): [pair][scale]{mcs, mssim}
//   values       count doubles (device): the ReLU'd weighted product
hipError_t launch_msssimf(const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, bool wide,
                          float data_range, const double* weights, int cu_count, int xcd_count, double* partials, double* means,
                          double* values, hipStream_t stream);

// Enqueues the gradient of `count` pairs on `stream`: the coefficients k_s, the pyramid again, then the fused recomputing gradient
// kernel from the coarsest scale down to scale 0.
//   descs_dev    as above
//   grads_dev    scales x count GradFDesc in device memory, [scale][pair]: scale 0 the caller's gradient planes, scales >= 1 dense
//                scratch planes; ga == NULL or gb == NULL in all of them when that gradient is not wanted (which)
//   means        the forward's count x scales x 2 doubles (device)
//   g_out        count floats (device): dLoss/dMS_i
//   coef         count x scales floats of device scratch (k_s per pair and scale)
hipError_t launch_msssimf_grad(const PairFDesc* descs_dev, const GradFDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height,
                               uint32_t scales, float data_range, const double* weights, const double* means, const float* g_out,
                               float* coef, int which, hipStream_t stream);

// The two launchers above from scale `first` (0 or 1) on, for a caller whose scale 0 is not float32 (msssimh_kernels.hip) and who has
// launched, on the same stream, the pyramid step from its scale 0 into row 1 of descs_dev and -- forward -- its own strip kernel over
// scale 0's share of `partials`, which comes first and has msf_cells(width, height, 0) x 2 x count doubles.  first == 0 is the launcher
// above.  first == 1 skips the pyramid step, the strip kernel and the gradient kernel of scale 0 and reads nothing of row 0 of descs_dev
// and grads_dev; the reduction, the product and the coefficients cover every scale.  `wide` is scale 0's and ignored when first == 1.
//
// They also take the window, the same at every scale: its taps, centre first (ssimk_kernels.h: window_taps), and its radius, which must
// be 5 here: windows of 11 taps run on the kernels of this file with the window's taps -- the engine's taps: the two launchers above, bit
// for bit.  Radius 1 .. 4: launch_msssimk_from / launch_msssimk_grad_from of msssimk_kernels.h, on kernels of that radius.
hipError_t launch_msssimf_from(uint32_t first, uint32_t radius, const float (&taps)[kSKMaxRadius + 1], const PairFDesc* descs_dev, uint32_t count,
                               uint32_t width, uint32_t height, uint32_t scales, bool wide, float data_range, const double* weights, int cu_count,
                               int xcd_count, double* partials, double* means, double* values, hipStream_t stream);
hipError_t launch_msssimf_grad_from(uint32_t first, uint32_t radius, const float (&taps)[kSKMaxRadius + 1], const PairFDesc* descs_dev,
                                    const GradFDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, float data_range,
                                    const double* weights, const double* means, const float* g_out, float* coef, int which, hipStream_t stream);

// What does not depend on the window, as the launchers above enqueue it -- for them and for msssimk_kernels.hip, whose launchers differ in
// the strip and gradient kernels alone:
//   _pyramid  the pyramid of `count` pairs from scale `first` (0 or 1) on, one launch per step, finest first: row s + 1 of descs_dev from row s
//   _means    the reduction of every (pair, scale, kind) over `partials` as laid out above ([scale][pair][cell]{cs, ssim}, the cells of a
//             scale msf_cells()) into `means`, then the ReLU'd weighted product into `values`
//   _coef     k_s of every pair and scale into `coef` (count x scales floats), from the forward's means and g_out
hipError_t launch_msssimf_pyramid(uint32_t first, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales,
                                  hipStream_t stream);
hipError_t launch_msssimf_means(uint32_t count, uint32_t width, uint32_t height, uint32_t scales, const double* weights, const double* partials,
                                double* means, double* values, hipStream_t stream);
hipError_t launch_msssimf_coef(uint32_t count, uint32_t width, uint32_t height, uint32_t scales, const double* weights, const double* means,
                               const float* g_out, float* coef, hipStream_t stream);

} // namespace ssim_hip

#endif
