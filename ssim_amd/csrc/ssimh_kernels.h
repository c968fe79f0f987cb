// ssimh_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, SSIM of float16 / bfloat16 samples and its gradient) and
// the kernels (ssimh_kernels.hip).  Not installed.  The definition the kernels implement is written out in include/rmgr/ssim-hip.h
// (rmgr_ssim_hip_enqueue_ssimh, rmgr_ssim_hip_enqueue_ssimh_grad).
#ifndef SSIM_AMD_SSIMH_KERNELS_H
#define SSIM_AMD_SSIMH_KERNELS_H

#include "ssimf_kernels.h"      // GeometryF, kSFStripW, kSFTile, kSFMaxDim, ssimf_max_count

namespace ssim_hip {

// The encoding of the 16-bit samples of one call: RMGR_SSIM_HIP_SAMPLE_F16 / _BF16 of the public header.
enum { kSHTypeF16 = 0, kSHTypeBF16 = 1 };

// One pair of 16-bit float images as the kernels address it: sample (x,y) of A is a[x*a_step + y*a_stride] (16-bit samples, signed),
// map element (x,y) is map[x*map_step + y*map_stride] (floats, signed; map == NULL: no map).
struct PairHDesc {
    const uint16_t* a;  int64_t a_step, a_stride;
    const uint16_t* b;  int64_t b_step, b_stride;
    float*          map; int64_t map_step, map_stride;
};

// The gradient planes of one pair (rmgr_ssim_hip_enqueue_ssimh_grad), in the samples' encoding: element (x,y) of dLoss/dA is
// ga[x*ga_step + y*ga_stride]; ga == NULL or gb == NULL: that gradient is not wanted.
struct GradHDesc {
    uint16_t* ga; int64_t ga_step, ga_stride;
    uint16_t* gb; int64_t gb_step, gb_stride;
};

// Strips, cells and gradient tiles are those of ssimf_kernels.h: the sums and gradients have the bits of the float32 path.
enum { kSHStripW = kSFStripW };
enum { kSHTile = kSFTile };

typedef GeometryF GeometryH;

// The strip kernel addresses a strip's samples as (64-bit row base) + (32-bit lane offset in bytes); a pair whose steps are too
// large for that runs on the form with 64-bit lane offsets.
inline bool fitsh_narrow(const PairHDesc& d)
{
    const int64_t lim = int64_t(1) << 22;      // samples: 144 columns x |step| x 2 B stays below 2^31
    const int64_t mlim = int64_t(1) << 21;     // map:     128 columns x |step| x 4 B stays below 2^31
    return d.a_step > -lim && d.a_step < lim && d.b_step > -lim && d.b_step < lim &&
           (d.map == 0 || (d.map_step > -mlim && d.map_step < mlim));
}

// Largest width / height the kernels take (32-bit coordinates with room for the halo and the strip round-up).
enum : uint32_t { kSHMaxDim = kSFMaxDim };

// Most pairs of this size one launch may take: ssimf_max_count (the grids are the same).
uint32_t ssimh_max_count(uint32_t width, uint32_t height);

// The strips of `count` pairs, chosen as ssimf_kernels.h's planf chooses them.  Results do not depend on the strip height.
GeometryH planh(uint32_t width, uint32_t height, uint32_t count, int cu_count);

// Enqueues the strip kernel and the per-image reduction of `geo.count` pairs on `stream`.
//   descs_dev   geo.count descriptors in device memory; every pair has a map, or none has (map)
//   type        kSHTypeF16 or kSHTypeBF16
//   map_unit    every map has ssimStep == 1 and the width is even (8-byte map stores)
//   wide        some pair fails fitsh_narrow()
//   data_range  R > 0, finite: sets C1 and C2, and bounds the centre
//   taps        the window's six taps, centre first, as launch_ssimf (ssimk_kernels.h: window_taps at radius 5)
//   partials    geo.count * geo.cells_per_image() doubles of device scratch
//   sums        geo.count doubles (device): each image's fp64 sum of its per-pixel values, in a fixed order
hipError_t launch_ssimh(const GeometryH& geo, const PairHDesc* descs_dev, int type, bool map, bool map_unit, bool wide, float data_range,
                        const float (&taps)[6], int xcd_count, double* partials, double* sums, hipStream_t stream);

// Enqueues the gradient kernel of `count` pairs of width x height on `stream`: one fused launch that recomputes the statistics and
// rounds each gradient pixel once, to nearest-even, into the samples' encoding.
//   descs_dev   count PairHDesc in device memory (map ignored)
//   grads_dev   count GradHDesc in device memory
//   g_out       count floats in device memory: dLoss/dS_i
//   which       1: dLoss/dA into ga; 2: dLoss/dB into gb; 3: both, in one pass, each with the bits it has alone
// Gradient planes are written, not accumulated; every pixel by exactly one work-item.
hipError_t launch_ssimh_grad(uint32_t width, uint32_t height, uint32_t count, const PairHDesc* descs_dev, const GradHDesc* grads_dev,
                             int type, const float* g_out, float data_range, const float (&taps)[6], int which, hipStream_t stream);

} // namespace ssim_hip

#endif
