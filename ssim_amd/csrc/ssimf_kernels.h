// ssimf_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, SSIM of float32 samples and its gradient) and the
// kernels (ssimf_kernels.hip).  Not installed.  The definition the kernels implement is written out in include/rmgr/ssim-hip.h
// (rmgr_ssim_hip_enqueue_ssimf, rmgr_ssim_hip_enqueue_ssimf_grad).
#ifndef SSIM_AMD_SSIMF_KERNELS_H
#define SSIM_AMD_SSIMF_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssim_hip {

// One pair of float32 images as the kernels address it: sample (x,y) of A is a[x*a_step + y*a_stride] (floats, signed), map element
// (x,y) is map[x*map_step + y*map_stride] (floats, signed; map == NULL: no map).
struct PairFDesc {
    const float* a;  int64_t a_step, a_stride;
    const float* b;  int64_t b_step, b_stride;
    float*       map; int64_t map_step, map_stride;
};

// The gradient planes of one pair (rmgr_ssim_hip_enqueue_ssimf_grad): element (x,y) of dLoss/dA is ga[x*ga_step + y*ga_stride];
// ga == NULL or gb == NULL: that gradient is not wanted.
struct GradFDesc {
    float* ga; int64_t ga_step, ga_stride;
    float* gb; int64_t gb_step, gb_stride;
};

enum { kSFStripW = 128 };
// The gradient kernel's output tile: kSFTile x kSFTile pixels at absolute positions, one 256-lane workgroup each.
enum { kSFTile = 32 };

// Strips of one launch: 128-column strips of strip_rows rows (a multiple of cell_rows) of every image, and the fp64 reduction
// cells of an image (64 columns x cell_rows rows at absolute positions; cell_rows depends on the height alone).
struct GeometryF {
    uint32_t width, height, count;
    uint32_t strip_rows, strips_x, strips_y;
    uint32_t cell_rows, cells_x, cells_y;
    uint64_t cells_per_image() const { return (uint64_t)cells_x * cells_y; }
};

// The strip kernel keeps coordinates in 32-bit registers and addresses a strip's samples as (64-bit row base) + (32-bit lane
// offset); a pair whose steps are too large for that runs on the form with 64-bit lane offsets.
inline bool fitsf_narrow(const PairFDesc& d)
{
    const int64_t lim = int64_t(1) << 21;     // 144 columns x |step| x 4 B stays below 2^31
    return d.a_step > -lim && d.a_step < lim && d.b_step > -lim && d.b_step < lim &&
           (d.map == 0 || (d.map_step > -lim && d.map_step < lim));
}

// Largest width / height the kernels take (32-bit coordinates with room for the halo and the strip round-up).
enum : uint32_t { kSFMaxDim = 0x7FFF0000u };

// Most pairs of this size one launch may take (its grid stays below 2^32 work-items, forward and gradient); 0 when one pair is
// already too large.
uint32_t ssimf_max_count(uint32_t width, uint32_t height);

// The strips of `count` pairs: strip_rows chosen so that the strips fill the chip's wave slots (cu_count CUs; <= 0: 256) in as few
// rounds as possible.  Results do not depend on it: per-pixel values and cells are the same for every strip height.
GeometryF planf(uint32_t width, uint32_t height, uint32_t count, int cu_count);

// Enqueues the strip kernel and the per-image reduction of `geo.count` pairs on `stream`.
//   descs_dev   geo.count descriptors in device memory; every pair has a map, or none has (map)
//   map_unit    every map has ssimStep == 1 and the width is even (8-byte map stores)
//   wide        some pair fails fitsf_narrow()
//   data_range  R > 0, finite: sets C1 and C2, and bounds the centre (see ssimf_kernels.hip)
//   taps        the window's six taps, centre first (ssimk_kernels.h: window_taps with radius 5; the default is the Gaussian of sigma 1.5)
//   partials    geo.count * geo.cells_per_image() doubles of device scratch
//   sums        geo.count doubles (device): each image's fp64 sum of its per-pixel values, in a fixed order
hipError_t launch_ssimf(const GeometryF& geo, const PairFDesc* descs_dev, bool map, bool map_unit, bool wide, float data_range,
                        const float (&taps)[6], int xcd_count, double* partials, double* sums, hipStream_t stream);

// Enqueues the gradient kernel of `count` pairs of width x height on `stream`: one fused launch that recomputes the statistics.
//   descs_dev   count PairFDesc in device memory (map ignored)
//   grads_dev   count GradFDesc in device memory
//   g_out       count floats in device memory: dLoss/dS_i
//   taps        the window's six taps, centre first, as launch_ssimf
//   which       1: dLoss/dA into ga; 2: dLoss/dB into gb; 3: both, in one pass, each with the bits it has alone
// Gradient planes are written, not accumulated; every pixel by exactly one work-item.
hipError_t launch_ssimf_grad(uint32_t width, uint32_t height, uint32_t count, const PairFDesc* descs_dev, const GradFDesc* grads_dev,
                             const float* g_out, float data_range, const float (&taps)[6], int which, hipStream_t stream);

// C1 and C2 of a data range, as the kernels use them: float((0.01 R)^2), float((0.03 R)^2) with the products in double.
void ssimf_constants(float data_range, float& c1, float& c2);

} // namespace ssim_hip

#endif
