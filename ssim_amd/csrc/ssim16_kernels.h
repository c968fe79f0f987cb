// ssim16_kernels.h -- internal interface between the C ABI (ssim_samples_abi.cpp, high-bit-depth SSIM) and the SSIM kernels of
// 9- to 16-bit samples (ssim16_kernels.hip).  Not installed.  The definition the kernels implement is written out in
// include/rmgr/ssim-hip.h (rmgr_ssim_hip_enqueue_ssim16).
#ifndef SSIM_AMD_SSIM16_KERNELS_H
#define SSIM_AMD_SSIM16_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssim_hip {

// One pair of uint16 images as the kernels address it: sample (x,y) of A is a[x*a_step + y*a_stride] (samples, signed), map element
// (x,y) is map[x*map_step + y*map_stride] (floats, signed; map == NULL: no map).
struct Pair16Desc {
    const uint16_t* a;  int64_t a_step, a_stride;
    const uint16_t* b;  int64_t b_step, b_stride;
    float*          map; int64_t map_step, map_stride;
};

enum { kS16StripW = 128 };

// Strips of one launch: 128-column strips of strip_rows rows (a multiple of cell_rows) of every image, and the fp64 reduction
// cells of an image (64 columns x cell_rows rows at absolute positions; cell_rows depends on the height alone).
struct Geometry16 {
    uint32_t width, height, count;
    uint32_t strip_rows, strips_x, strips_y;
    uint32_t cell_rows, cells_x, cells_y;
    uint64_t cells_per_image() const { return (uint64_t)cells_x * cells_y; }
};

// The strip kernel keeps coordinates in 32-bit registers and addresses a strip's samples as (64-bit row base) + (32-bit lane
// offset); a pair whose steps are too large for that runs on the form with 64-bit lane offsets.
inline bool fits16_narrow(const Pair16Desc& d)
{
    const int64_t lim = int64_t(1) << 21;     // 144 columns x |step| x 4 B (map) stays below 2^31
    return d.a_step > -lim && d.a_step < lim && d.b_step > -lim && d.b_step < lim &&
           (d.map == 0 || (d.map_step > -lim && d.map_step < lim));
}

// Largest width / height the kernels take (32-bit coordinates with room for the 5-pixel halo and the strip round-up).
enum : uint32_t { kS16MaxDim = 0x7FFF0000u };

// Most pairs of this size one launch may take (its grid stays below 2^32 work-items); 0 when one pair is already too large.
uint32_t ssim16_max_count(uint32_t width, uint32_t height);

// The strips of `count` pairs: strip_rows chosen so that the strips fill the chip's wave slots (cu_count CUs; <= 0: 256) in as few
// rounds as possible.  Results do not depend on it: per-pixel values and cells are the same for every strip height.
Geometry16 plan16(uint32_t width, uint32_t height, uint32_t count, int cu_count);

// Enqueues the strip kernel and the per-image reduction of `geo.count` pairs on `stream`.
//   descs_dev   geo.count descriptors in device memory; every pair has a map, or none has (map)
//   map_unit    every map has ssimStep == 1 and the width is even (8-byte map stores)
//   wide        some pair fails fits16_narrow()
//   bit_depth   8 .. 16: L = 2^bit_depth - 1 sets C1 and C2
//   partials    geo.count * geo.cells_per_image() doubles of device scratch
//   sums        geo.count doubles (device): each image's fp64 sum of its per-pixel values, in a fixed order
hipError_t launch_ssim16(const Geometry16& geo, const Pair16Desc* descs_dev, bool map, bool map_unit, bool wide, uint32_t bit_depth,
                         int xcd_count, double* partials, double* sums, hipStream_t stream);

// C1 and C2 of a bit depth, as the kernels use them: float((0.01 L)^2), float((0.03 L)^2) with the products in double.
void ssim16_constants(uint32_t bit_depth, float& c1, float& c2);

} // namespace ssim_hip

#endif
