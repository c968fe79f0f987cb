// msssim_kernels.h -- internal interface between the C ABI (ssim_hip_abi.cpp, MS-SSIM) and the multi-scale SSIM kernels
// (msssim_kernels.hip).  Not installed.  The definition the kernels implement is written out in include/rmgr/ssim-hip.h
// (rmgr_ssim_hip_compute_msssim_device).
#ifndef SSIM_AMD_MSSSIM_KERNELS_H
#define SSIM_AMD_MSSSIM_KERNELS_H

#include "ssim_kernels.h"

namespace ssim_hip {

enum { kMsMaxScales = 8, kMsTileW = 64, kMsTileH = 16 };

// Size of scale s of a width x height image: ceil(./2) per halving.
inline uint32_t ms_dim(uint32_t n, uint32_t s) { for (uint32_t i = 0; i < s; ++i) n = (n + 1) / 2; return n; }
inline uint64_t ms_tiles(uint32_t w, uint32_t h)
{
    return (uint64_t)((w + kMsTileW - 1) / kMsTileW) * ((h + kMsTileH - 1) / kMsTileH);
}

// Bytes of device scratch one launch_msssim() of `count` pairs needs: the float2 (a, b) planes of scales 1 .. scales-1 and the
// per-tile fp64 partials of every scale.
size_t msssim_scratch_bytes(uint32_t width, uint32_t height, uint32_t count, uint32_t scales);

// Most pairs of this size one launch_msssim() may take: its grids stay below the 2^32 work-items of one launch dimension.
uint32_t msssim_max_count(uint32_t width, uint32_t height, uint32_t scales);

// Enqueues MS-SSIM statistics of `count` pairs of one size on `stream`: per scale one statistics launch (and one downsample launch to
// the next scale), then one reduction launch.  descs_dev: count descriptors in device memory (uint8 images, any step / stride; the map
// fields are ignored).  sums_dev: count x scales x 2 doubles, [image][scale]{sum of cs, sum of ssim} over the W_s x H_s pixels of the
// scale, each summed in a fixed order over fixed tiles of the image: the bits do not depend on `count` or on the pair's place in it.
hipError_t launch_msssim(const PairDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales,
                         void* scratch, double* sums_dev, hipStream_t stream);

} // namespace ssim_hip

#endif
