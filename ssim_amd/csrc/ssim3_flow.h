// ssim3_flow.h -- the volume-only pieces of the host flow of the volume families (ssim_volumes_abi.cpp), written once over the sample
// type: the bytes of a staged volume, the sub-batch rule, and the strided copy-back of a map.  What the image families use as well --
// the scratch cap, the parsed window, the ring launch -- is in ssim_flow.h.  Not installed.
#ifndef SSIM_AMD_SSIM3_FLOW_H
#define SSIM_AMD_SSIM3_FLOW_H

#include "ssim_flow.h"

#include <vector>

namespace ssim_host {
namespace volumes {

// The bytes of the sample range of a volume (Img: rmgr_ssim_hip_Img3F or _Img3H); lo: where the range starts, in samples relative to
// topLeft (<= 0).
template <typename Img>
size_t volume_bytes(const Img& im, uint32_t w, uint32_t h, uint32_t d, int64_t& lo)
{
    const int64_t ext[3] = {(int64_t)(w - 1) * (int64_t)im.step, (int64_t)(h - 1) * (int64_t)im.stride, (int64_t)(d - 1) * (int64_t)im.sliceStride};
    int64_t hi = 0;
    lo = 0;
    for (int k = 0; k < 3; ++k) { if (ext[k] < 0) lo += ext[k]; else hi += ext[k]; }
    return (size_t)(hi - lo + 1) * sizeof(*im.topLeft);
}

// Volumes of params[i0 ..] that one sub-batch takes (Params: rmgr_ssim_hip_Params3F or _Params3H): at least one; at most nmax (the
// launch limit) and, with `scratch` bytes per volume and -- stage: host pointers -- the staged volumes and float32 maps of each pair,
// kScratchCap of device scratch.  staged: the bytes its staged volumes and maps take, each rounded up to 64.
template <typename Params>
uint32_t take3f(const Params* params, uint32_t i0, uint32_t count, uint32_t nmax, uint64_t scratch, bool stage, uint64_t& staged)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    uint32_t n = 0;
    staged = 0;
    while (i0 + n < count && n < nmax) {
        uint64_t bytes = 0;
        if (stage) {
            const Params& p = params[i0 + n];
            int64_t lo;
            bytes += round64(volume_bytes(p.imgA, W, H, D, lo)) + round64(volume_bytes(p.imgB, W, H, D, lo));
            if (p.ssimMap) bytes += round64((uint64_t)W * H * D * 4);
        }
        if (n > 0 && scratch * (n + 1) + staged + bytes > kScratchCap) break;
        staged += bytes;
        ++n;
    }
    return n;
}

// Copies a dense W x H x D float32 map in device memory to the caller's map at its own step, stride and sliceStride (blocking).
template <typename Params>
int copy_map_back(const float* src, const Params& p, std::vector<float>& back)
{
    const uint32_t W = p.width, H = p.height, D = p.depth;
    const size_t n = (size_t)W * H * D;
    if (p.ssimStep == 1 && p.ssimStride == (ptrdiff_t)W && p.ssimSliceStride == (ptrdiff_t)W * (ptrdiff_t)H) {
        HIP_TRY(hipMemcpy(p.ssimMap, src, n * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    back.resize(n);
    HIP_TRY(hipMemcpy(&back[0], src, n * 4, hipMemcpyDeviceToHost));
    for (uint32_t z = 0; z < D; ++z)
        for (uint32_t y = 0; y < H; ++y) {
            float* row = p.ssimMap + (ptrdiff_t)z * p.ssimSliceStride + (ptrdiff_t)y * p.ssimStride;
            const float* s = &back[((size_t)z * H + y) * W];
            for (uint32_t x = 0; x < W; ++x) row[(ptrdiff_t)x * p.ssimStep] = s[x];
        }
    return 0;
}

} // namespace volumes
} // namespace ssim_host

#endif
