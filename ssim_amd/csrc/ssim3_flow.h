// ssim3_flow.h -- what the host flows of the volume families share (ssim3f_abi.cpp: float32 volumes; ssim3h_abi.cpp: float16 /
// bfloat16 volumes; msssim3f_abi.cpp and msssim3h_abi.cpp: multi-scale SSIM of float32 and of 16-bit volumes), written once over the sample type: the sub-batch rule, the bytes of a staged volume, the launch through the
// context's ring of descriptor tables, the strided copy-back of a map, and the parsed window of a launch.  Not installed.
#ifndef SSIM_AMD_SSIM3_FLOW_H
#define SSIM_AMD_SSIM3_FLOW_H

#include "ssim_context.h"
#include "ssimk_kernels.h"      // kSKMaxRadius, window_taps

#include <vector>

namespace ssim_host {
namespace volumes {

const uint64_t kScratchCap = uint64_t(1) << 30;     // device scratch of one sub-batch

inline uint64_t round64(uint64_t bytes) { return (bytes + 63) & ~uint64_t(63); }

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

// One launch that reads a table of `bytes` from the next slot of the context's ring (ssim_samples_abi.cpp: ring_launch).
template <typename Fill, typename Launch>
int ring_launch(rmgr_ssim_hip_Context* c, size_t bytes, Fill fill, Launch launch)
{
    rmgr_ssim_hip_Context_::SfSlot& s = c->sf_slots[c->sf_next];
    c->sf_next = (c->sf_next + 1) % rmgr_ssim_hip_Context_::kSfSlots;
    if (s.pending) {
        HIP_TRY(hipEventSynchronize(s.used));
        s.pending = false;
    }
    HIP_TRY(s.used.ensure());
    int rc;
    if ((rc = s.pin.grow(bytes))) return rc;
    if ((rc = s.dev.grow(bytes))) return rc;
    fill(s.pin.get());
    HIP_TRY(hipMemcpyAsync(s.dev, s.pin, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch(const_cast<const uint8_t*>(s.dev.get())));
    HIP_TRY(hipEventRecord(s.used, c->stream));
    s.pending = true;
    return 0;
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

// The window of a launch: its radius and taps, centre first (ssimk_kernels.h: window_taps).  Radius 5 runs on the 11-tap kernels
// (ssim3f_kernels.hip / ssim3w_kernels.hip; ssim3h_kernels.hip), the smaller ones on ssim3k_kernels.hip / ssim3hk_kernels.hip.
struct Window3 {
    uint32_t radius;
    float    gf[ssim_hip::kSKMaxRadius + 1];
};

// The engine's window, that of every entry without _win: 11 taps, Gaussian, sigma 1.5.
inline Window3 default_window()
{
    Window3 w;
    w.radius = 5;
    ssim_hip::window_taps(5, ssim_hip::kSKGaussian, 1.5f, w.gf);
    return w;
}

// The window of a _win entry: NULL is the engine's; else size 3, 5, 7, 9 or 11, a known kind and -- Gaussian -- a finite sigma > 0.
inline int window_validate(const rmgr_ssim_hip_Window* window, Window3& w)
{
    if (window == NULL) { w = default_window(); return 0; }
    const uint32_t size = window->size;
    if (size < 3 || size > 11 || (size & 1u) == 0) return EINVAL;
    if (window->kind != RMGR_SSIM_HIP_WINDOW_GAUSSIAN && window->kind != RMGR_SSIM_HIP_WINDOW_UNIFORM) return EINVAL;
    w.radius = (size - 1) / 2;
    return ssim_hip::window_taps(w.radius, window->kind == RMGR_SSIM_HIP_WINDOW_UNIFORM ? ssim_hip::kSKUniform : ssim_hip::kSKGaussian, window->sigma, w.gf)
               ? 0 : EINVAL;
}

} // namespace volumes
} // namespace ssim_host

#endif
