// ssim_flow.h -- what the host flows of the image families (ssim_samples_abi.cpp) and of the volume families (ssim_volumes_abi.cpp)
// share: the scratch cap of a sub-batch, the checks of a data range and the mapping of a sample type, the parsed window of a launch, and
// the launch through the context's ring of descriptor tables.  Not installed.
#ifndef SSIM_AMD_SSIM_FLOW_H
#define SSIM_AMD_SSIM_FLOW_H

#include "ssim_context.h"
#include "ssimh_kernels.h"      // kSHTypeF16, kSHTypeBF16
#include "ssimk_kernels.h"      // kSKMaxRadius, window_taps

#include <cmath>

namespace ssim_host {

const uint64_t kScratchCap = uint64_t(1) << 30;     // device scratch (partials, pyramids, staged samples and maps) of one sub-batch

inline uint64_t round64(uint64_t bytes) { return (bytes + 63) & ~uint64_t(63); }

inline bool valid_range(float r) { return r > 0.0f && std::isfinite(r); }

// What the kernels are told of a valid sample type (RMGR_SSIM_HIP_SAMPLE_F16 / _BF16).
inline int sample_type(uint32_t sampleType) { return sampleType == RMGR_SSIM_HIP_SAMPLE_BF16 ? ssim_hip::kSHTypeBF16 : ssim_hip::kSHTypeF16; }

// The window of a launch: its radius and taps, centre first (ssimk_kernels.h: window_taps).  Radius 5 runs on the 11-tap kernels of a
// family, the smaller ones on its ssimk / ssimhk / ssim3k / ssim3hk kernels.
struct Window {
    uint32_t radius;
    float    gf[ssim_hip::kSKMaxRadius + 1];
};

// The engine's window, that of every entry without _win: 11 taps, Gaussian, sigma 1.5.
inline Window default_window()
{
    Window w;
    w.radius = 5;
    ssim_hip::window_taps(5, ssim_hip::kSKGaussian, 1.5f, w.gf);
    return w;
}

// The window of a _win entry: NULL is the engine's; else size 3, 5, 7, 9 or 11, a known kind and -- Gaussian -- a finite sigma > 0.
inline int window_validate(const rmgr_ssim_hip_Window* window, Window& w)
{
    if (window == NULL) { w = default_window(); return 0; }
    const uint32_t size = window->size;
    if (size < 3 || size > 11 || (size & 1u) == 0) return EINVAL;
    if (window->kind != RMGR_SSIM_HIP_WINDOW_GAUSSIAN && window->kind != RMGR_SSIM_HIP_WINDOW_UNIFORM) return EINVAL;
    w.radius = (size - 1) / 2;
    return ssim_hip::window_taps(w.radius, window->kind == RMGR_SSIM_HIP_WINDOW_UNIFORM ? ssim_hip::kSKUniform : ssim_hip::kSKGaussian, window->sigma, w.gf)
               ? 0 : EINVAL;
}

// One launch that reads a table of `bytes` from the next slot of the context's ring (sf_slots): waits, at most, for the launch that read
// the slot kSfSlots enqueues ago; fill(pinned) writes the table, launch(device) enqueues its reader.
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

} // namespace ssim_host

#endif
