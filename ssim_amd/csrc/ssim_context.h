// ssim_context.h -- internal to the C ABI (include/rmgr/ssim-hip.h): the context, the resources it owns, and what the host-layer
// files share.  ssim_context.cpp creates and destroys contexts and keeps the default pool; ssim_hip_abi.cpp holds the entry points
// of 8-bit samples, ssim_samples_abi.cpp those of 16-bit, float32 and float16 / bfloat16 samples, ssim_volumes_abi.cpp those of
// float32 and float16 / bfloat16 volumes, single- and multi-scale (the two share ssim_flow.h); ssim_comm.cpp the RCCL all-reduce;
// ssim_tune.cpp profiling and tuning.  Not installed.
#ifndef SSIM_AMD_CONTEXT_H
#define SSIM_AMD_CONTEXT_H

#include <rmgr/ssim-hip.h>
#include "ssim_kernels.h"
#include "ssim16_kernels.h"
#include "ssimf_kernels.h"
#include "msssimf_kernels.h"
#include <rccl/rccl.h>      // types only: the library is dlopen()ed on first use, never linked

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

namespace ssim_host {

using ssim_hip::PairDesc;

inline int map_hip_error(hipError_t e)
{
    switch (e) {
    case hipSuccess:                return 0;
    case hipErrorOutOfMemory:       return ENOMEM;
    case hipErrorNoDevice:
    case hipErrorInvalidDevice:
    case hipErrorInsufficientDriver:
    case hipErrorNoBinaryForGpu:
    case hipErrorInvalidDeviceFunction:
        return ENODEV;
    case hipErrorInvalidValue:      return EINVAL;
    default:                        return ECHILD;   // "an error occurred in a worker" (src/ssim.cpp:1096-1097)
    }
}

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipGetLastError(); return ::ssim_host::map_hip_error(e_); } } while (0)

// Entry points run on the context's device WITHOUT changing the calling thread's current device (the reference API
// has no such side effect): the previous device is restored on every exit path.
struct DeviceGuard {
    int prev, rc;
    bool restore;
    DeviceGuard() : prev(-1), rc(0), restore(false) {}          // inactive until enter()
    explicit DeviceGuard(int dev) : prev(-1), rc(0), restore(false) { enter(dev); }
    int enter(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != dev) {
            const hipError_t e = hipSetDevice(dev);
            if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); return rc; }
            restore = prev >= 0;
        }
        return 0;
    }
    ~DeviceGuard() { if (restore) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define USE_DEVICE(c) ::ssim_host::DeviceGuard device_guard_((c)->device); if (device_guard_.rc) return device_guard_.rc

// Grow-only scratch of T in device (hipMalloc) or pinned host (hipHostMalloc) memory.  grow() frees first, then allocates a
// quarter more than asked plus 64 elements; bytes() is what the pool's memory report and its retain cap count.
template <typename T, bool Pinned>
class GrowBuffer {
public:
    static constexpr bool pinned = Pinned;
    GrowBuffer() = default;
    ~GrowBuffer() { drop(); }
    GrowBuffer(const GrowBuffer&) = delete;
    GrowBuffer& operator=(const GrowBuffer&) = delete;

    int grow(size_t need)
    {
        if (need <= cap_) return 0;
        if (p_) { HIP_TRY(release(p_)); p_ = NULL; cap_ = 0; }
        const size_t n = need + need / 4 + 64;
        void* p = NULL;
        HIP_TRY(Pinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T)));
        p_ = static_cast<T*>(p);
        cap_ = n;
        return 0;
    }
    void drop() { if (p_) (void)release(p_); p_ = NULL; cap_ = 0; }
    uint64_t bytes() const { return (uint64_t)cap_ * sizeof(T); }
    T* get() const { return p_; }
    operator T*() const { return p_; }

private:
    static hipError_t release(T* p) { return Pinned ? hipHostFree(p) : hipFree(p); }
    T* p_ = NULL;
    size_t cap_ = 0;       // elements
};
template <typename T> using DeviceBuffer = GrowBuffer<T, false>;
template <typename T> using PinnedBuffer = GrowBuffer<T, true>;

// An event (no timing) or a non-blocking stream, created by the first ensure() and destroyed with its owner.
inline hipError_t lazy_create(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
inline hipError_t lazy_create(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
inline void lazy_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void lazy_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }

template <typename H>
class Lazy {
public:
    Lazy() = default;
    ~Lazy() { if (h_) lazy_destroy(h_); }
    Lazy(const Lazy&) = delete;
    Lazy& operator=(const Lazy&) = delete;
    hipError_t ensure() { return h_ ? hipSuccess : lazy_create(&h_); }
    operator H() const { return h_; }
private:
    H h_ = NULL;
};
typedef Lazy<hipEvent_t>  LazyEvent;
typedef Lazy<hipStream_t> LazyStream;

} // namespace ssim_host

struct rmgr_ssim_hip_Context_ {
    template <typename T> using DeviceBuffer = ssim_host::DeviceBuffer<T>;
    template <typename T> using PinnedBuffer = ssim_host::PinnedBuffer<T>;
    typedef ssim_host::LazyEvent LazyEvent;
    typedef ssim_host::LazyStream LazyStream;

    LazyStream  own_stream;     // created when the caller brings no stream; destroyed last
    int         device = 0;
    int         cu_count = 0;
    int         xcd_count = 8;  // hipDeviceAttributeNumberOfXccs (8 on MI355X): the modulus of the kernels' XCD-aware workgroup order
    hipStream_t stream = NULL;   // the caller's or own_stream
    int         mode = RMGR_SSIM_HIP_MODE_EXACT;
    int         strip_rows = 0;
    int         variant = 0;

    // grow-only device scratch
    DeviceBuffer<double> partials;
    // Batch descriptor tables: a small ring of (device table, pinned mirror, "last launch that read it" event), so
    // that enqueueing a DIFFERENT batch never waits for the stream -- only for the launch kDescSlots enqueues ago --
    // and a serving loop that alternates between a few batches re-uses their uploaded tables.
    enum { kDescSlots = 4 };
    struct DescSlot {
        DeviceBuffer<ssim_hip::PairDesc> dev;
        PinnedBuffer<ssim_hip::PairDesc> host;        // pinned mirror of what `dev` holds (or will hold once the queued copy ran)
        size_t    live = 0;                 // entries of `host`/`dev` that are valid (0: nothing uploaded)
        LazyEvent used;                     // recorded after the last launch reading `dev`
        bool      in_flight = false;
    } desc_slots[kDescSlots];
    int       desc_next = 0;
    DeviceBuffer<uint8_t> stage_a, stage_b;     // host-pointer path
    DeviceBuffer<float>   stage_map;
    // pinned host scratch
    PinnedBuffer<double>  h_sums;               // per-image sums of the blocking entry points, written by the GPU
    // pipelined host batches: two device slots, two pinned gather buffers, a copy stream and per-slot events
    DeviceBuffer<uint8_t> slot_dev[2];
    PinnedBuffer<uint8_t> slot_pin[2];
    DeviceBuffer<double>  batch_sums;
    LazyStream  copy_stream;
    LazyEvent   slot_copied[2], slot_done[2];
    // banded single-pair host calls: a third stream for the map on its way back, per-band events
    enum { kMaxBands = 16 };
    LazyStream  out_stream;
    LazyEvent   band_copied[kMaxBands], band_done[kMaxBands];
    PinnedBuffer<uint8_t> h_stage;              // small image pairs are gathered here for one DMA
    PinnedBuffer<float>   h_map[2];             // bounce buffers for the map copy-back
    LazyEvent   map_ev[2];
    // multi-scale SSIM (rmgr_ssim_hip_compute_msssim_*): pyramid planes + tile partials, descriptor table, per-scale sums
    DeviceBuffer<uint8_t>  ms_scratch;
    DeviceBuffer<ssim_hip::PairDesc> ms_desc;
    PinnedBuffer<ssim_hip::PairDesc> ms_desc_pin;
    DeviceBuffer<double>   ms_sums;
    PinnedBuffer<double>   ms_sums_pin;
    // SSIM of 16-bit, float32 and float16 / bfloat16 samples and the gradients (rmgr_ssim_hip_*_ssim16, _ssimf*, _ssimh*): a ring of
    // descriptor tables (pair descriptors, then the gradient descriptors of a gradient launch), so that an enqueue waits at most for the
    // launch kSfSlots enqueues ago -- a training step's forward and backward never wait for each other --, cell partials, per-pair sums
    // written by the GPU.  Every family shares them: one stream, stream order.
    enum { kSfSlots = 8 };
    struct SfSlot {
        DeviceBuffer<uint8_t> dev;
        PinnedBuffer<uint8_t> pin;          // rewritten only once the launch that read its upload has run: `used`
        LazyEvent used;
        bool      pending = false;
    } sf_slots[kSfSlots];
    int                    sf_next = 0;
    DeviceBuffer<double>   sf_partials;
    PinnedBuffer<double>   sf_sums_pin;
    // multi-scale SSIM of float32 samples and its gradient (rmgr_ssim_hip_*_msssimf*), reused in stream order: the pyramid planes
    // of scales >= 1, the backward's gradient planes of scales >= 1, cell partials, the backward's coefficients k_s, and the
    // blocking entry points' values and means (device, and pinned for the copy back).  Descriptor tables come from sf_slots.
    // Multi-scale SSIM of volumes (rmgr_ssim_hip_*_msssim3f*, _msssim3h*; ssim_volumes_abi.cpp) uses the same six for its pyramid volumes, coarse
    // gradient volumes, k_s, cell partials and outputs, and s3_coef below for the coefficient volumes.
    DeviceBuffer<float>    msf_pyramid, msf_grads, msf_coef;
    DeviceBuffer<double>   msf_partials, msf_out;
    PinnedBuffer<double>   msf_out_pin;
    // SSIM of float32 and of float16 / bfloat16 volumes (rmgr_ssim_hip_*_ssim3f*, _ssim3h*; ssim_volumes_abi.cpp): the backward's
    // float32 coefficient volumes, rewritten by every sub-batch in stream order.  Descriptor tables, cell partials and pinned sums are
    // sf_slots, sf_partials and sf_sums_pin.
    DeviceBuffer<float>    s3_coef;

    // Every grow-only staging buffer above, once: what context_held counts and context_trim gives back.
    template <typename F> void for_each_staging(F f)
    {
        f(partials);
        for (DescSlot& s : desc_slots) { f(s.dev); f(s.host); }
        f(stage_a); f(stage_b); f(stage_map); f(h_sums); f(h_stage);
        for (int i = 0; i < 2; ++i) { f(slot_dev[i]); f(slot_pin[i]); f(h_map[i]); }
        f(batch_sums);
        f(ms_scratch); f(ms_desc); f(ms_desc_pin); f(ms_sums); f(ms_sums_pin);
        for (SfSlot& s : sf_slots) { f(s.dev); f(s.pin); }
        f(sf_partials); f(sf_sums_pin);
        f(msf_pyramid); f(msf_grads); f(msf_coef); f(msf_partials); f(msf_out); f(msf_out_pin);
        f(s3_coef);
    }

    bool profiling = false;
    DeviceBuffer<uint64_t> clock_dev;   // kClockWords device counters the profiled strip launches' first workgroups (one per XCD) add their shader cycles / reference ticks to (ssim_kernels.hip clock_begin); empty until profiling is first enabled; never trimmed
    int       wall_clock_khz = 100000;  // rate of s_memrealtime (hipDeviceAttributeWallClockRate; 100 MHz on MI355X)
    std::vector<std::pair<hipEvent_t, hipEvent_t> > pending;   // recorded, not yet read
    std::vector<std::pair<hipEvent_t, hipEvent_t> > free_events;
    uint64_t prof_launches = 0;
    double   prof_ms = 0.0;

    ncclComm_t comm = NULL;  // RCCL communicator (rmgr_ssim_hip_comm_*), NULL until comm_init
    // every queued all-reduce is bracketed by two events on the stream: what is still outstanding, oldest first.  The deadline of
    // rmgr_ssim_hip_synchronize / _destroy applies to ONE collective from the moment its turn has come (its `begin` event is complete) --
    // never to the kernels queued around it (30 s of legitimate work used to get a healthy communicator aborted)
    struct Collective { hipEvent_t begin, end; bool started; std::chrono::steady_clock::time_point since; };
    std::deque<Collective> collectives;
    std::vector<hipEvent_t> spare_events;
    bool       comm_nonblocking = false;   // created with ncclCommInitRankConfig(blocking = 0): calls may report "in progress"
    int        comm_ranks = 0;             // ncclCommCount of the communicator

    // rmgr_ssim_hip_tune: the measured choice per launch shape, consulted by enqueue() while the context is on its default tuning
    struct Tuned { uint32_t width, height, count; int mode; bool map; int variant, strip_rows; };
    std::vector<Tuned> tuned;
    // The entry for a launch shape under the context's current mode, or NULL.
    Tuned* tuned_for(uint32_t width, uint32_t height, uint32_t count, bool map)
    {
        for (Tuned& t : tuned)
            if (t.width == width && t.height == height && t.count == count && t.mode == mode && t.map == map) return &t;
        return NULL;
    }

    char describe[256] = "";

    ~rmgr_ssim_hip_Context_()       // the recycled event pools; everything else goes with its owning member
    {
        for (hipEvent_t e : spare_events) (void)hipEventDestroy(e);
        for (const auto& p : pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        for (const auto& p : free_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    }
};

namespace ssim_host {

// The default pool of contexts behind ctx == NULL (ssim_context.cpp).
int pool_acquire(rmgr_ssim_hip_Context** out);
void pool_release(rmgr_ssim_hip_Context* c);

// The context a call runs on: the caller's, or a leased default one (returned when the call ends).
struct Lease {
    rmgr_ssim_hip_Context* c = NULL;
    bool pooled = false;
    Lease() = default;
    int take(rmgr_ssim_hip_Context* given)
    {
        if (given) { c = given; return 0; }
        const int rc = pool_acquire(&c);
        if (rc) { c = NULL; return rc; }
        if (!c) return ENODEV;
        pooled = true;
        return 0;
    }
    ~Lease() { if (pooled && c) pool_release(c); }
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
};

// ssim_hip_abi.cpp
// Enqueue kernel + reduction for `count` pairs whose descriptors are in `descs` (host).
// y_begin / y_rows / reduce: the row window of this launch (ssim_kernels.h plan()); the default is the whole image.
// cells_out (row-band entry point only): the strips write their cell partials there instead of into the context's scratch.
int enqueue(rmgr_ssim_hip_Context* c, uint32_t width, uint32_t height, uint32_t count, const PairDesc* descs, bool any_map, double* sums_dev,
            uint32_t y_begin = 0, uint32_t y_rows = 0xFFFFFFFFu, bool reduce = true, double* cells_out = NULL);
int drain_profile(rmgr_ssim_hip_Context* c);
extern const double kWangWeights[5];     // the default weights of the multi-scale entry points (ssim_samples_abi.cpp uses them too)

// ssim_comm.cpp
int comm_bounded_sync(rmgr_ssim_hip_Context* c);
void comm_forget_collectives(rmgr_ssim_hip_Context* c);

} // namespace ssim_host

#endif
