// ssim_context.cpp -- the context of the C ABI (include/rmgr/ssim-hip.h): create / destroy, the default pool of contexts behind
// ctx == NULL, what a context holds and giving it back, the arithmetic mode, memory queries and the raw memory entry points.
// The only host-layer file that differs between the two flavours of the library (RMGR_SSIM_USE_DOUBLE: the default mode).
#include "ssim_context.h"

#include <condition_variable>

namespace ssim_host {

// ---- the process-wide default contexts of the drop-in entry points (ctx == NULL) -------------------------------------
// The reference's compute_ssim() is re-entrant and has no global state (src/ssim.cpp:933-1106): six caller threads get six
// computations running side by side.  Rounds 1-4 ran every ctx == NULL call on ONE default context under its lock: six
// serialised copy-in -> kernel -> copy-out sequences.  Now the default is a small POOL of contexts on the default device
// ($RMGR_SSIM_HIP_DEVICE), each with its own stream, staging buffers and pinned memory: a call leases one for its duration,
// so that one caller's copy-in runs under another's kernel and a third's map on its way back.  Contexts are created on
// demand -- a single-threaded process only ever has one -- up to $RMGR_SSIM_HIP_POOL (default 4, 1 = the old behaviour);
// callers beyond that wait for a lease.  The arithmetic mode of the drop-in calls (rmgr_ssim_hip_set_mode(NULL, ...), i.e.
// rmgr::ssim::select_impl, $RMGR_SSIM_HIP_MODE, the double build's default) is a property of the pool, applied at lease time.
struct DefaultPool {
    std::mutex m;
    std::condition_variable freed;
    std::vector<rmgr_ssim_hip_Context*> all, idle;
    int device, limit, mode, create_err;
    bool configured;
    // memory policy (round 6): staging a context may keep between calls, in bytes (device + pinned); what each context held when its last lease ended
    uint64_t retain_cap;
    struct Held { rmgr_ssim_hip_Context* c; uint64_t device_bytes, pinned_bytes; };
    std::vector<Held> held;
    DefaultPool() : device(0), limit(4), mode(RMGR_SSIM_HIP_MODE_EXACT), create_err(0), configured(false), retain_cap(uint64_t(256) << 20) {}
};
// A LEAKED singleton: neither the pool nor its contexts are ever destroyed.  The process may still be inside a ctx == NULL call when exit() runs
// the static destructors or the library is unloaded (a daemon thread, a detached worker): its Lease must find the mutex, the condition variable
// and the vectors alive when it ends (rounds 1-4 kept a raw pointer for the same reason).
DefaultPool& pool()
{
    static DefaultPool* p = new DefaultPool;
    return *p;
}
#define g_pool (pool())

void pool_configure_locked()
{
    if (g_pool.configured) return;
    g_pool.configured = true;
    if (const char* s = getenv("RMGR_SSIM_HIP_DEVICE")) g_pool.device = atoi(s);
    if (const char* s = getenv("RMGR_SSIM_HIP_POOL")) { const int n = atoi(s); if (n >= 1 && n <= 64) g_pool.limit = n; }
    if (const char* s = getenv("RMGR_SSIM_HIP_POOL_RETAIN_MB")) {       // per context; 0: keep nothing between calls (the reference's behaviour); negative: no cap
        const long long mb = atoll(s);
        g_pool.retain_cap = mb < 0 ? ~uint64_t(0) : (uint64_t)mb << 20;
    }
    const char* m = getenv("RMGR_SSIM_HIP_MODE");
    if (m && atoi(m) >= RMGR_SSIM_HIP_MODE_EXACT && atoi(m) <= RMGR_SSIM_HIP_MODE_SEPARABLE) g_pool.mode = atoi(m);
#if defined(RMGR_SSIM_USE_DOUBLE) && RMGR_SSIM_USE_DOUBLE
    else g_pool.mode = RMGR_SSIM_HIP_MODE_DOUBLE;
#endif
}

// A context of the pool for the duration of one call; blocks while `limit` calls are in flight.
int pool_acquire(rmgr_ssim_hip_Context** out)
{
    std::unique_lock<std::mutex> lk(g_pool.m);
    pool_configure_locked();
    bool create_failed_here = false;     // this call tried to grow the pool and could not (out of memory ...): it waits for a lease instead of trying again
    for (;;) {
        if (!g_pool.idle.empty()) {
            *out = g_pool.idle.back();
            g_pool.idle.pop_back();
            (*out)->mode = g_pool.mode;
            return 0;
        }
        if (g_pool.create_err && g_pool.all.empty()) {
            if (g_pool.create_err == ENODEV) return ENODEV;                         // no usable device: every call fails the same way, at once
            g_pool.create_err = 0;                                                  // anything else (out of memory at that moment ...) is tried again by the next call
        }
        if ((int)g_pool.all.size() < g_pool.limit && !create_failed_here) {
            g_pool.all.push_back(NULL);                                             // reserve a slot; create outside the lock
            lk.unlock();
            rmgr_ssim_hip_Context* c = NULL;
            const int rc = rmgr_ssim_hip_create(&c, g_pool.device, NULL);
            lk.lock();
            if (rc || !c) {
                g_pool.all.erase(std::find(g_pool.all.begin(), g_pool.all.end(), (rmgr_ssim_hip_Context*)NULL));      // one reserved slot (any: they are alike)
                g_pool.create_err = rc ? rc : ENODEV;
                g_pool.freed.notify_all();
                if (g_pool.all.empty()) return g_pool.create_err;
                create_failed_here = true;
                continue;                                                           // others exist (or are being created): wait for one of them
            }
            *std::find(g_pool.all.begin(), g_pool.all.end(), (rmgr_ssim_hip_Context*)NULL) = c;
            c->mode = g_pool.mode;
            *out = c;
            return 0;
        }
        if (g_pool.all.empty()) return g_pool.create_err ? g_pool.create_err : ENODEV;      // nothing exists and nothing is being created: no lease will ever come
        g_pool.freed.wait(lk);                                                      // a context exists or is being created: its release (or its failure) wakes this call
    }
}

// What a context's grow-only staging holds right now (bytes of device memory / of pinned host memory).  Caller owns the context.
void context_held(rmgr_ssim_hip_Context* c, uint64_t& dev, uint64_t& pin)
{
    dev = pin = 0;
    c->for_each_staging([&](const auto& b) { (b.pinned ? pin : dev) += b.bytes(); });
}

// Gives a context's grow-only staging back to the system: device scratch, staged images and map, descriptor tables, pinned mirrors and bounce
// buffers.  Streams, events, the communicator and the tuning stay; the next call grows what it needs again.  The context must be the caller's
// (not in use by another thread); everything it has queued is waited for first.
int context_trim(rmgr_ssim_hip_Context* c)
{
    DeviceGuard device_guard_(c->device);
    if (device_guard_.rc) return device_guard_.rc;
    int rc = 0;
    if (!c->collectives.empty()) rc = comm_bounded_sync(c);
    else { const hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); } }
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->out_stream) (void)hipStreamSynchronize(c->out_stream);
    (void)hipGetLastError();
    c->for_each_staging([](auto& b) { b.drop(); });
    for (rmgr_ssim_hip_Context_::DescSlot& s : c->desc_slots) { s.live = 0; s.in_flight = false; }
    (void)hipGetLastError();
    return rc;
}

void pool_note_held_locked(rmgr_ssim_hip_Context* c, uint64_t dev, uint64_t pin)
{
    for (size_t i = 0; i < g_pool.held.size(); ++i)
        if (g_pool.held[i].c == c) { g_pool.held[i].device_bytes = dev; g_pool.held[i].pinned_bytes = pin; return; }
    try { const DefaultPool::Held h = {c, dev, pin}; g_pool.held.push_back(h); } catch (...) {}
}

// The lease ends: staging above the pool's retain cap ($RMGR_SSIM_HIP_POOL_RETAIN_MB, per context; default 256) goes back to the system
// before the context becomes available again -- the reference keeps nothing past the call (src/ssim.cpp:1048-1088) -- and what the
// context still holds is noted for rmgr_ssim_hip_get_default_pool_memory.
void pool_release(rmgr_ssim_hip_Context* c)
{
    uint64_t cap;
    { std::lock_guard<std::mutex> lk(g_pool.m); cap = g_pool.retain_cap; }
    uint64_t dev = 0, pin = 0;
    context_held(c, dev, pin);
    if (dev + pin > cap) {
        (void)context_trim(c);
        context_held(c, dev, pin);
    }
    {
        std::lock_guard<std::mutex> lk(g_pool.m);
        pool_note_held_locked(c, dev, pin);
        g_pool.idle.push_back(c);
    }
    g_pool.freed.notify_one();
}

// ctx == NULL set_mode / get_mode touch an int of the pool: when a default context exists they need no lease (they used to wait behind
// $RMGR_SSIM_HIP_POOL calls in flight, or create another context, to learn whether a device exists).  Only an EMPTY pool leases -- i.e. creates
// its first context -- to keep the contract that the call fails with ENODEV on a machine without a device (select_impl() returns 0 there).
int default_pool_has_device()
{
    {
        std::lock_guard<std::mutex> guard(g_pool.m);
        pool_configure_locked();
        for (size_t i = 0; i < g_pool.all.size(); ++i)
            if (g_pool.all[i] != NULL) return 0;
    }
    Lease probe;
    return probe.take(NULL);
}

} // namespace ssim_host

using namespace ssim_host;

extern "C" {

rmgr_int32_t rmgr_ssim_hip_get_device_count(rmgr_int32_t* count) RMGR_NOEXCEPT
{
    if (!count) return EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_create(rmgr_ssim_hip_Context** out, rmgr_int32_t device, void* stream) RMGR_NOEXCEPT
{
    if (!out) return EINVAL;
    *out = NULL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return ENODEV; }
    if (device < 0 || device >= n) return EINVAL;
    DeviceGuard device_guard_(device);
    if (device_guard_.rc) return device_guard_.rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    rmgr_ssim_hip_Context* c = NULL;
    try { c = new rmgr_ssim_hip_Context_(); } catch (...) { return ENOMEM; }
    c->device = device;
    c->cu_count = prop.multiProcessorCount;
    int xccs = 0, khz = 0;
    if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, device) == hipSuccess && xccs >= 1) c->xcd_count = xccs;
    else (void)hipGetLastError();
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) c->wall_clock_khz = khz;
    else (void)hipGetLastError();
    c->stream = static_cast<hipStream_t>(stream);
    if (!stream) {
        const hipError_t e = c->own_stream.ensure();
        if (e != hipSuccess) { delete c; return map_hip_error(e); }
        c->stream = c->own_stream;
    }
    snprintf(c->describe, sizeof(c->describe), "%s %s, %d CUs in %d XCDs, %.0f MHz, %.1f GiB; rmgr-ssim hip backend (code object gfx950)",
             prop.name, prop.gcnArchName, prop.multiProcessorCount, c->xcd_count, prop.clockRate / 1000.0, prop.totalGlobalMem / 1073741824.0);
    *out = c;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_destroy(rmgr_ssim_hip_Context* c) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    DeviceGuard device_guard_(c->device);
    if (!c->collectives.empty()) (void)comm_bounded_sync(c);      // the same bounded wait as rmgr_ssim_hip_synchronize (aborts a stuck collective)
    else (void)hipStreamSynchronize(c->stream);
    (void)rmgr_ssim_hip_comm_destroy(c);
    comm_forget_collectives(c);
    delete c;                                                     // on the context's device: every owned buffer, event and stream with it
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_set_mode(rmgr_ssim_hip_Context* c, rmgr_int32_t mode) RMGR_NOEXCEPT
{
    if (mode < RMGR_SSIM_HIP_MODE_EXACT || mode > RMGR_SSIM_HIP_MODE_SEPARABLE) return EINVAL;
    if (!c) {
        // the process-wide default contexts of the drop-in entry points (what rmgr::ssim::select_impl switches): a property of the
        // pool, applied to a context when a call leases it (calls already in flight keep the mode they were leased with).
        const int rc = default_pool_has_device();
        if (rc) return rc;
        std::lock_guard<std::mutex> guard(g_pool.m);
#if defined(RMGR_SSIM_USE_DOUBLE) && RMGR_SSIM_USE_DOUBLE
        if (mode == RMGR_SSIM_HIP_MODE_EXACT || mode == RMGR_SSIM_HIP_MODE_UNFUSED) mode = RMGR_SSIM_HIP_MODE_DOUBLE;   // a double build stays double
#endif
        g_pool.mode = mode;
        return 0;
    }
    c->mode = mode;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_get_mode(const rmgr_ssim_hip_Context* c, rmgr_int32_t* mode) RMGR_NOEXCEPT
{
    if (!mode) return EINVAL;
    if (!c) {                 // the process-wide default contexts, as for set_mode (ENODEV without a device)
        const int rc = default_pool_has_device();
        if (rc) return rc;
        std::lock_guard<std::mutex> guard(g_pool.m);
        *mode = g_pool.mode;
        return 0;
    }
    *mode = c->mode;
    return 0;
}

const char* rmgr_ssim_hip_get_kernel_source_id(void) RMGR_NOEXCEPT
{
    return ssim_hip::kernels_source_id();
}

rmgr_int32_t rmgr_ssim_hip_get_default_pool(rmgr_int32_t* contexts, rmgr_int32_t* limit) RMGR_NOEXCEPT
{
    std::lock_guard<std::mutex> lk(g_pool.m);
    pool_configure_locked();
    if (contexts) {
        *contexts = 0;
        for (size_t i = 0; i < g_pool.all.size(); ++i) *contexts += g_pool.all[i] != NULL;
    }
    if (limit) *limit = g_pool.limit;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_get_default_pool_memory(rmgr_uint64_t* deviceBytes, rmgr_uint64_t* pinnedBytes, rmgr_uint64_t* retainCapBytes) RMGR_NOEXCEPT
{
    std::lock_guard<std::mutex> lk(g_pool.m);
    pool_configure_locked();
    uint64_t dev = 0, pin = 0;
    for (size_t i = 0; i < g_pool.held.size(); ++i) { dev += g_pool.held[i].device_bytes; pin += g_pool.held[i].pinned_bytes; }
    if (deviceBytes) *deviceBytes = dev;
    if (pinnedBytes) *pinnedBytes = pin;
    if (retainCapBytes) *retainCapBytes = g_pool.retain_cap;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_trim_default_pool(void) RMGR_NOEXCEPT
{
    // the idle contexts leave the pool while they are trimmed (no call can lease one half-freed); contexts in use are left alone
    std::vector<rmgr_ssim_hip_Context*> mine;
    {
        std::lock_guard<std::mutex> lk(g_pool.m);
        mine.swap(g_pool.idle);
    }
    int rc = 0;
    for (size_t i = 0; i < mine.size(); ++i) {
        const int r = context_trim(mine[i]);
        if (r && !rc) rc = r;
    }
    {
        std::lock_guard<std::mutex> lk(g_pool.m);
        for (size_t i = 0; i < mine.size(); ++i) {
            uint64_t dev = 0, pin = 0;
            context_held(mine[i], dev, pin);
            pool_note_held_locked(mine[i], dev, pin);
            g_pool.idle.push_back(mine[i]);
        }
    }
    g_pool.freed.notify_all();
    return rc;
}

rmgr_int32_t rmgr_ssim_hip_trim(rmgr_ssim_hip_Context* c) RMGR_NOEXCEPT
{
    if (!c) return rmgr_ssim_hip_trim_default_pool();
    return context_trim(c);
}

rmgr_int32_t rmgr_ssim_hip_get_memory_info(const rmgr_ssim_hip_Context* c, rmgr_uint64_t* freeBytes, rmgr_uint64_t* totalBytes) RMGR_NOEXCEPT
{
    int device;
    if (c) device = c->device;
    else { std::lock_guard<std::mutex> lk(g_pool.m); pool_configure_locked(); device = g_pool.device; }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return ENODEV; }
    if (device < 0 || device >= n) return EINVAL;
    DeviceGuard device_guard_(device);
    if (device_guard_.rc) return device_guard_.rc;
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (freeBytes) *freeBytes = f;
    if (totalBytes) *totalBytes = t;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_get_abi_version(void) RMGR_NOEXCEPT
{
    return RMGR_SSIM_HIP_ABI_VERSION;
}

rmgr_int32_t rmgr_ssim_hip_malloc(rmgr_ssim_hip_Context* c, void** p, size_t size) RMGR_NOEXCEPT
{
    if (!c || !p) return EINVAL;
    USE_DEVICE(c);
    HIP_TRY(hipMalloc(p, size ? size : 1));
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_free(rmgr_ssim_hip_Context* c, void* p) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    HIP_TRY(hipFree(p));
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_memcpy_h2d(rmgr_ssim_hip_Context* c, void* dst, const void* src, size_t size) RMGR_NOEXCEPT
{
    if (!c || (size && (!dst || !src))) return EINVAL;
    USE_DEVICE(c);
    HIP_TRY(hipMemcpyAsync(dst, src, size, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_memcpy_d2h(rmgr_ssim_hip_Context* c, void* dst, const void* src, size_t size) RMGR_NOEXCEPT
{
    if (!c || (size && (!dst || !src))) return EINVAL;
    USE_DEVICE(c);
    HIP_TRY(hipMemcpyAsync(dst, src, size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

const char* rmgr_ssim_hip_describe(rmgr_ssim_hip_Context* c) RMGR_NOEXCEPT
{
    return c ? c->describe : "rmgr-ssim hip backend (no context)";
}

} // extern "C"
