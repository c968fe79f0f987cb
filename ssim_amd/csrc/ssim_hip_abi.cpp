// ssim_hip_abi.cpp -- the SSIM entry points of the C ABI declared in include/rmgr/ssim-hip.h for 8-bit samples: SSIM, multi-scale SSIM, the
// multi-device entry, the channel and luminance entries (the context itself: ssim_context.cpp; other sample types: ssim_samples_abi.cpp).
//
// Host-side driver of the GPU path: what src/ssim.cpp:933-1106 (compute_ssim) is to the
// reference's tile kernels, this file is to ssim_kernels.hip -- parameter validation with the
// reference's error codes, staging, launch, final mean.  No CPU arithmetic fallback exists: when
// no gfx950 device is usable every entry point fails loudly with ENODEV.
#include "ssim_context.h"
#include "msssim_kernels.h"

#include <cmath>
#include <condition_variable>
#include <thread>

namespace ssim_host {

const size_t kSmallStageBytes = size_t(768) << 10;   // image pairs up to this many bytes go through one pinned gather copy
const double kWangWeights[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};     // msssim.m (Wang, Simoncelli & Bovik 2003)

// The reference's parameter checks, in its order (src/ssim.cpp:962-978).
int validate(const float* ssim, const rmgr_ssim_Params* p, const rmgr_ssim_ThreadPool* tp)
{
    if (p == NULL) return EINVAL;                                    // src/ssim.cpp:1147-1151
    if (ssim == NULL && p->ssimMap == NULL) return EINVAL;
    if (p->imgA.topLeft == NULL || p->imgB.topLeft == NULL) return EINVAL;
    if (tp != NULL && tp->dispatch != NULL && tp->threadCount == 0u) return EINVAL;
    return 0;
}

// Byte extent [lo, hi] (inclusive, relative to topLeft) touched by a width x height image.
void extent(const rmgr_ssim_ImgParams& im, uint32_t w, uint32_t h, int64_t& lo, int64_t& hi)
{
    const int64_t dx = (int64_t)(w - 1) * (int64_t)im.step, dy = (int64_t)(h - 1) * (int64_t)im.stride;
    lo = (dx < 0 ? dx : 0) + (dy < 0 ? dy : 0);
    hi = (dx > 0 ? dx : 0) + (dy > 0 ? dy : 0);
}

// The bytes a width x height image occupies, as staged: `size` of them from `lo` (relative to topLeft) on, `padded` = size rounded
// up to `align` (a power of two); to_host / to_device copy them to pinned memory at once / to device memory on a stream.
struct ByteRange {
    const uint8_t* first = NULL;
    int64_t lo = 0;
    size_t size = 0, padded = 0;
    ByteRange() = default;
    ByteRange(const rmgr_ssim_ImgParams& im, uint32_t w, uint32_t h, size_t align)
    {
        int64_t hi;
        extent(im, w, h, lo, hi);
        first = im.topLeft + lo;
        size = (size_t)(hi - lo + 1);
        padded = (size + align - 1) & ~(align - 1);
    }
    void to_host(uint8_t* dst) const { memcpy(dst, first, size); }
    hipError_t to_device(uint8_t* dst, hipStream_t stream) const { return hipMemcpyAsync(dst, first, size, hipMemcpyHostToDevice, stream); }
};

// Event pair for timing one launch (NULLs when profiling is off).  The pair enters `pending` only after BOTH events
// were recorded (commit_events); a launch that fails, or launches nothing, hands it back (release_events).
int acquire_events(rmgr_ssim_hip_Context* c, hipEvent_t& b, hipEvent_t& e)
{
    b = e = NULL;
    if (!c->profiling) return 0;
    if (!c->free_events.empty()) {
        b = c->free_events.back().first; e = c->free_events.back().second;
        c->free_events.pop_back();
        return 0;
    }
    HIP_TRY(hipEventCreate(&b));
    hipError_t err = hipEventCreate(&e);
    if (err != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(b); b = e = NULL; return map_hip_error(err); }
    return 0;
}

void release_events(rmgr_ssim_hip_Context* c, hipEvent_t b, hipEvent_t e)
{
    if (!b) return;
    try { c->free_events.push_back(std::make_pair(b, e)); }
    catch (...) { (void)hipEventDestroy(b); (void)hipEventDestroy(e); }
}

int commit_events(rmgr_ssim_hip_Context* c, hipEvent_t b, hipEvent_t e)
{
    if (!b) return 0;
    try { c->pending.push_back(std::make_pair(b, e)); }
    catch (...) { (void)hipEventDestroy(b); (void)hipEventDestroy(e); return ENOMEM; }
    return 0;
}

// Reads every pending pair.  A pair that cannot be read is dropped (its events recycled) and reported once; the
// pairs before and after it are counted exactly once.
int drain_profile(rmgr_ssim_hip_Context* c)
{
    int rc = 0;
    for (size_t i = 0; i < c->pending.size(); ++i) {
        float ms = 0.f;
        hipError_t err = hipEventSynchronize(c->pending[i].second);
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, c->pending[i].first, c->pending[i].second);
        if (err == hipSuccess) {
            c->prof_ms += ms;
            c->prof_launches += 1;
        } else {
            (void)hipGetLastError();
            if (!rc) rc = map_hip_error(err);
        }
        release_events(c, c->pending[i].first, c->pending[i].second);
    }
    c->pending.clear();
    return rc;
}

// Device copy of a batch's descriptor table: re-used when any ring slot already holds exactly these descriptors,
// otherwise uploaded into the next slot (waiting, at most, for the launch that read that slot kDescSlots batches ago).
int upload_descs(rmgr_ssim_hip_Context* c, const PairDesc* descs, uint32_t count, int& slot_out)
{
    typedef rmgr_ssim_hip_Context_::DescSlot Slot;
    for (int i = 0; i < rmgr_ssim_hip_Context_::kDescSlots; ++i) {
        Slot& s = c->desc_slots[i];
        if (s.live == count && memcmp(s.host, descs, sizeof(PairDesc) * count) == 0) { slot_out = i; return 0; }
    }
    const int k = c->desc_next;
    c->desc_next = (k + 1) % rmgr_ssim_hip_Context_::kDescSlots;
    Slot& s = c->desc_slots[k];
    if (s.in_flight) { HIP_TRY(hipEventSynchronize(s.used)); s.in_flight = false; }
    s.live = 0;
    int rc;
    if ((rc = s.dev.grow(count))) return rc;
    if ((rc = s.host.grow(count))) return rc;
    HIP_TRY(s.used.ensure());
    memcpy(s.host, descs, sizeof(PairDesc) * count);
    HIP_TRY(hipMemcpyAsync(s.dev, s.host, sizeof(PairDesc) * count, hipMemcpyHostToDevice, c->stream));
    s.live = count;
    slot_out = k;
    return 0;
}

int enqueue(rmgr_ssim_hip_Context* c, uint32_t width, uint32_t height, uint32_t count, const PairDesc* descs, bool any_map, double* sums_dev,
            uint32_t y_begin, uint32_t y_rows, bool reduce, double* cells_out)
{
    int variant = c->variant, strip_rows = c->strip_rows;
    if (variant == 0 && strip_rows == 0 && y_begin == 0 && y_rows == 0xFFFFFFFFu && !cells_out)      // default tuning, whole images: a measured choice, if one was made
        if (const rmgr_ssim_hip_Context_::Tuned* t = c->tuned_for(width, height, count, any_map)) { variant = t->variant; strip_rows = t->strip_rows; }
    if (variant == 0 && strip_rows == 0) variant = ssim_hip::default_variant(width, height, count, c->mode, c->cu_count);
    bool all_fit = true;
    for (uint32_t i = 0; i < count && all_fit; ++i)
        all_fit = ssim_hip::fits_strip2(descs[i], width, height);
    if (!all_fit) variant = 1;
    ssim_hip::Geometry geo = ssim_hip::plan(width, height, count, c->mode, strip_rows, variant, c->cu_count, c->xcd_count, y_begin, y_rows);
    geo.wide = !all_fit;                             // the 64-bit form of the one-column kernel only where it is needed
    geo.map_unit = any_map && (width & 1u) == 0;     // the 8-byte map stores of the two-column kernel (ssim_kernels.hip, MAP == 2)
    for (uint32_t i = 0; i < count && geo.map_unit; ++i)
        geo.map_unit = descs[i].map != NULL && descs[i].map_step == 1;
    int rc = cells_out ? 0 : c->partials.grow(ssim_hip::partials_size(geo));
    if (rc) return rc;
    PairDesc single = descs[0];
    const PairDesc* descs_dev = NULL;
    int slot = -1;
    if (count > 1) {
        if ((rc = upload_descs(c, descs, count, slot))) return rc;
        descs_dev = c->desc_slots[slot].dev;
        if (any_map && !single.map) single.map = reinterpret_cast<float*>(1);  // only its non-NULLness is used
    }
    const bool launches_kernel = count > 0 && geo.strips_x > 0 && geo.strips_y > 0;
    hipEvent_t eb = NULL, ee = NULL;
    if (launches_kernel && (rc = acquire_events(c, eb, ee))) return rc;
    const hipError_t err = ssim_hip::launch(geo, c->mode, variant, ssim_hip::interleaved_group(descs, count), descs_dev, single, cells_out ? cells_out : c->partials.get(), sums_dev, c->stream, eb, ee, reduce, c->profiling ? c->clock_dev.get() : NULL);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        release_events(c, eb, ee);
        if (slot >= 0) { (void)hipStreamSynchronize(c->stream); c->desc_slots[slot].live = 0; }   // the table upload may still be queued
        return map_hip_error(err);
    }
    // the launch is queued and reads the slot's device table: mark the slot busy BEFORE anything else can fail
    if (slot >= 0) {
        const hipError_t e = hipEventRecord(c->desc_slots[slot].used, c->stream);
        if (e != hipSuccess) {              // cannot track the reader: wait for it instead of leaving the table unprotected
            (void)hipGetLastError();
            (void)hipStreamSynchronize(c->stream);
            release_events(c, eb, ee);
            return map_hip_error(e);
        }
        c->desc_slots[slot].in_flight = true;
    }
    if ((rc = commit_events(c, eb, ee))) return rc;
    return 0;
}

PairDesc make_desc(const rmgr_ssim_Params& p)
{
    PairDesc d;
    d.a = p.imgA.topLeft; d.a_step = p.imgA.step; d.a_stride = p.imgA.stride;
    d.b = p.imgB.topLeft; d.b_step = p.imgB.step; d.b_stride = p.imgB.stride;
    d.map = p.ssimMap;
    d.map_step = p.ssimMap ? p.ssimStep : 0;      // src/ssim.cpp:980-987
    d.map_stride = p.ssimMap ? p.ssimStride : 0;
    return d;
}

float mean_of(double sum, uint32_t width, uint32_t height)
{
    return float(sum / double(uint32_t(width * height)));   // src/ssim.cpp:1102 (32-bit product kept)
}

// ---- the per-pixel map on its way back to the caller (host-pointer entry points) ----

// Rows [y0, y1) of the dense device map (c->stage_map, W floats per row) into the caller's map, any ssimStep /
// ssimStride.  Unit step and a positive stride: the DMA engine writes the caller's rows directly (one 2-D copy).
// Anything else: through two pinned bounce buffers in chunks, the CPU scattering chunk k-1 while chunk k is in
// flight.  Returns after the rows are in the caller's memory.
int map_rows_to_host(rmgr_ssim_hip_Context* c, const rmgr_ssim_Params& p, uint32_t y0, uint32_t y1, hipStream_t stream)
{
    const uint32_t W = p.width;
    if (y1 <= y0 || W == 0) return 0;
    const float* src = c->stage_map + (size_t)y0 * W;
    if (p.ssimStep == 1 && p.ssimStride >= (ptrdiff_t)W) {
        float* dst = p.ssimMap + (ptrdiff_t)y0 * p.ssimStride;
        if (p.ssimStride == (ptrdiff_t)W)
            HIP_TRY(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)(y1 - y0) * W, hipMemcpyDeviceToHost, stream));
        else
            HIP_TRY(hipMemcpy2DAsync(dst, sizeof(float) * (size_t)p.ssimStride, src, sizeof(float) * W, sizeof(float) * W, y1 - y0, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return 0;
    }
    int rc;
    const size_t rowsPerChunk = std::max<size_t>(1, (size_t(8) << 20) / (sizeof(float) * W));
    const size_t chunkFloats = rowsPerChunk * W;
    if ((rc = c->h_map[0].grow(chunkFloats))) return rc;
    if ((rc = c->h_map[1].grow(chunkFloats))) return rc;
    for (int i = 0; i < 2; ++i) HIP_TRY(c->map_ev[i].ensure());
    const size_t total = y1 - y0, chunks = (total + rowsPerChunk - 1) / rowsPerChunk;
    for (size_t k = 0; k <= chunks; ++k) {
        if (k < chunks) {
            const size_t r0 = k * rowsPerChunk, rows = std::min(rowsPerChunk, total - r0);
            HIP_TRY(hipMemcpyAsync(c->h_map[k & 1], src + r0 * W, sizeof(float) * rows * W, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipEventRecord(c->map_ev[k & 1], stream));
        }
        if (k > 0) {
            const size_t j = k - 1, r0 = j * rowsPerChunk, rows = std::min(rowsPerChunk, total - r0);
            HIP_TRY(hipEventSynchronize(c->map_ev[j & 1]));
            const float* from = c->h_map[j & 1];
            for (size_t y = 0; y < rows; ++y, from += W) {
                float* row = p.ssimMap + (ptrdiff_t)(y0 + r0 + y) * p.ssimStride;
                if (p.ssimStep == 1) memcpy(row, from, sizeof(float) * W);
                else for (uint32_t x = 0; x < W; ++x) row[(ptrdiff_t)x * p.ssimStep] = from[x];
            }
        }
    }
    return 0;
}

// Rows of both images occupy disjoint byte ranges (no column-major or otherwise row-interleaved layout), and the
// image is tall enough to be worth cutting: the precondition of the banded pipeline.
bool bandable(const rmgr_ssim_Params& p)
{
    if (p.height < 256 || p.width == 0) return false;
    const rmgr_ssim_ImgParams* im[2] = {&p.imgA, &p.imgB};
    for (int i = 0; i < 2; ++i) {
        const int64_t span = (int64_t)(p.width - 1) * (im[i]->step < 0 ? -(int64_t)im[i]->step : (int64_t)im[i]->step) + 1;
        const int64_t stride = im[i]->stride < 0 ? -(int64_t)im[i]->stride : (int64_t)im[i]->stride;
        if (stride < span) return false;
    }
    return true;
}

// Byte range [lo, hi] (relative to topLeft) of rows [r0, r1) of a row-separable image.
void rows_extent(const rmgr_ssim_ImgParams& im, uint32_t w, uint32_t r0, uint32_t r1, int64_t& lo, int64_t& hi)
{
    const int64_t dx = (int64_t)(w - 1) * (int64_t)im.step;
    const int64_t ya = (int64_t)r0 * (int64_t)im.stride, yb = (int64_t)(r1 - 1) * (int64_t)im.stride;
    lo = std::min(ya, yb) + (dx < 0 ? dx : 0);
    hi = std::max(ya, yb) + (dx > 0 ? dx : 0);
}

// Bands of a host pair: ~2 Mpixel (8 MB of map) per band, at most kMaxBands, at most 4 without a map -- measured on MI355X / PCIe Gen5
// (profiles/r02_host_probe.txt): 4096^2 10.6 Gpix/s at 6-8 bands (8.2 unpipelined), 8192^2 12.0 at 16 (8.7), 2048^2 8.1 at 2 (7.0).
// $RMGR_SSIM_HIP_BANDS overrides the count.
int band_count(const rmgr_ssim_Params& p)
{
    int bands = (int)std::min<uint64_t>(((uint64_t)p.width * p.height + (1u << 21) - 1) >> 21, rmgr_ssim_hip_Context_::kMaxBands);
    if (!p.ssimMap) bands = std::min(bands, 4);
    if (const char* e = getenv("RMGR_SSIM_HIP_BANDS")) bands = atoi(e);
    return std::max(1, std::min<int>(bands, rmgr_ssim_hip_Context_::kMaxBands));
}

// The banded pipeline of one large host pair (see the call site), with or without a map.  `d` addresses the staged
// device copies (not yet filled), loA/loB are the byte offsets of the images' lowest addresses relative to topLeft.
// Without a map there is nothing to send back and no helper thread: the bands only hide the kernel behind the H2D copy
// of the following band.  Measured (round 3, profiles/r03_host_probe.txt, on a build that banded every map-less call): every
// additional pageable copy costs ~20 us, more than the ~12 us of kernel a band hides at 4096^2 (0.742 ms unbanded, 0.762 /
// 0.790 / 0.891 ms at 2 / 4 / 8 bands); it pays from 8192^2 on (2.795 -> 2.650 ms at 4 bands), so by default only such images
// take this path without a map ($RMGR_SSIM_HIP_BANDS forces it for any size: tools/host_call_probe.py).
int compute_banded(rmgr_ssim_hip_Context* c, const rmgr_ssim_Params& p, const PairDesc& d, int64_t loA, int64_t loB)
{
    const uint32_t W = p.width, H = p.height;
    const int bands = band_count(p);
    const uint32_t cell = ssim_hip::cell_rows_for(H);         // windows start on reduction-cell boundaries
    uint32_t band_rows = ((H + bands - 1) / bands + cell - 1) & ~(cell - 1);
    if (band_rows < 64) band_rows = 64;
    const int n = (int)((H + band_rows - 1) / band_rows);
    HIP_TRY(c->copy_stream.ensure());
    HIP_TRY(c->out_stream.ensure());
    for (int k = 0; k < n; ++k) { HIP_TRY(c->band_copied[k].ensure()); HIP_TRY(c->band_done[k].ensure()); }
    // input chunk k = rows [in[k], in[k+1]); once it has landed, output rows [out[k], out[k+1]) can be computed:
    // everything up to one reduction cell (>= the 5 halo rows) short of the rows present.
    uint32_t in[rmgr_ssim_hip_Context_::kMaxBands + 1], out[rmgr_ssim_hip_Context_::kMaxBands + 1];
    for (int k = 0; k <= n; ++k) {
        in[k] = std::min<uint64_t>((uint64_t)k * band_rows, H);
        out[k] = (k == 0) ? 0 : (k == n ? H : in[k] - cell);
    }

    // The helper thread returns band k's map rows while the caller's thread feeds bands k+1, k+2, ...
    struct Shared {
        std::mutex m; std::condition_variable cv;
        int launched; bool abort; int rc;
    } sh;
    sh.launched = 0; sh.abort = false; sh.rc = 0;
    struct Worker {
        rmgr_ssim_hip_Context* c; const rmgr_ssim_Params* p; Shared* sh; const uint32_t* out; int n;
        void operator()() const
        {
            int rc = 0;
            if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); rc = ENODEV; }
            for (int k = 0; k < n && rc == 0; ++k) {
                {
                    std::unique_lock<std::mutex> lk(sh->m);
                    sh->cv.wait(lk, [&] { return sh->launched > k || sh->abort; });
                    if (sh->launched <= k) break;            // aborted before band k was launched
                }
                const hipError_t e = hipEventSynchronize(c->band_done[k]);
                if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); break; }
                rc = map_rows_to_host(c, *p, out[k], out[k + 1], c->out_stream);
            }
            std::lock_guard<std::mutex> lk(sh->m);
            if (rc && !sh->rc) sh->rc = rc;
        }
    };
    const Worker work = {c, &p, &sh, out, n};
    const bool with_map = p.ssimMap != NULL;
    std::thread helper;
    bool threaded = with_map;
    if (with_map) { try { helper = std::thread(work); } catch (...) { threaded = false; } }

    int rc = 0;
    const rmgr_ssim_ImgParams* img[2] = {&p.imgA, &p.imgB};
    uint8_t* stage[2] = {c->stage_a, c->stage_b};
    const int64_t lo_img[2] = {loA, loB};
    for (int k = 0; k < n && rc == 0; ++k) {
        for (int j = 0; j < 2 && rc == 0; ++j) {
            int64_t lo, hi;
            rows_extent(*img[j], W, in[k], in[k + 1], lo, hi);
            const hipError_t e = hipMemcpyAsync(stage[j] + (lo - lo_img[j]), img[j]->topLeft + lo, (size_t)(hi - lo + 1), hipMemcpyHostToDevice, c->copy_stream);
            if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); }
        }
        hipError_t e = rc ? hipSuccess : hipEventRecord(c->band_copied[k], c->copy_stream);
        if (!rc && e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->band_copied[k], 0);
        if (!rc && e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); }
        if (!rc && out[k + 1] > out[k])
            rc = enqueue(c, W, H, 1, &d, with_map, c->h_sums, out[k], out[k + 1] - out[k], k == n - 1);
        if (!rc) {
            e = hipEventRecord(c->band_done[k], c->stream);
            if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); }
        }
        if (!rc) {
            { std::lock_guard<std::mutex> lk(sh.m); sh.launched = k + 1; }
            sh.cv.notify_one();
        }
    }
    if (rc) {
        { std::lock_guard<std::mutex> lk(sh.m); sh.abort = true; }
        sh.cv.notify_one();
    }
    if (threaded) helper.join();
    else if (!rc && with_map) work();             // no thread could be started: the same steps, serially
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); if (!rc) rc = map_hip_error(e); }
    (void)hipStreamSynchronize(c->copy_stream);
    return rc ? rc : sh.rc;
}

// ---- the caller's thread pool (rmgr_ssim_ThreadPool) ---------------------------------------------------------------------------
// The reference cuts the image into 256 x 64 tiles and hands them to threadPool->dispatch as jobs: `fct` is to be called exactly jobCount
// times with jobNum in [0, jobCount), on up to threadCount threads, args[t] used by one thread at a time; a non-zero return becomes ECHILD
// -- when a global value was asked for (src/ssim.cpp:1048-1100, include/rmgr/ssim.h:448-466).  Rounds 1-5 validated the pool and never
// called it.  Here the contract is kept with the unit of work this engine has on the HOST side: a ROW BAND of the pair -- its source rows
// (with the 5-row halo) to the device, the strips of the band (a row window of the launch: cells at absolute positions, so any order and
// any number of threads give the one-launch result bit for bit), and, with a map, the band's map rows back into the caller's buffer.  Jobs
// are independent and may run in any order; the context itself is single-threaded, so a job holds the call's lock while it enqueues and
// lets go of it while it waits for its map rows -- with several pool threads one band's copy-back overlaps the next band's copy-in and
// kernel, as in the library's own pipeline (compute_banded()).  After dispatch returns: the fixed-order reduction of the cells, the mean.
struct PoolCall {
    rmgr_ssim_hip_Context* c;
    const rmgr_ssim_Params* host;      // the caller's parameters (host pointers)
    PairDesc d;                        // the staged pair (device pointers)
    int64_t loA, loB;                  // byte offsets of the images' lowest addresses relative to topLeft
    uint32_t jobs, band_rows;
    bool whole;                        // the layout cannot be cut into row bands: one job stages the whole byte ranges
    std::mutex m;
    int rc;                            // first error of a job (errno)
    uint32_t ran;                      // jobs that ran to their end
    char done[rmgr_ssim_hip_Context_::kMaxBands];
};

void pool_job(void* arg, rmgr_uint32_t jobNum) RMGR_NOEXCEPT
{
    PoolCall& pc = **static_cast<PoolCall**>(arg);
    rmgr_ssim_hip_Context* c = pc.c;
    const rmgr_ssim_Params& p = *pc.host;
    const uint32_t W = p.width, H = p.height;
    int rc = 0;
    DeviceGuard on_device(c->device);            // a pool thread has a current device of its own
    std::unique_lock<std::mutex> lk(pc.m);
    if (jobNum >= pc.jobs || pc.done[jobNum]) { if (!pc.rc) pc.rc = ECHILD; return; }      // a pool that invents or repeats jobs: "an error occurred in a worker"
    if (on_device.rc) rc = on_device.rc;
    const uint32_t y0 = jobNum * pc.band_rows, y1 = (uint32_t)std::min<uint64_t>((uint64_t)y0 + pc.band_rows, H);
    if (!rc) {
        const rmgr_ssim_ImgParams* img[2] = {&p.imgA, &p.imgB};
        uint8_t* stage[2] = {const_cast<uint8_t*>(pc.d.a) + pc.loA, const_cast<uint8_t*>(pc.d.b) + pc.loB};      // = the staging buffers' first bytes
        const int64_t lo_img[2] = {pc.loA, pc.loB};
        for (int j = 0; j < 2 && !rc; ++j) {
            int64_t lo, hi;
            if (pc.whole) extent(*img[j], W, H, lo, hi);
            else rows_extent(*img[j], W, y0 >= 5 ? y0 - 5 : 0, (uint32_t)std::min<uint64_t>((uint64_t)y1 + 5, H), lo, hi);      // the band's rows and its 5-row halo
            const hipError_t e = hipMemcpyAsync(stage[j] + (lo - lo_img[j]), img[j]->topLeft + lo, (size_t)(hi - lo + 1), hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); }
        }
    }
    if (!rc) rc = enqueue(c, W, H, 1, &pc.d, p.ssimMap != NULL, c->h_sums, y0, y1 - y0, false);
    if (!rc && p.ssimMap) {
        const bool direct = p.ssimStep == 1 && p.ssimStride >= (ptrdiff_t)W;       // the DMA engine writes the caller's rows itself: no shared bounce buffers
        if (direct) {
            hipError_t e = c->band_done[jobNum].ensure();
            if (e == hipSuccess) e = c->out_stream.ensure();
            if (e == hipSuccess) e = hipEventRecord(c->band_done[jobNum], c->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->out_stream, c->band_done[jobNum], 0);
            if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); }
            if (!rc) {
                // the copy is queued behind this band's kernel on the third stream; the wait happens WITHOUT the call's lock
                float* dst = p.ssimMap + (ptrdiff_t)y0 * p.ssimStride;
                const float* src = c->stage_map + (size_t)y0 * W;
                if (p.ssimStride == (ptrdiff_t)W) e = hipMemcpyAsync(dst, src, sizeof(float) * (size_t)(y1 - y0) * W, hipMemcpyDeviceToHost, c->out_stream);
                else e = hipMemcpy2DAsync(dst, sizeof(float) * (size_t)p.ssimStride, src, sizeof(float) * W, sizeof(float) * W, y1 - y0, hipMemcpyDeviceToHost, c->out_stream);
                hipEvent_t mine = NULL;
                if (e == hipSuccess) e = hipEventCreateWithFlags(&mine, hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventRecord(mine, c->out_stream);
                lk.unlock();
                if (e == hipSuccess) e = hipEventSynchronize(mine);
                if (mine) (void)hipEventDestroy(mine);
                if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); }
                lk.lock();
            }
        } else {
            rc = map_rows_to_host(c, p, y0, y1, c->stream);      // through the context's two bounce buffers: under the lock
        }
    }
    if (rc) { if (!pc.rc) pc.rc = rc; return; }
    pc.done[jobNum] = 1;
    ++pc.ran;
}

// compute_ssim on host pointers through the caller's pool.  `dev` / `d`: the staged pair (buffers grown, nothing copied yet).
int compute_via_pool(rmgr_ssim_hip_Context* c, float* ssim, const rmgr_ssim_Params& p, const PairDesc& d, int64_t loA, int64_t loB, const rmgr_ssim_ThreadPool& tp)
{
    const uint32_t W = p.width, H = p.height;
    const uint32_t maxThreadCount = sizeof(void*) * 8;                               // the reference's cap (src/ssim.cpp:1025)
    const uint32_t threads = std::min<uint32_t>(tp.threadCount, maxThreadCount);
    PoolCall pc;
    pc.c = c; pc.host = &p; pc.d = d; pc.loA = loA; pc.loB = loB; pc.rc = 0; pc.ran = 0;
    memset(pc.done, 0, sizeof(pc.done));
    pc.whole = !bandable(p);
    const int bands = (W && H && !pc.whole) ? band_count(p) : 1;
    const uint32_t cell = ssim_hip::cell_rows_for(H);
    pc.band_rows = std::max<uint32_t>(((H + bands - 1) / bands + cell - 1) & ~(cell - 1), cell);
    pc.jobs = (W && H) ? (H + pc.band_rows - 1) / pc.band_rows : 0;                 // an empty image has no jobs (the reference dispatches its 0 tiles)
    PoolCall* self = &pc;
    void* args[sizeof(void*) * 8];
    for (uint32_t t = 0; t < threads; ++t) args[t] = &self;
    const int poolResult = tp.dispatch(tp.context, pool_job, args, threads, pc.jobs);
    // whatever the pool did, nothing of this call may still be queued when the staging buffers are handed on
    hipError_t e = hipStreamSynchronize(c->stream);
    if (c->out_stream && hipStreamSynchronize(c->out_stream) != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess) { (void)hipGetLastError(); return map_hip_error(e); }
    if (pc.rc && pc.rc != ECHILD) return pc.rc;                                      // a HIP call failed inside a job
    if (ssim == NULL) return 0;                                                      // src/ssim.cpp:1091: the pool's result is only looked at for the global value
    if (poolResult != 0 || pc.rc || pc.ran != pc.jobs) return ECHILD;                // src/ssim.cpp:1094-1097 (and a pool that ran fewer jobs than it was given)
    double sum = 0.0;
    if (pc.jobs) {
        const ssim_hip::Geometry geo = ssim_hip::plan(W, H, 1, c->mode, c->strip_rows, 0, c->cu_count, c->xcd_count);
        e = ssim_hip::launch_reduce(geo, c->partials, c->partials + geo.partials_per_image(), c->h_sums, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); return map_hip_error(e); }
        sum = c->h_sums[0];
    }
    *ssim = mean_of(sum, W, H);
    return 0;
}

} // namespace ssim_host

using namespace ssim_host;

extern "C" {

rmgr_int32_t rmgr_ssim_hip_get_plan(const rmgr_ssim_hip_Context* c, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count, rmgr_ssim_hip_Plan* plan) RMGR_NOEXCEPT
{
    if (!plan || plan->structSize < RMGR_SSIM_HIP_PLAN_MIN_SIZE) return EINVAL;
    const int mode = c ? c->mode : RMGR_SSIM_HIP_MODE_EXACT, cus = c ? c->cu_count : 256, xcds = c ? c->xcd_count : 8, rows = c ? c->strip_rows : 0;
    int variant = c ? c->variant : 0;
    if (variant == 0 && rows == 0) variant = ssim_hip::default_variant(width, height, count, mode, cus);    // as enqueue() does
    const ssim_hip::Geometry geo = ssim_hip::plan(width, height, count, mode, rows, variant, cus, xcds);
    rmgr_ssim_hip_Plan full;
    memset(&full, 0, sizeof(full));
    full.structSize = plan->structSize;
    full.stripWidth = geo.strip_w;
    full.stripRows = geo.strip_rows;
    full.stripsX = geo.strips_x;
    full.stripsY = geo.strips_y;
    full.wavefronts = geo.strips_x * geo.strips_y * count;
    full.waveSlots = geo.wave_slots;
    full.earlyRowSums = ssim_hip::uses_early_row_sums(geo, mode, variant) ? 1u : 0u;
    full.cellRows = geo.cell_rows;
    full.cellsX = geo.cells_x;
    full.cellsY = geo.cells_y;
    full.balancedChunks = geo.n_chunks;
    full.balancedChunkRows = geo.chunk_cells * geo.cell_rows;
    full.balancedInterleave = geo.n_chunks ? geo.bal_stride : 0u;
    memcpy(plan, &full, std::min<size_t>(plan->structSize, sizeof(full)));      // never beyond what the caller allocated
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_enqueue_batch(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_Params* params, double* sumsDevice) RMGR_NOEXCEPT
{
    if (!c || (count && (!params || !sumsDevice))) return EINVAL;
    if (count == 0) return 0;
    bool any_map = false;
    for (uint32_t i = 0; i < count; ++i) {
        if (params[i].imgA.topLeft == NULL || params[i].imgB.topLeft == NULL) return EINVAL;
        if (params[i].width != params[0].width || params[i].height != params[0].height) return EINVAL;
        any_map = any_map || params[i].ssimMap != NULL;
    }
    for (uint32_t i = 0; i < count; ++i)
        if (any_map && params[i].ssimMap == NULL) return EINVAL;   // all or none
    USE_DEVICE(c);
    // One launch covers up to 65535 pairs (grid.z); larger batches go out in consecutive launches.
    const uint32_t kMaxPerLaunch = 65535;
    const std::unique_ptr<PairDesc[]> descs(new (std::nothrow) PairDesc[std::min(kMaxPerLaunch, count)]);
    if (!descs) return ENOMEM;
    int rc = 0;
    for (uint32_t first = 0; first < count && rc == 0; first += kMaxPerLaunch) {
        const uint32_t n = std::min(kMaxPerLaunch, count - first);
        for (uint32_t i = 0; i < n; ++i) descs[i] = make_desc(params[first + i]);
        rc = enqueue(c, params[0].width, params[0].height, n, descs.get(), any_map, sumsDevice + first);
    }
    return rc;
}

rmgr_int32_t rmgr_ssim_hip_enqueue_rows(rmgr_ssim_hip_Context* c, const rmgr_ssim_Params* params, rmgr_uint32_t yBegin, rmgr_uint32_t yRows, double* cellsDevice) RMGR_NOEXCEPT
{
    if (!c || !params || !cellsDevice) return EINVAL;
    if (params->imgA.topLeft == NULL || params->imgB.topLeft == NULL) return EINVAL;
    const uint32_t W = params->width, H = params->height, cell = ssim_hip::cell_rows_for(H);
    if (yBegin > H) return EINVAL;
    if (yRows == 0 || yBegin == H) return 0;                                      // an empty band (split_rows gives ranks beyond the image's cell rows (H, H)): nothing to do, whatever its alignment
    if ((yBegin % cell) != 0) return EINVAL;                                      // bands start on reduction-cell boundaries ...
    const uint32_t yEnd = yRows >= H - yBegin ? H : yBegin + yRows;
    if (yEnd != H && (yEnd % cell) != 0) return EINVAL;                           // ... and end on one, or at the image's last row
    if (W == 0 || yEnd == yBegin) return 0;
    USE_DEVICE(c);
    const PairDesc d = make_desc(*params);
    return enqueue(c, W, H, 1, &d, d.map != NULL, NULL, yBegin, yEnd - yBegin, false, cellsDevice);
}

rmgr_int32_t rmgr_ssim_hip_reduce_cells(rmgr_ssim_hip_Context* c, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count,
                                        const double* cellsDevice, double* sumsDevice) RMGR_NOEXCEPT
{
    if (!c || (count && (!cellsDevice || !sumsDevice))) return EINVAL;
    if (count == 0) return 0;
    USE_DEVICE(c);
    const ssim_hip::Geometry geo = ssim_hip::plan(width, height, count, c->mode, c->strip_rows, c->variant, c->cu_count, c->xcd_count);
    int rc = c->partials.grow(ssim_hip::reduce_scratch_size(geo) + 1);     // the chunk sums of very large images
    if (rc) return rc;
    HIP_TRY(ssim_hip::launch_reduce(geo, cellsDevice, c->partials, sumsDevice, c->stream));
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim_batch_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_Params* params, float* ssim) RMGR_NOEXCEPT
{
    if (count && (!params || !ssim)) return EINVAL;
    if (count == 0) return 0;
    for (uint32_t i = 0; i < count; ++i) {
        if (params[i].imgA.topLeft == NULL || params[i].imgB.topLeft == NULL || params[i].ssimMap != NULL) return EINVAL;
        if (params[i].width != params[0].width || params[i].height != params[0].height) return EINVAL;
    }
    int rc = 0;
    Lease lease;
    if ((rc = lease.take(c))) return rc;
    c = lease.c;
    USE_DEVICE(c);
    const uint32_t W = params[0].width, H = params[0].height;
    if (W == 0 || H == 0) {                       // 0/0, like the single call
        for (uint32_t i = 0; i < count; ++i) ssim[i] = mean_of(0.0, W, H);
        return 0;
    }
    HIP_TRY(c->copy_stream.ensure());
    for (int i = 0; i < 2; ++i) { HIP_TRY(c->slot_copied[i].ensure()); HIP_TRY(c->slot_done[i].ensure()); }
    if ((rc = c->batch_sums.grow(count))) return rc;
    if ((rc = c->h_sums.grow(count))) return rc;

    const size_t kChunkBytes = size_t(48) << 20, kAlign = 256;
    const uint32_t kMaxChunkPairs = 4096;
    const std::unique_ptr<PairDesc[]> descs(new (std::nothrow) PairDesc[std::min(count, kMaxChunkPairs)]);
    if (!descs) return ENOMEM;

    bool slot_busy[2] = {false, false};
    uint32_t first = 0;
    for (int k = 0; first < count; ++k) {
        const int slot = k & 1;
        // this chunk: as many pairs as fit the byte budget (at least one)
        uint32_t n = 0;
        size_t bytes = 0;
        bool small = true;
        while (first + n < count && n < kMaxChunkPairs) {
            const ByteRange a(params[first + n].imgA, W, H, kAlign), b(params[first + n].imgB, W, H, kAlign);
            if (n > 0 && bytes + a.padded + b.padded > kChunkBytes) break;
            bytes += a.padded + b.padded;
            small = small && (a.size + b.size <= kSmallStageBytes);
            ++n;
        }
        // the slot's previous occupant (chunk k-2) must have been consumed
        if (slot_busy[slot]) HIP_TRY(hipEventSynchronize(c->slot_done[slot]));
        if ((rc = c->slot_dev[slot].grow(bytes))) return rc;
        if (small && (rc = c->slot_pin[slot].grow(bytes))) return rc;
        size_t off = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const rmgr_ssim_Params& p = params[first + i];
            rmgr_ssim_Params dev = p;
            const rmgr_ssim_ImgParams* src[2] = {&p.imgA, &p.imgB};
            rmgr_ssim_ImgParams* dst[2] = {&dev.imgA, &dev.imgB};
            for (int j = 0; j < 2; ++j) {
                const ByteRange r(*src[j], W, H, kAlign);
                if (small) r.to_host(c->slot_pin[slot] + off);
                else HIP_TRY(r.to_device(c->slot_dev[slot] + off, c->copy_stream));
                dst[j]->topLeft = c->slot_dev[slot] + off - r.lo;
                off += r.padded;
            }
            descs[i] = make_desc(dev);
        }
        if (small) HIP_TRY(hipMemcpyAsync(c->slot_dev[slot], c->slot_pin[slot], bytes, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(hipEventRecord(c->slot_copied[slot], c->copy_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->slot_copied[slot], 0));
        if ((rc = enqueue(c, W, H, n, descs.get(), false, c->batch_sums + first))) return rc;
        HIP_TRY(hipEventRecord(c->slot_done[slot], c->stream));
        slot_busy[slot] = true;
        first += n;
    }
    HIP_TRY(hipMemcpyAsync(c->h_sums, c->batch_sums, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < count; ++i) ssim[i] = mean_of(c->h_sums[i], W, H);
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_finalize(rmgr_uint32_t count, const double* sums, rmgr_uint32_t width, rmgr_uint32_t height, float* ssim) RMGR_NOEXCEPT
{
    if (count && (!sums || !ssim)) return EINVAL;
    for (uint32_t i = 0; i < count; ++i) ssim[i] = mean_of(sums[i], width, height);
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_synchronize(rmgr_ssim_hip_Context* c) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    if (!c->collectives.empty()) return comm_bounded_sync(c);      // an all-reduce is queued: its peers might never arrive
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim_device(rmgr_ssim_hip_Context* c, float* ssim, const rmgr_ssim_Params* params) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    int rc = validate(ssim, params, NULL);
    if (rc) return rc;
    USE_DEVICE(c);
    // The reduction kernel stores the sum straight into pinned host memory (mapped into the device's address
    // space): no device-to-host copy call on the latency path, just the stream synchronisation.
    if ((rc = c->h_sums.grow(1))) return rc;
    const PairDesc d = make_desc(*params);
    if ((rc = enqueue(c, params->width, params->height, 1, &d, d.map != NULL, c->h_sums))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ssim)
        *ssim = mean_of(c->h_sums[0], params->width, params->height);
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim_host(rmgr_ssim_hip_Context* c, float* ssim, const rmgr_ssim_Params* params,
                                             const rmgr_ssim_ThreadPool* threadPool) RMGR_NOEXCEPT
{
    int rc = validate(ssim, params, threadPool);
    if (rc) return rc;
    Lease lease;                         // ctx == NULL: one of the default contexts, for this call only (concurrent callers overlap)
    if ((rc = lease.take(c))) return rc;
    c = lease.c;
    USE_DEVICE(c);
    const uint32_t W = params->width, H = params->height;

    // The reference allocates its tile scratch through params->alloc exactly once and fails with
    // ENOMEM when that returns NULL (src/ssim.cpp:1048-1052).  The GPU path has no use for host
    // scratch, but the contract is kept observable: one 64-byte allocation, released before returning.
    void* user_mem = NULL;
    if (params->alloc != NULL) {
        user_mem = params->alloc(64, 64);        // nothing else needs host scratch: staging is pinned memory owned by the context
        if (user_mem == NULL) return ENOMEM;
    }
    const auto release = [params](void* m) { if (params->dealloc) params->dealloc(m); };
    const std::unique_ptr<void, decltype(release)> user_mem_owner(user_mem, release);

    rmgr_ssim_Params dev = *params;
    const bool pooled = threadPool != NULL && threadPool->dispatch != NULL;
    bool staged = true;                  // false: the large-image copies are still to be issued
    ByteRange a, b;
    if (W && H) {
        // Stage the byte range each image occupies; step/stride semantics carry over unchanged.
        a = ByteRange(params->imgA, W, H, 64);
        b = ByteRange(params->imgB, W, H, 64);
        if (a.size + b.size <= kSmallStageBytes) {
            // Small images: two pageable copies cost ~12 us each in driver overhead.  Gather both byte ranges in
            // one pinned buffer (a ~4 us memcpy at this size) and send them with a single DMA.
            if ((rc = c->h_stage.grow(a.padded + b.size))) return rc;
            if ((rc = c->stage_a.grow(a.padded + b.size))) return rc;
            if (!pooled) {                    // with the caller's thread pool the images are sent by its jobs (compute_via_pool())
                a.to_host(c->h_stage);
                b.to_host(c->h_stage + a.padded);
                HIP_TRY(hipMemcpyAsync(c->stage_a, c->h_stage, a.padded + b.size, hipMemcpyHostToDevice, c->stream));
            }
            dev.imgA.topLeft = c->stage_a - a.lo;
            dev.imgB.topLeft = c->stage_a + a.padded - b.lo;
        } else {
            if ((rc = c->stage_a.grow(a.size))) return rc;
            if ((rc = c->stage_b.grow(b.size))) return rc;
            dev.imgA.topLeft = c->stage_a - a.lo;
            dev.imgB.topLeft = c->stage_b - b.lo;
            staged = false;                   // copied below: in one piece, or band by band
        }
        if (params->ssimMap) {
            if ((rc = c->stage_map.grow((size_t)W * H))) return rc;
            dev.ssimMap = c->stage_map;      // dense W x H on the device
            dev.ssimStep = 1;
            dev.ssimStride = W;
        }
    } else {
        dev.ssimMap = NULL;
    }

    if ((rc = c->h_sums.grow(1))) return rc;
    const PairDesc d = make_desc(dev);

    // A large pair whose map is wanted moves 2 B/px in and 4 B/px out over PCIe; the link is full duplex and the
    // 0.1 ms kernel is nothing next to either.  The image is therefore cut into row bands: band k+1 is copied in
    // while band k is computed (a row window of the same launch geometry; the cell-based reduction makes the sum
    // bit-identical to the one-launch result) and band k-1's map rows travel back, written by a helper thread
    // straight into the caller's buffer.
    // Without a map a few bands hide the kernel behind the copy, which pays only for very large images (compute_banded()).
    // An explicit $RMGR_SSIM_HIP_BANDS always takes the banded path (so that a band sweep measures what it says it does).
    const bool bands_forced = getenv("RMGR_SSIM_HIP_BANDS") != NULL;
    if (pooled)           // the caller brought a thread pool: its dispatch function runs the row-band jobs
        return compute_via_pool(c, ssim, *params, d, a.lo, b.lo, *threadPool);
    if (!staged && bandable(*params) && (params->ssimMap || bands_forced || (uint64_t)W * H >= (uint64_t(1) << 26))) {
        if ((rc = compute_banded(c, *params, d, a.lo, b.lo))) return rc;
    } else {
        if (!staged) {
            HIP_TRY(a.to_device(c->stage_a, c->stream));
            HIP_TRY(b.to_device(c->stage_b, c->stream));
        }
        if ((rc = enqueue(c, W, H, 1, &d, d.map != NULL, c->h_sums))) return rc;      // sum lands in pinned host memory
        if (params->ssimMap && W && H) {
            if ((rc = map_rows_to_host(c, *params, 0, H, c->stream))) return rc;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (ssim)
        *ssim = mean_of(c->h_sums[0], W, H);
    return 0;
}

// ---- multi-scale SSIM (rmgr_ssim_hip_compute_msssim_*) ------------------------------------------------------------------------------------------
// The definition is in include/rmgr/ssim-hip.h, the kernels in msssim_kernels.hip.  A batch runs in sub-batches whose device scratch (pyramid,
// tile partials and, for host pointers, the staged images) stays under kMsScratchCap; every image's statistics are summed over fixed tiles in a
// fixed order, so the split changes nothing in the results.
namespace {

const uint64_t kMsScratchCap = uint64_t(1) << 30;

// Every check of the two entry points, before any device is touched.
int msssim_validate(rmgr_uint32_t count, const rmgr_ssim_Params* params, rmgr_uint32_t scales, const double* weights, const float* msssim)
{
    if (count == 0 || params == NULL || msssim == NULL) return EINVAL;
    if (scales < 1 || scales > RMGR_SSIM_HIP_MSSSIM_MAX_SCALES) return EINVAL;
    if (weights == NULL) {
        if (scales != 5) return EINVAL;
    } else {
        for (uint32_t s = 0; s < scales; ++s)
            if (!std::isfinite(weights[s]) || weights[s] < 0.0) return EINVAL;
    }
    const uint32_t W = params[0].width, H = params[0].height;
    if (W == 0 || H == 0) return EINVAL;
    for (uint32_t i = 0; i < count; ++i) {
        const rmgr_ssim_Params& p = params[i];
        if (p.width != W || p.height != H) return EINVAL;
        if (p.imgA.topLeft == NULL || p.imgB.topLeft == NULL || p.ssimMap != NULL) return EINVAL;
    }
    if (ssim_hip::msssim_max_count(W, H, scales) == 0) return EINVAL;      // one pair beyond a launch grid (tens of gigapixels)
    return 0;
}

// prod_{s < M-1} max(mcs_s, 0)^w_s * max(mssim_{M-1}, 0)^w_{M-1}, in double; means = [scale]{mcs, mssim}
float msssim_combine(const double* means, uint32_t scales, const double* w)
{
    double r = 1.0;
    for (uint32_t s = 0; s < scales; ++s) {
        const double v = means[2 * s + (s + 1 == scales ? 1 : 0)];
        r *= std::pow(v > 0.0 ? v : 0.0, w[s]);
    }
    return (float)r;
}

// n pairs (device descriptors in d) -> their n x scales x 2 means.  Blocks.
int msssim_run(rmgr_ssim_hip_Context* c, uint32_t n, const PairDesc* d, uint32_t W, uint32_t H, uint32_t scales, double* means)
{
    int rc;
    const size_t ns = (size_t)n * scales * 2;
    if ((rc = c->ms_desc_pin.grow(n))) return rc;
    if ((rc = c->ms_desc.grow(n))) return rc;
    if ((rc = c->ms_scratch.grow(ssim_hip::msssim_scratch_bytes(W, H, n, scales)))) return rc;
    if ((rc = c->ms_sums.grow(ns))) return rc;
    if ((rc = c->ms_sums_pin.grow(ns))) return rc;
    memcpy(c->ms_desc_pin, d, n * sizeof(PairDesc));
    HIP_TRY(hipMemcpyAsync(c->ms_desc, c->ms_desc_pin, n * sizeof(PairDesc), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(ssim_hip::launch_msssim(c->ms_desc, n, W, H, scales, c->ms_scratch, c->ms_sums, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ms_sums_pin, c->ms_sums, ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t s = 0; s < scales; ++s) {
        const double px = (double)ssim_hip::ms_dim(W, s) * (double)ssim_hip::ms_dim(H, s);
        for (uint32_t i = 0; i < n; ++i)
            for (int k = 0; k < 2; ++k) means[((size_t)i * scales + s) * 2 + k] = c->ms_sums_pin[((size_t)i * scales + s) * 2 + k] / px;
    }
    return 0;
}

// The whole batch, sub-batch by sub-batch; stage: the images are host memory, copied (plain copies of each image's byte range) into c->stage_a first.
int msssim_batches(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_Params* params, uint32_t scales, const double* w,
                   float* msssim, double* scaleMeans, bool stage)
{
    const uint32_t W = params[0].width, H = params[0].height;
    const uint64_t per = ssim_hip::msssim_scratch_bytes(W, H, 1, scales);
    const uint32_t nmax = (uint32_t)std::min<uint64_t>(ssim_hip::msssim_max_count(W, H, scales), std::max<uint64_t>(1, kMsScratchCap / per));
    try {
        std::vector<PairDesc> d;
        std::vector<double> means;
        for (uint32_t i0 = 0; i0 < count;) {
            uint32_t n = 0;
            uint64_t staged = 0;
            while (i0 + n < count && n < nmax) {
                const uint64_t bytes = stage ? ByteRange(params[i0 + n].imgA, W, H, 64).padded + ByteRange(params[i0 + n].imgB, W, H, 64).padded : 0;
                if (n > 0 && per * (n + 1) + staged + bytes > kMsScratchCap) break;
                staged += bytes;
                ++n;
            }
            d.resize(n);
            int rc;
            if (stage && (rc = c->stage_a.grow((size_t)staged))) return rc;
            size_t off = 0;                      // stage: where the next image's byte range goes in c->stage_a
            for (uint32_t i = 0; i < n; ++i) {
                rmgr_ssim_Params p = params[i0 + i];
                p.ssimMap = NULL;
                for (int k = 0; k < 2 && stage; ++k) {
                    rmgr_ssim_ImgParams& im = k ? p.imgB : p.imgA;
                    const ByteRange r(im, W, H, 64);
                    HIP_TRY(r.to_device(c->stage_a + off, c->stream));
                    im.topLeft = c->stage_a + off - r.lo;
                    off += r.padded;
                }
                d[i] = make_desc(p);
            }
            means.resize((size_t)n * scales * 2);
            if ((rc = msssim_run(c, n, &d[0], W, H, scales, &means[0]))) return rc;
            for (uint32_t i = 0; i < n; ++i) {
                msssim[i0 + i] = msssim_combine(&means[(size_t)i * scales * 2], scales, w);
                if (scaleMeans) memcpy(scaleMeans + (size_t)(i0 + i) * scales * 2, &means[(size_t)i * scales * 2], scales * 2 * sizeof(double));
            }
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    return 0;
}

} // namespace

rmgr_int32_t rmgr_ssim_hip_compute_msssim_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_Params* params,
                                                 rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    int rc = msssim_validate(count, params, scales, weights, msssim);
    if (rc) return rc;
    USE_DEVICE(c);
    return msssim_batches(c, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, false);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_Params* params,
                                               rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    int rc = msssim_validate(count, params, scales, weights, msssim);
    if (rc) return rc;
    Lease lease;                         // ctx == NULL: one of the default contexts, for this call only
    if ((rc = lease.take(c))) return rc;
    c = lease.c;
    USE_DEVICE(c);
    return msssim_batches(c, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, true);
}

// ---- one process, several devices ------------------------------------------------------------------------------------
// The reference parallelises one call over a caller-supplied thread pool (tile jobs, src/ssim.cpp:1048-1088; the OpenMP
// adapter src/ssim-openmp.c:26-47).  The batch-level counterpart here: a contiguous block of the pairs per device, one
// worker thread and one cached engine context per device slot, every block through the pipelined host-batch path above.
// Pairs are independent and every ssim[i] is written by exactly one worker, so there is no exchange step at all in one
// address space (the RCCL all-reduce exists for the one-process-per-GPU form, rmgr_ssim_hip_comm_*), and ssim[i] is
// bit-identical to the single-device call for any device list.
namespace {
std::mutex g_slots_lock;
std::vector<std::pair<int, rmgr_ssim_hip_Context*> > g_slots;     // (device, context) per slot of the last device lists; never freed
std::mutex g_multi_lock;                                          // one multi-device call at a time (the slots are shared)

rmgr_ssim_hip_Context* slot_context(size_t slot, int device, int* err)
{
    std::lock_guard<std::mutex> guard(g_slots_lock);
    try {
        if (g_slots.size() <= slot) g_slots.resize(slot + 1, std::make_pair(-1, (rmgr_ssim_hip_Context*)NULL));
    } catch (...) { *err = ENOMEM; return NULL; }
    if (g_slots[slot].second && g_slots[slot].first != device) {     // the slot served another device last time
        rmgr_ssim_hip_destroy(g_slots[slot].second);
        g_slots[slot].second = NULL;
    }
    if (!g_slots[slot].second) {
        *err = rmgr_ssim_hip_create(&g_slots[slot].second, device, NULL);
        if (*err) { g_slots[slot].second = NULL; return NULL; }
        g_slots[slot].first = device;
    }
    return g_slots[slot].second;
}
} // namespace

extern "C" rmgr_int32_t rmgr_ssim_hip_compute_ssim_batch_host_devices(const rmgr_int32_t* devices, rmgr_uint32_t deviceCount, rmgr_int32_t mode,
                                                                      rmgr_uint32_t count, const rmgr_ssim_Params* params, float* ssim) RMGR_NOEXCEPT
{
    if (count && (!params || !ssim)) return EINVAL;
    if (mode < RMGR_SSIM_HIP_MODE_EXACT || mode > RMGR_SSIM_HIP_MODE_SEPARABLE) return EINVAL;
    if (devices && deviceCount == 0) return EINVAL;
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess) { (void)hipGetLastError(); visible = 0; }
    if (visible <= 0) return ENODEV;
    std::vector<int> devs;
    try {
        if (devices) devs.assign(devices, devices + deviceCount);
        else for (int d = 0; d < visible; ++d) devs.push_back(d);
    } catch (...) { return ENOMEM; }
    for (size_t k = 0; k < devs.size(); ++k)
        if (devs[k] < 0 || devs[k] >= visible) return EINVAL;
    if (count == 0) return 0;
    std::lock_guard<std::mutex> one_call(g_multi_lock);
    const size_t n = std::min<size_t>(devs.size(), count);          // no more workers than pairs
    // contiguous blocks, the first count % n slots one pair longer (ssim_amd/sharding.py split_batch)
    std::vector<int> rcs;
    std::vector<std::thread> workers;
    try { rcs.assign(n, 0); workers.reserve(n); } catch (...) { return ENOMEM; }
    struct Job {
        static void run(size_t slot, int device, int mode, uint32_t first, uint32_t cnt, const rmgr_ssim_Params* params, float* ssim, int* rc)
        {
            rmgr_ssim_hip_Context* c = slot_context(slot, device, rc);
            if (!c) return;
            if ((*rc = rmgr_ssim_hip_set_mode(c, mode))) return;
            *rc = rmgr_ssim_hip_compute_ssim_batch_host(c, cnt, params + first, ssim + first);
        }
    };
    const uint32_t base = (uint32_t)(count / n), extra = (uint32_t)(count % n);
    uint32_t first = 0;
    int launch_rc = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint32_t cnt = base + (k < extra ? 1u : 0u);
        if (k + 1 == n) {
            Job::run(k, devs[k], mode, first, cnt, params, ssim, &rcs[k]);          // the calling thread takes the last block
        } else {
            try { workers.push_back(std::thread(Job::run, k, devs[k], (int)mode, first, cnt, params, ssim, &rcs[k])); }
            catch (...) { launch_rc = EAGAIN; break; }
        }
        first += cnt;
    }
    for (size_t k = 0; k < workers.size(); ++k) workers[k].join();
    if (launch_rc) return launch_rc;
    for (size_t k = 0; k < n; ++k)
        if (rcs[k]) return rcs[k];
    return 0;
}

} // extern "C"

namespace {

struct StagedPair {
    rmgr_ssim_hip_Context* c;
    Lease lease;
    DeviceGuard device;           // the context's device stays current for as long as the staged pair lives, i.e. for the WHOLE
                                  // entry point: its later allocations, events and launches must not land on the caller's device
    uint8_t* a; uint8_t* b;       // device copies of the two interleaved images, rows `pitch` bytes apart
    size_t pitch;
};

// Shared front half of the multi-channel entry points: context, validation, one H2D copy per image.
int stage_interleaved(rmgr_ssim_hip_Context* c, StagedPair& sp, const void* out1, const void* out2,
                      const uint8_t* imgA, ptrdiff_t strideA, const uint8_t* imgB, ptrdiff_t strideB,
                      uint32_t width, uint32_t height, uint32_t channels)
{
    if ((out1 == NULL && out2 == NULL) || imgA == NULL || imgB == NULL || channels == 0) return EINVAL;
    int rc = 0;
    if ((rc = sp.lease.take(c))) return rc;
    c = sp.lease.c;
    sp.c = c;
    if ((rc = sp.device.enter(c->device))) return rc;
    sp.pitch = ((size_t)width * channels + 3) & ~(size_t)3;      // dword-aligned rows for the packed luminance path
    const size_t bytes = sp.pitch * height + 4;
    if ((rc = c->stage_a.grow(bytes))) return rc;
    if ((rc = c->stage_b.grow(bytes))) return rc;
    sp.a = c->stage_a; sp.b = c->stage_b;
    if (width && height) {
        // rows may be stored bottom-up (negative stride): copy row 0 first either way
        HIP_TRY(hipMemcpy2DAsync(sp.a, sp.pitch, strideA >= 0 ? imgA : imgA + (ptrdiff_t)(height - 1) * strideA, (size_t)(strideA >= 0 ? strideA : -strideA),
                                 (size_t)width * channels, height, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpy2DAsync(sp.b, sp.pitch, strideB >= 0 ? imgB : imgB + (ptrdiff_t)(height - 1) * strideB, (size_t)(strideB >= 0 ? strideB : -strideB),
                                 (size_t)width * channels, height, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

// A plane of a staged image for a PairDesc: the copy at `copy` holds the rows `pitch` apart in the order they were copied (row 0 of a
// bottom-up image last).
void staged_plane(const uint8_t* copy, size_t pitch, uint32_t height, bool bottom_up, const uint8_t*& row0, int64_t& stride)
{
    row0 = bottom_up ? copy + (size_t)(height ? height - 1 : 0) * pitch : copy;
    stride = bottom_up ? -(int64_t)pitch : (int64_t)pitch;
}

} // namespace

extern "C" rmgr_int32_t rmgr_ssim_hip_luminance_device(rmgr_ssim_hip_Context* c, rmgr_uint8_t* dstY, ptrdiff_t dstStride,
                                                       const rmgr_uint8_t* src, ptrdiff_t srcStep, ptrdiff_t srcStride,
                                                       rmgr_uint32_t width, rmgr_uint32_t height) RMGR_NOEXCEPT
{
    if (!c || !dstY || !src || srcStep < 3) return EINVAL;
    USE_DEVICE(c);
    HIP_TRY(ssim_hip::launch_luminance(dstY, dstStride, src, srcStep, srcStride, width, height, c->stream));
    return 0;
}

extern "C" rmgr_int32_t rmgr_ssim_hip_compute_ssim_channels_host(rmgr_ssim_hip_Context* ctx, float* ssim,
                                                                 const rmgr_uint8_t* imgA, ptrdiff_t strideA, const rmgr_uint8_t* imgB, ptrdiff_t strideB,
                                                                 rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t channels, float* ssimMap) RMGR_NOEXCEPT
{
    StagedPair sp;
    int rc = stage_interleaved(ctx, sp, ssim, ssimMap, imgA, strideA, imgB, strideB, width, height, channels);
    if (rc) return rc;
    rmgr_ssim_hip_Context* c = sp.c;
    const bool bottomA = strideA < 0, bottomB = strideB < 0;
    const size_t mapFloats = (size_t)width * height * channels;
    if (ssimMap && mapFloats && (rc = c->stage_map.grow(mapFloats))) return rc;
    if ((rc = c->h_sums.grow(channels))) return rc;
    const std::unique_ptr<PairDesc[]> descs(new (std::nothrow) PairDesc[channels]);
    if (!descs) return ENOMEM;
    for (uint32_t ch = 0; ch < channels; ++ch) {
        PairDesc& d = descs[ch];
        staged_plane(sp.a + ch, sp.pitch, height, bottomA, d.a, d.a_stride); d.a_step = channels;
        staged_plane(sp.b + ch, sp.pitch, height, bottomB, d.b, d.b_stride); d.b_step = channels;
        d.map = (ssimMap && mapFloats) ? c->stage_map + ch : NULL;
        d.map_step = d.map ? channels : 0;
        d.map_stride = d.map ? (int64_t)width * channels : 0;
    }
    if ((rc = enqueue(c, width, height, channels, descs.get(), ssimMap != NULL && mapFloats, c->h_sums))) return rc;
    if (ssimMap && mapFloats)
        HIP_TRY(hipMemcpyAsync(ssimMap, c->stage_map, sizeof(float) * mapFloats, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ssim)
        for (uint32_t ch = 0; ch < channels; ++ch) ssim[ch] = mean_of(c->h_sums[ch], width, height);
    return 0;
}

extern "C" rmgr_int32_t rmgr_ssim_hip_compute_ssim_luminance_host(rmgr_ssim_hip_Context* ctx, float* ssim,
                                                                  const rmgr_uint8_t* imgA, ptrdiff_t strideA, const rmgr_uint8_t* imgB, ptrdiff_t strideB,
                                                                  rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t channels, float* ssimMap) RMGR_NOEXCEPT
{
    if (channels < 3) return EINVAL;
    StagedPair sp;
    int rc = stage_interleaved(ctx, sp, ssim, ssimMap, imgA, strideA, imgB, strideB, width, height, channels);
    if (rc) return rc;
    rmgr_ssim_hip_Context* c = sp.c;
    // the Y planes live behind the staged RGB data of each image (rows in copy order: flip if bottom-up)
    const size_t ypitch = ((size_t)width + 3) & ~(size_t)3;
    const size_t yBytes = ypitch * height + 4;
    // grow WITHOUT losing the staged pixels: allocate the Y planes separately in the map staging area
    const size_t mapFloats = (size_t)width * height;
    const size_t needFloats = (ssimMap ? mapFloats : 0) + (2 * yBytes + 3) / 4 + 4;
    if ((rc = c->stage_map.grow(needFloats))) return rc;
    uint8_t* ya = reinterpret_cast<uint8_t*>(c->stage_map + (ssimMap ? mapFloats : 0));
    ya += (4 - (reinterpret_cast<uintptr_t>(ya) & 3u)) & 3u;
    uint8_t* yb = ya + yBytes;
    yb += (4 - (reinterpret_cast<uintptr_t>(yb) & 3u)) & 3u;
    HIP_TRY(ssim_hip::launch_luminance(ya, (int64_t)ypitch, sp.a, channels, (int64_t)sp.pitch, width, height, c->stream));
    HIP_TRY(ssim_hip::launch_luminance(yb, (int64_t)ypitch, sp.b, channels, (int64_t)sp.pitch, width, height, c->stream));
    if ((rc = c->h_sums.grow(1))) return rc;
    PairDesc d;
    staged_plane(ya, ypitch, height, strideA < 0, d.a, d.a_stride); d.a_step = 1;
    staged_plane(yb, ypitch, height, strideB < 0, d.b, d.b_stride); d.b_step = 1;
    d.map = (ssimMap && mapFloats) ? c->stage_map : NULL;
    d.map_step = d.map ? 1 : 0;
    d.map_stride = d.map ? width : 0;
    if ((rc = enqueue(c, width, height, 1, &d, d.map != NULL, c->h_sums))) return rc;
    if (d.map)
        HIP_TRY(hipMemcpyAsync(ssimMap, c->stage_map, sizeof(float) * mapFloats, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ssim) *ssim = mean_of(c->h_sums[0], width, height);
    return 0;
}
