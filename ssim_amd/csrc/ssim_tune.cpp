// ssim_tune.cpp -- profiling and tuning entry points of the C ABI: kernel timing and shader clock read-out, rmgr_ssim_hip_tune and the
// tuned table, the VALU probe, synthetic pairs.
#include "ssim_context.h"

using namespace ssim_host;

namespace {

// The per-XCD clock counters (ssim_kernels.hip clock_begin): mean and lowest shader clock over the XCDs that reported, and the launches counted (per XCD, the most any saw).
void clocks_from(const uint64_t* v, int xcds, int wall_clock_khz, double* mean_mhz, double* min_mhz, rmgr_uint64_t* launches)
{
    double sum = 0.0, lo = 0.0;
    int n = 0;
    uint64_t most = 0;
    for (int x = 0; x < xcds && x < (int)ssim_hip::kClockMaxXcds; ++x) {
        const uint64_t* c = v + ssim_hip::kClockStride * x;
        if (c[3] == 0) continue;
        const double mhz = (double)c[2] / (double)c[3] * (double)wall_clock_khz / 1000.0;
        sum += mhz;
        lo = n == 0 ? mhz : std::min(lo, mhz);
        most = std::max(most, c[4]);
        ++n;
    }
    if (mean_mhz) *mean_mhz = n ? sum / n : 0.0;
    if (min_mhz) *min_mhz = lo;
    if (launches) *launches = most;
}

// Reads and clears the clock counters the profiled launches added to (after the stream is idle).
int read_clock(rmgr_ssim_hip_Context* c, double* mhz, double* min_mhz, rmgr_uint64_t* launches)
{
    if (mhz) *mhz = 0.0;
    if (min_mhz) *min_mhz = 0.0;
    if (launches) *launches = 0;
    if (!c->clock_dev) return 0;
    uint64_t v[ssim_hip::kClockWords];
    HIP_TRY(hipMemcpyAsync(v, c->clock_dev, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->clock_dev, 0, sizeof(v), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    clocks_from(v, c->xcd_count, c->wall_clock_khz, mhz, min_mhz, launches);
    return 0;
}

struct TuneCandidate { int variant, rows; double ms; uint64_t key; };

// The tuner's synthetic pairs: device memory owned for the length of the call.
struct HipFree { void operator()(void* p) const { (void)hipFree(p); (void)hipGetLastError(); } };
template <typename T> int device_alloc(std::unique_ptr<T, HipFree>& m, size_t n)
{
    void* p = NULL;
    HIP_TRY(hipMalloc(&p, n * sizeof(T)));
    m.reset(static_cast<T*>(p));
    return 0;
}

uint64_t plan_key(const ssim_hip::Geometry& g, bool early, int one_column)
{
    uint64_t k = g.strip_w;
    k = k * 1000003u + g.strip_rows; k = k * 1000003u + g.n_chunks; k = k * 1000003u + g.chunk_cells; k = k * 1000003u + g.bal_stride;
    return (k * 4 + (early ? 1 : 0)) * 2 + (uint64_t)one_column;
}

} // namespace

extern "C" {

rmgr_int32_t rmgr_ssim_hip_set_tuning(rmgr_ssim_hip_Context* c, rmgr_int32_t stripRows, rmgr_int32_t variant) RMGR_NOEXCEPT
{
    if (!c || stripRows < 0 || variant < 0) return EINVAL;
    c->strip_rows = stripRows;
    c->variant = variant;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_set_profiling(rmgr_ssim_hip_Context* c, rmgr_int32_t enabled) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    if (enabled && !c->clock_dev) {
        USE_DEVICE(c);
        int rc = c->clock_dev.grow(ssim_hip::kClockWords);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(c->clock_dev, 0, ssim_hip::kClockWords * sizeof(uint64_t), c->stream));
    }
    c->profiling = enabled != 0;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_get_profile_clock(rmgr_ssim_hip_Context* c, double* shaderMHz, double* slowestXcdMHz, rmgr_uint64_t* launches) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return read_clock(c, shaderMHz, slowestXcdMHz, launches);
}

rmgr_int32_t rmgr_ssim_hip_get_profile(rmgr_ssim_hip_Context* c, rmgr_uint64_t* launches, double* kernelMs) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    int rc = drain_profile(c);
    if (rc) return rc;
    if (launches) *launches = c->prof_launches;
    if (kernelMs) *kernelMs = c->prof_ms;
    c->prof_launches = 0;
    c->prof_ms = 0.0;
    return 0;
}

// ---- rmgr_ssim_hip_tune: the plan for one launch shape, MEASURED on the device the context runs on ---------------------------------------------
// plan()'s default is a model fitted on 256-CU boxes that differ by +-4 % (strip height by a packing model, EARLY by launch length, the balanced
// schedule by a priced rule); this times the handful of candidates that model chooses between -- on THIS device, at THIS clock -- and keeps the
// winner for later launches of the shape.  Candidates: the default; the two-column strips at the default height with the row sums in the blur
// phase / EARLY; the default kernel at half and at twice the strip height; the balanced schedule (no map; modes 0, 3, 1); the one-column kernel for
// small launches.  Every candidate gives the same bits (cells at absolute positions, fixed-order reduction): only time is at stake.
rmgr_int32_t rmgr_ssim_hip_tune(rmgr_ssim_hip_Context* c, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count, rmgr_int32_t withMap,
                                rmgr_ssim_hip_TuneResult* result) RMGR_NOEXCEPT
{
    if (!c || width == 0 || height == 0 || count == 0 || count > 65535u) return EINVAL;
    if (result && result->structSize < RMGR_SSIM_HIP_TUNE_RESULT_MIN_SIZE) return EINVAL;
    USE_DEVICE(c);
    const bool map = withMap != 0;
    const int mode = c->mode;
    // forget an earlier choice for this shape: the default candidate must run the default
    if (const rmgr_ssim_hip_Context_::Tuned* t = c->tuned_for(width, height, count, map)) c->tuned.erase(c->tuned.begin() + (t - c->tuned.data()));

    // candidates, de-duplicated by the launch they produce
    const int v0 = ssim_hip::default_variant(width, height, count, mode, c->cu_count);
    const ssim_hip::Geometry g0 = ssim_hip::plan(width, height, count, mode, 0, v0, c->cu_count, c->xcd_count);
    const uint32_t cell = g0.cell_rows, R = g0.strip_rows;
    std::vector<TuneCandidate> cand;
    std::vector<std::vector<double> > samples;      // per candidate: its per-round means
    try {
        struct Add {
            static void one(std::vector<TuneCandidate>& list, rmgr_ssim_hip_Context* c, uint32_t w, uint32_t h, uint32_t n, bool map, int variant, int rows)
            {
                int v = variant;
                if (v == 0 && rows == 0) v = ssim_hip::default_variant(w, h, n, c->mode, c->cu_count);
                ssim_hip::Geometry g = ssim_hip::plan(w, h, n, c->mode, rows, v, c->cu_count, c->xcd_count);
                if (map) { g.chunk_cells = 0; g.n_chunks = 0; g.bal_stride = 1; }                   // launches with a map run the strips
                if (ssim_hip::is_balanced_variant(variant) && g.n_chunks == 0) return;             // no balanced form for this launch
                const bool one = c->mode == RMGR_SSIM_HIP_MODE_DOUBLE || v == 1;
                const TuneCandidate t = {variant, rows, 0.0, plan_key(g, g.n_chunks ? true : ssim_hip::uses_early_row_sums(g, c->mode, v), one ? 1 : 0)};
                for (size_t i = 0; i < list.size(); ++i) if (list[i].key == t.key) return;
                list.push_back(t);
            }
        };
        Add::one(cand, c, width, height, count, map, 0, 0);                                        // the default, first
        if (mode != RMGR_SSIM_HIP_MODE_DOUBLE) {
            Add::one(cand, c, width, height, count, map, 2, (int)R);
            if (mode == RMGR_SSIM_HIP_MODE_EXACT || mode == RMGR_SSIM_HIP_MODE_UNFUSED) Add::one(cand, c, width, height, count, map, 3, (int)R);
            if (!map) Add::one(cand, c, width, height, count, map, 6, 0);
            if ((uint64_t)width * height * count <= (uint64_t(1) << 22)) Add::one(cand, c, width, height, count, map, 1, 0);
        }
        const uint32_t half = std::max(cell, ((R / 2) + cell - 1) & ~(cell - 1)), twice = std::min<uint32_t>(2 * R, (height + cell - 1) & ~(cell - 1));
        const int keep = (mode == RMGR_SSIM_HIP_MODE_DOUBLE) ? 0 : (g0.strip_w == 64 ? 1 : ssim_hip::uses_early_row_sums(g0, mode, v0) ? 3 : 2);
        if (!map && g0.n_chunks == 0) {            // where the chunks would divide the strip column evenly, the strips at the chunk height: the same partition without the segment loop
            const ssim_hip::Geometry gb = ssim_hip::plan(width, height, count, mode, 0, 6, c->cu_count, c->xcd_count);
            if (gb.n_chunks && gb.cells_y % gb.chunk_cells == 0) Add::one(cand, c, width, height, count, map, keep ? keep : 2, (int)(gb.chunk_cells * cell));
        } else if (!map && g0.cells_y % g0.chunk_cells == 0) {
            Add::one(cand, c, width, height, count, map, (mode == RMGR_SSIM_HIP_MODE_EXACT || mode == RMGR_SSIM_HIP_MODE_UNFUSED) ? 3 : 2, (int)(g0.chunk_cells * cell));
        }
        if (half != R) Add::one(cand, c, width, height, count, map, keep, (int)half);
        if (twice != R) Add::one(cand, c, width, height, count, map, keep, (int)twice);
        samples.resize(cand.size());
    } catch (...) { return ENOMEM; }

    // synthetic pairs of the shape (SURVEY.md 8(d) pattern): distinct images up to ~1.5 GB, then the descriptors cycle through them
    const size_t plane = (size_t)width * height, per_pair = 2 * plane + (map ? 4 * plane : 0);
    const uint32_t distinct = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(count, (uint64_t(3) << 29) / per_pair));
    const std::unique_ptr<PairDesc[]> descs(new (std::nothrow) PairDesc[count]);
    if (!descs) return ENOMEM;
    std::unique_ptr<uint8_t, HipFree> images;
    std::unique_ptr<float, HipFree> maps;
    std::unique_ptr<double, HipFree> sums;
    int rc;
    if ((rc = device_alloc(images, 2 * plane * distinct))) return rc;
    if (map && (rc = device_alloc(maps, plane * distinct))) return rc;
    if ((rc = device_alloc(sums, count))) return rc;
    for (uint32_t i = 0; i < distinct; ++i)
        HIP_TRY(ssim_hip::launch_synth_pair(images.get() + 2 * plane * i, width, images.get() + 2 * plane * i + plane, width, width, height, 0x5EEDull + i, c->stream));
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t k = i % distinct;
        PairDesc& d = descs[i];
        d.a = images.get() + 2 * plane * k; d.a_step = 1; d.a_stride = width;
        d.b = d.a + plane;            d.b_step = 1; d.b_stride = width;
        d.map = map ? maps.get() + plane * k : NULL; d.map_step = map ? 1 : 0; d.map_stride = map ? (int64_t)width : 0;
    }

    // timing: rounds of (every candidate: one untimed + three timed launches), candidates interleaved so that clock drift hits all alike; the
    // figure of a candidate is the median of its per-round means
    const int saved_rows = c->strip_rows, saved_variant = c->variant;
    const bool saved_prof = c->profiling;
    rc = drain_profile(c);
    const uint64_t saved_launches = c->prof_launches;
    const double saved_ms = c->prof_ms;
    const int rounds = 3, per_round = 3;
    for (int r = 0; r < rounds && !rc; ++r) {
        for (size_t k = 0; k < cand.size() && !rc; ++k) {
            c->strip_rows = cand[k].rows; c->variant = cand[k].variant;
            c->profiling = false;
            rc = enqueue(c, width, height, count, descs.get(), map, sums.get());
            c->profiling = true;
            c->prof_launches = 0; c->prof_ms = 0.0;
            for (int j = 0; j < per_round && !rc; ++j) rc = enqueue(c, width, height, count, descs.get(), map, sums.get());
            if (!rc) { const hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess) { (void)hipGetLastError(); rc = map_hip_error(e); } }
            if (!rc) rc = drain_profile(c);
            if (!rc && c->prof_launches) { try { samples[k].push_back(c->prof_ms / (double)c->prof_launches); } catch (...) { rc = ENOMEM; } }
        }
    }
    (void)hipStreamSynchronize(c->stream);
    c->strip_rows = saved_rows; c->variant = saved_variant; c->profiling = saved_prof;
    c->prof_launches = saved_launches; c->prof_ms = saved_ms;
    if (rc) return rc;
    size_t best = 0;
    for (size_t k = 0; k < cand.size(); ++k) {
        if (samples[k].empty()) return ECHILD;
        std::sort(samples[k].begin(), samples[k].end());
        cand[k].ms = samples[k][samples[k].size() / 2];
        if (cand[k].ms < cand[best].ms) best = k;
    }
    // a winner must beat the default by more than the measurement's own scatter (0.5 %) to replace it
    if (best != 0 && cand[best].ms > cand[0].ms * 0.995) best = 0;
    if (best != 0) {
        try { const rmgr_ssim_hip_Context_::Tuned t = {width, height, count, mode, map, cand[best].variant, cand[best].rows}; c->tuned.push_back(t); }
        catch (...) { return ENOMEM; }
    }
    if (result) {
        rmgr_ssim_hip_TuneResult full;
        memset(&full, 0, sizeof(full));
        full.structSize = result->structSize;
        full.candidates = (rmgr_uint32_t)cand.size();
        full.bestVariant = cand[best].variant;
        full.bestStripRows = (rmgr_uint32_t)cand[best].rows;
        full.defaultMs = cand[0].ms;
        full.bestMs = cand[best].ms;
        for (size_t k = 0; k < cand.size() && k < RMGR_SSIM_HIP_TUNE_MAX_CANDIDATES; ++k) {
            full.candidateVariant[k] = cand[k].variant; full.candidateStripRows[k] = (rmgr_uint32_t)cand[k].rows; full.candidateMs[k] = cand[k].ms;
        }
        memcpy(result, &full, std::min<size_t>(result->structSize, sizeof(full)));
    }
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_clear_tuned(rmgr_ssim_hip_Context* c) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    c->tuned.clear();
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_get_tuned(const rmgr_ssim_hip_Context* c, rmgr_uint32_t index, rmgr_ssim_hip_TunedEntry* entry) RMGR_NOEXCEPT
{
    if (!c || !entry) return EINVAL;
    if (index >= c->tuned.size()) return ENOENT;
    const rmgr_ssim_hip_Context_::Tuned& t = c->tuned[index];
    entry->width = t.width; entry->height = t.height; entry->count = t.count;
    entry->withMap = t.map ? 1 : 0; entry->mode = t.mode; entry->variant = t.variant; entry->stripRows = (rmgr_uint32_t)t.strip_rows;
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_set_tuned(rmgr_ssim_hip_Context* c, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count, rmgr_int32_t withMap,
                                     rmgr_int32_t variant, rmgr_uint32_t stripRows) RMGR_NOEXCEPT
{
    if (!c || width == 0 || height == 0 || count == 0 || variant < 0 || stripRows > 0x7FFFFFFFu || (variant == 0 && stripRows == 0)) return EINVAL;
    const bool map = withMap != 0;
    const rmgr_ssim_hip_Context_::Tuned t = {width, height, count, c->mode, map, variant, (int)stripRows};
    if (rmgr_ssim_hip_Context_::Tuned* old = c->tuned_for(width, height, count, map)) { *old = t; return 0; }
    try { c->tuned.push_back(t); } catch (...) { return ENOMEM; }
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_probe_valu(rmgr_ssim_hip_Context* c, rmgr_int32_t wavesPerSimd, rmgr_int32_t streamKind, rmgr_int32_t launches, double* teraLaneOps,
                                      double* shaderMHz, double* slowestXcdMHz) RMGR_NOEXCEPT
{
    if (!c || !teraLaneOps || launches < 1 || launches > 64 || (streamKind != 0 && streamKind != 1)) return EINVAL;
    if (wavesPerSimd != 1 && wavesPerSimd != 2 && wavesPerSimd != 3 && wavesPerSimd != 4 && wavesPerSimd != 8) return EINVAL;
    USE_DEVICE(c);
    // ~2 ms per launch at any occupancy (the strip kernel's own duration on the headline batch): a SIMD retires one packed instruction per
    // 4.2 ... 4.9 clocks, so W waves x 24 instructions x iters / 2.4 GHz ~ 2 ms  ->  iters ~ 40000 / W
    const int iters = 40000 / wavesPerSimd;
    int rc = c->partials.grow(64 + ssim_hip::kClockWords);        // the kernel's (never written) output pointer + the clock counters
    if (rc) return rc;
    uint64_t* clock = NULL;                                        // the timed launches' first workgroups (one per XCD) report the shader clock they ran at
    if (shaderMHz || slowestXcdMHz) {
        clock = reinterpret_cast<uint64_t*>(c->partials.get() + 64);
        HIP_TRY(hipMemsetAsync(clock, 0, ssim_hip::kClockWords * sizeof(uint64_t), c->stream));
    }
    // A BURST is enqueued back to back -- untimed launches (20 in the first burst, ~40 ms: the chip takes ~25 ms of sustained load to leave its idle clock, and every
    // host-side wait between launches is an idle gap after which it ramps again), then the timed ones, each between two events -- and waited for once.  THREE bursts, the
    // best one counts: a burst sometimes runs in a degraded mode for its whole length -- at an unchanged shader clock on every XCD the rate is what W - 1 concurrent
    // waves followed by a lone one would give (two waves: 51 T, the ONE-wave rate, instead of 65...68; three: 58 / 70; four: 62 / 71; eight: 68 / 72) -- about one burst
    // in four, more often right after short or sparse launches, never two calls alike (profiles/r06_probe_bimodal.txt; the strip kernels show nothing of the kind).  The
    // yardstick is what the device CAN sustain: the best burst's median.
    std::vector<hipEvent_t> ev;
    hipError_t err = hipSuccess;
    try { ev.assign((size_t)launches + 1, (hipEvent_t)NULL); } catch (...) { return ENOMEM; }
    for (size_t k = 0; k < ev.size() && err == hipSuccess; ++k) err = hipEventCreate(&ev[k]);
    float best = 0.f;
    uint64_t best_clock[ssim_hip::kClockWords];
    memset(best_clock, 0, sizeof(best_clock));
    for (int burst = 0; burst < 3 && err == hipSuccess; ++burst) {
        if (clock) err = hipMemsetAsync(clock, 0, ssim_hip::kClockWords * sizeof(uint64_t), c->stream);
        for (int k = 0; k < (burst == 0 ? 20 : 6) && err == hipSuccess; ++k)
            err = ssim_hip::launch_probe_valu(wavesPerSimd, streamKind, c->cu_count, c->xcd_count, iters, reinterpret_cast<float*>(c->partials.get()), c->stream, NULL);
        if (err == hipSuccess) err = hipEventRecord(ev[0], c->stream);
        for (int k = 0; k < launches && err == hipSuccess; ++k) {
            err = ssim_hip::launch_probe_valu(wavesPerSimd, streamKind, c->cu_count, c->xcd_count, iters, reinterpret_cast<float*>(c->partials.get()), c->stream, clock);
            if (err == hipSuccess) err = hipEventRecord(ev[k + 1], c->stream);
        }
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        float ms[64];
        for (int k = 0; k < launches && err == hipSuccess; ++k) err = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
        if (err != hipSuccess) break;
        std::sort(ms, ms + launches);
        const float med = ms[launches / 2];
        if (med > 0.f && (best == 0.f || med < best)) {
            best = med;
            if (clock) err = hipMemcpy(best_clock, clock, sizeof(best_clock), hipMemcpyDeviceToHost);
        }
    }
    for (size_t k = 0; k < ev.size(); ++k) if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (err != hipSuccess) { (void)hipGetLastError(); return map_hip_error(err); }
    if (!(best > 0.f)) return ECHILD;
    *teraLaneOps = (double)ssim_hip::probe_valu_lane_ops(wavesPerSimd, c->cu_count, iters) / ((double)best * 1e-3) / 1e12;
    if (clock) clocks_from(best_clock, c->xcd_count, c->wall_clock_khz, shaderMHz, slowestXcdMHz, NULL);
    return 0;
}

rmgr_int32_t rmgr_ssim_hip_synth_pair_device(rmgr_ssim_hip_Context* c, rmgr_uint8_t* imgA, ptrdiff_t strideA, rmgr_uint8_t* imgB, ptrdiff_t strideB,
                                             rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint64_t seed) RMGR_NOEXCEPT
{
    if (!c || !imgA || !imgB) return EINVAL;
    USE_DEVICE(c);
    HIP_TRY(ssim_hip::launch_synth_pair(imgA, strideA, imgB, strideB, width, height, seed, c->stream));
    return 0;
}

} // extern "C"
