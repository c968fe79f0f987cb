// ssim3f_abi.cpp -- the entry points of the C ABI for float32 VOLUMES: SSIM under the three-dimensional window, its gradient and the
// gradient of its map for a per-voxel upstream gradient (rmgr_ssim_hip_*_ssim3f*), each under the engine's window and, _win, under the
// caller's.  The definition is in include/rmgr/ssim-hip.h, the kernels in ssim3f_kernels.hip and ssim3w_kernels.hip (11 taps) and in
// ssim3k_kernels.hip (3, 5, 7 and 9 taps).
//
// The flow is the one of ssim_samples_abi.cpp, written for three strides: validation before any device is touched, sub-batches under
// kScratchCap of device scratch (cell partials, staged volumes and maps; the backward's coefficient volumes) with at least one volume
// each, staging of host volumes, enqueue, strided map copy-back.  Every volume's sum runs over fixed cells in a fixed order and every
// map and gradient voxel belongs to one fixed tile: neither the sub-batches nor the launch a volume lands in change a bit.
//
// It runs on the context's ring of descriptor tables, its cell partials and its pinned sums (sf_slots, sf_partials, sf_sums_pin), which
// the 2-D families use as well, and on the coefficient scratch s3_coef: one stream, stream order.  An enqueue form never waits for the
// host, except -- at most -- for the launch that read its ring slot kSfSlots enqueues ago.
#include "ssim_context.h"
#include "ssim3_flow.h"
#include "ssim3f_kernels.h"
#include "ssim3w_kernels.h"
#include "ssim3k_kernels.h"

#include <cmath>

using namespace ssim_host;
using namespace ssim_host::volumes;      // kScratchCap, round64, volume_bytes, take3f, ring_launch, copy_map_back, Window3, window_validate

namespace {

using ssim_hip::Pair3FDesc;
using ssim_hip::Grad3FDesc;
using ssim_hip::GradOut3FDesc;
using ssim_hip::Geometry3F;

// ---- validation, before any device is touched -----------------------------------------------------------------------------------------------

int validate3f(uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange, const void* out)
{
    if (!(dataRange > 0.0f) || !std::isfinite(dataRange)) return EINVAL;
    if (count == 0 || params == NULL || out == NULL) return EINVAL;
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    if (W == 0 || H == 0 || D == 0 || W > ssim_hip::kS3MaxDim || H > ssim_hip::kS3MaxDim || D > ssim_hip::kS3MaxDim) return EINVAL;
    for (uint32_t i = 0; i < count; ++i) {
        const rmgr_ssim_hip_Params3F& p = params[i];
        if (p.width != W || p.height != H || p.depth != D) return EINVAL;
        if (p.imgA.topLeft == NULL || p.imgB.topLeft == NULL) return EINVAL;
        if (((uintptr_t)p.imgA.topLeft & 3u) || ((uintptr_t)p.imgB.topLeft & 3u) || ((uintptr_t)p.ssimMap & 3u)) return EINVAL;
    }
    if (ssim_hip::ssim3f_max_count(W, H, D) == 0) return EINVAL;
    return 0;
}

int validate_grads3f(uint32_t count, const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB)
{
    if (gradA == NULL && gradB == NULL) return EINVAL;
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 2; ++k) {
            const rmgr_ssim_hip_Grad3F* g = k ? gradB : gradA;
            if (g && (g[i].topLeft == NULL || ((uintptr_t)g[i].topLeft & 3u))) return EINVAL;
        }
    return 0;
}

// ---- descriptors (the sub-batch rule take3f, the staged bytes, the ring launch and the map copy-back: ssim3_flow.h) ----------------------

Pair3FDesc make_desc(const rmgr_ssim_hip_Params3F& p, bool with_map)
{
    Pair3FDesc d;
    d.a = p.imgA.topLeft; d.a_step = p.imgA.step; d.a_stride = p.imgA.stride; d.a_slice = p.imgA.sliceStride;
    d.b = p.imgB.topLeft; d.b_step = p.imgB.step; d.b_stride = p.imgB.stride; d.b_slice = p.imgB.sliceStride;
    const bool m = with_map && p.ssimMap;
    d.map = m ? p.ssimMap : NULL;
    d.map_step = m ? p.ssimStep : 0;
    d.map_stride = m ? p.ssimStride : 0;
    d.map_slice = m ? p.ssimSliceStride : 0;
    return d;
}

// ---- the forward flow -----------------------------------------------------------------------------------------------------------------------------

uint64_t partials_per_volume(uint32_t W, uint32_t H, uint32_t D) { return ssim_hip::plan3f(W, H, D, 1, 0).cells_per_volume() * sizeof(double); }

// Enqueues n pairs (descriptors in host memory, volumes on the device): descriptor upload, walk, reduction into sums[0 .. n-1].
// The cells (and with them the partials) are the same for every radius; a smaller window's chunks pay fewer warm-up slices.
int enqueue_volumes(rmgr_ssim_hip_Context* c, float range, const Window3& win, uint32_t n, const Pair3FDesc* d, uint32_t W, uint32_t H, uint32_t D, double* sums)
{
    const Geometry3F geo = ssim_hip::plan3k(win.radius, W, H, D, n, c->cu_count);
    int rc;
    if ((rc = c->sf_partials.grow((size_t)(geo.cells_per_volume() * n)))) return rc;
    return ring_launch(c, n * sizeof(Pair3FDesc),
        [&](uint8_t* pin) { memcpy(pin, d, n * sizeof(Pair3FDesc)); },
        [&](const uint8_t* dev) {
            const Pair3FDesc* descs = reinterpret_cast<const Pair3FDesc*>(dev);
            if (win.radius == 5)
                return ssim_hip::launch_ssim3f(geo, descs, range, c->sf_partials, sums, c->stream, win.gf);
            return ssim_hip::launch_ssim3k(win.radius, win.gf, geo, descs, range, c->sf_partials, sums, c->stream);
        });
}

int enqueue_all(rmgr_ssim_hip_Context* c, float range, const Window3& win, uint32_t count, const rmgr_ssim_hip_Params3F* params, double* sums)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    try {
        std::vector<Pair3FDesc> d;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged;
            const uint32_t n = take3f(params, i0, count, ssim_hip::ssim3f_max_count(W, H, D), partials_per_volume(W, H, D), false, staged);
            d.resize(n);
            for (uint32_t i = 0; i < n; ++i) d[i] = make_desc(params[i0 + i], true);
            const int rc = enqueue_volumes(c, range, win, n, &d[0], W, H, D, sums + i0);
            if (rc) return rc;
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    return 0;
}

// The blocking entry points: every sub-batch into the pinned sums, then the means.  stage: host pointers -- the volumes are copied (each
// volume's sample range) into c->stage_a, a pair's map is written densely into it as well and copied back at its own strides.
int blocking(rmgr_ssim_hip_Context* c, float range, const Window3& win, uint32_t count, const rmgr_ssim_hip_Params3F* params, float* ssim, bool stage)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const double voxels = (double)W * (double)H * (double)D;
    int rc;
    if ((rc = c->sf_sums_pin.grow(count))) return rc;
    try {
        std::vector<Pair3FDesc> d;
        std::vector<uint64_t> map_off;
        std::vector<float> back;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged;
            const uint32_t n = take3f(params, i0, count, ssim_hip::ssim3f_max_count(W, H, D), partials_per_volume(W, H, D), stage, staged);
            d.resize(n);
            map_off.assign(n, 0);
            if (stage && (rc = c->stage_a.grow((size_t)staged))) return rc;
            uint64_t off = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const rmgr_ssim_hip_Params3F& p = params[i0 + i];
                d[i] = make_desc(p, true);
                if (!stage) continue;
                for (int k = 0; k < 2; ++k) {
                    const rmgr_ssim_hip_Img3F& im = k ? p.imgB : p.imgA;
                    int64_t lo;
                    const size_t bytes = volume_bytes(im, W, H, D, lo);
                    HIP_TRY(hipMemcpyAsync(c->stage_a + off, im.topLeft + lo, bytes, hipMemcpyHostToDevice, c->stream));
                    (k ? d[i].b : d[i].a) = reinterpret_cast<const float*>(c->stage_a + off) - lo;
                    off += round64(bytes);
                }
                if (p.ssimMap) {
                    map_off[i] = off;
                    d[i].map = reinterpret_cast<float*>(c->stage_a + off);
                    d[i].map_step = 1; d[i].map_stride = W; d[i].map_slice = (int64_t)W * H;
                    off += round64((uint64_t)W * H * D * 4);
                }
            }
            if ((rc = enqueue_volumes(c, range, win, n, &d[0], W, H, D, c->sf_sums_pin + i0))) return rc;
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (uint32_t i = 0; i < n && stage; ++i) {
                const rmgr_ssim_hip_Params3F& p = params[i0 + i];
                if (!p.ssimMap) continue;
                if ((rc = copy_map_back(reinterpret_cast<const float*>(c->stage_a + map_off[i]), p, back))) return rc;
            }
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    for (uint32_t i = 0; i < count; ++i) ssim[i] = (float)(c->sf_sums_pin[i] / voxels);
    return 0;
}

// ---- the gradient and the gradient of the map ---------------------------------------------------------------------------------------------
// Per sub-batch: the walk that writes the coefficient volumes (3 floats per voxel for one gradient, 4 for both) into c->s3_coef, then the
// adjoint walk that reads them.  The next sub-batch rewrites the scratch in stream order.  One flow serves both upstream forms: the scalar
// form (gradOutDevice) or -- maps -- a third table in the descriptor slot, the GradOut3FDesc of the sub-batch, through which the first walk
// reads k per voxel (ssim3w_kernels.hip; ssim3k_kernels.hip for the smaller windows).
int validate_grad_maps3f(uint32_t count, const rmgr_ssim_hip_GradOut3F* maps)
{
    if (maps == NULL) return EINVAL;
    for (uint32_t i = 0; i < count; ++i)
        if (maps[i].topLeft == NULL || ((uintptr_t)maps[i].topLeft & 3u)) return EINVAL;
    return 0;
}

int grad_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params3F* params, float range, const Window3& win,
               const float* gradOutDevice, const rmgr_ssim_hip_GradOut3F* maps, const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const int which = (gradA ? 1 : 0) | (gradB ? 2 : 0);
    const uint64_t per_volume = (uint64_t)ssim_hip::ssim3f_coef_planes(which) * W * H * D;
    for (uint32_t i0 = 0; i0 < count;) {
        uint64_t staged;
        const uint32_t n = take3f(params, i0, count, ssim_hip::ssim3f_max_count(W, H, D), per_volume * sizeof(float), false, staged);
        const Geometry3F geo = ssim_hip::plan3k(win.radius, W, H, D, n, c->cu_count);
        int rc;
        if ((rc = c->s3_coef.grow((size_t)(per_volume * n)))) return rc;
        const size_t pair_bytes = n * sizeof(Pair3FDesc), grad_bytes = n * sizeof(Grad3FDesc);
        rc = ring_launch(c, pair_bytes + grad_bytes + (maps ? n * sizeof(GradOut3FDesc) : 0),
            [&](uint8_t* pin) {
                Pair3FDesc* pd = reinterpret_cast<Pair3FDesc*>(pin);
                Grad3FDesc* gd = reinterpret_cast<Grad3FDesc*>(pin + pair_bytes);
                GradOut3FDesc* od = reinterpret_cast<GradOut3FDesc*>(pin + pair_bytes + grad_bytes);
                for (uint32_t i = 0; i < n; ++i) {
                    pd[i] = make_desc(params[i0 + i], false);
                    Grad3FDesc g = {NULL, 0, 0, 0, NULL, 0, 0, 0};
                    if (gradA) { const rmgr_ssim_hip_Grad3F& s = gradA[i0 + i]; g.ga = s.topLeft; g.ga_step = s.step; g.ga_stride = s.stride; g.ga_slice = s.sliceStride; }
                    if (gradB) { const rmgr_ssim_hip_Grad3F& s = gradB[i0 + i]; g.gb = s.topLeft; g.gb_step = s.step; g.gb_stride = s.stride; g.gb_slice = s.sliceStride; }
                    gd[i] = g;
                    if (!maps) continue;
                    const rmgr_ssim_hip_GradOut3F& m = maps[i0 + i];
                    const GradOut3FDesc o = {m.topLeft, (int64_t)m.step, (int64_t)m.stride, (int64_t)m.sliceStride};
                    od[i] = o;
                }
            },
            [&](const uint8_t* dev) {
                const Pair3FDesc* pd = reinterpret_cast<const Pair3FDesc*>(dev);
                const Grad3FDesc* gd = reinterpret_cast<const Grad3FDesc*>(dev + pair_bytes);
                const GradOut3FDesc* od = maps ? reinterpret_cast<const GradOut3FDesc*>(dev + pair_bytes + grad_bytes) : NULL;
                const float* g_out = maps ? NULL : gradOutDevice + i0;
                if (win.radius != 5)
                    return ssim_hip::launch_ssim3k_grad(win.radius, win.gf, geo, pd, gd, g_out, od, range, which, c->s3_coef, c->stream);
                if (maps)
                    return ssim_hip::launch_ssim3w_grad(geo, pd, gd, od, range, which, c->s3_coef, c->stream, win.gf);
                return ssim_hip::launch_ssim3f_grad(geo, pd, gd, g_out, range, which, c->s3_coef, c->stream, win.gf);
            });
        if (rc) return rc;
        i0 += n;
    }
    return 0;
}

// ---- what an entry does once its pairs are valid; `window` is NULL (the engine's window) or the caller's ---------------------------------

int enqueue_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange, const rmgr_ssim_hip_Window* window,
                  double* sumsDevice)
{
    Window3 win;
    const int rc = window_validate(window, win);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return enqueue_all(c, dataRange, win, count, params, sumsDevice);
}

int device_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange, const rmgr_ssim_hip_Window* window,
                 float* ssim)
{
    Window3 win;
    const int rc = window_validate(window, win);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return blocking(c, dataRange, win, count, params, ssim, false);
}

int host_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange, const rmgr_ssim_hip_Window* window,
               float* ssim)
{
    Window3 win;
    int rc = window_validate(window, win);
    if (rc) return rc;
    Lease lease;                         // ctx == NULL: one of the default contexts, for this call only
    if ((rc = lease.take(c))) return rc;
    USE_DEVICE(lease.c);
    return blocking(lease.c, dataRange, win, count, params, ssim, true);
}

int grad_entry_checked(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange, const rmgr_ssim_hip_Window* window,
                       const float* gradOutDevice, const rmgr_ssim_hip_GradOut3F* maps, const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB)
{
    Window3 win;
    int rc = validate_grads3f(count, gradA, gradB);
    if (rc) return rc;
    if (gradOutDevice == NULL && (rc = validate_grad_maps3f(count, maps))) return rc;
    if ((rc = window_validate(window, win))) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return grad_entry(c, count, params, dataRange, win, gradOutDevice, gradOutDevice ? NULL : maps, gradA, gradB);
}

} // namespace

extern "C" {

// Every entry exists twice: under the engine's window and, _win, under the caller's (include/rmgr/ssim-hip.h: rmgr_ssim_hip_Window).
// Both run the same flow; the window is one more input.

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                          float dataRange, double* sumsDevice) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, sumsDevice);
    return rc ? rc : enqueue_entry(c, count, params, dataRange, NULL, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                              float dataRange, const rmgr_ssim_hip_Window* window, double* sumsDevice) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, sumsDevice);
    return rc ? rc : enqueue_entry(c, count, params, dataRange, window, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                 float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, ssim);
    return rc ? rc : device_entry(c, count, params, dataRange, NULL, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                     float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, ssim);
    return rc ? rc : device_entry(c, count, params, dataRange, window, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                               float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, ssim);
    return rc ? rc : host_entry(c, count, params, dataRange, NULL, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, ssim);
    return rc ? rc : host_entry(c, count, params, dataRange, window, ssim);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                               float dataRange, const float* gradOutDevice,
                                               const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, gradOutDevice);
    return rc ? rc : grad_entry_checked(c, count, params, dataRange, NULL, gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_Window* window, const float* gradOutDevice,
                                                   const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, gradOutDevice);
    return rc ? rc : grad_entry_checked(c, count, params, dataRange, window, gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                   const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, gradOutMaps);
    return rc ? rc : grad_entry_checked(c, count, params, dataRange, NULL, NULL, gradOutMaps, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                       float dataRange, const rmgr_ssim_hip_Window* window, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                       const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const int rc = validate3f(count, params, dataRange, gradOutMaps);
    return rc ? rc : grad_entry_checked(c, count, params, dataRange, window, NULL, gradOutMaps, gradA, gradB);
}

} // extern "C"
