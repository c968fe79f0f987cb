// ssim_volumes_abi.cpp -- the entry points of the C ABI for VOLUMES: SSIM under the three-dimensional window of float32 (ssim3f) and of
// float16 / bfloat16 samples (ssim3h), its gradient for a scalar and for a per-voxel upstream gradient, each under the engine's window
// and, _win, under the caller's; and multi-scale SSIM of float32 (msssim3f) and of float16 / bfloat16 volumes (msssim3h) with its
// gradient.  The definitions are in include/rmgr/ssim-hip.h, the kernels in ssim3f_ / ssim3w_ / ssim3k_ / ssim3h_ / ssim3hk_ /
// msssim3f_ / msssim3h_ / msssim3k_ / msssim3hk_kernels.hip.
//
// The flow is the one of ssim_samples_abi.cpp, written for three strides: validation before any device is touched, sub-batches under
// kScratchCap of device scratch (cell partials, staged volumes and maps; the backward's coefficient volumes; the pyramids) with at least
// one volume each, staging of host volumes, enqueue, strided map copy-back.  The two sample types differ in their sample, in what a
// launch is told (data range; encoding and data range) and in the kernels that read and write the caller's volumes; each is described
// once by a small struct (Family3F / Family3H, and Multi3F / Multi3H for the multi-scale path) and the flow is written once over it.
// The planner, the cells, the coefficient layout and every scratch volume are float32's whatever the samples are.
//
// Every volume's sum runs over fixed cells in a fixed order, every map and gradient voxel belongs to one fixed tile, and every pyramid
// volume belongs to one pair: neither the sub-batches nor the launch a volume lands in change a bit.
//
// It runs on the context's ring of descriptor tables, its cell partials and its pinned sums (sf_slots, sf_partials, sf_sums_pin), which
// the 2-D families use as well, on the coefficient scratch s3_coef and -- multi-scale -- on msf_pyramid, msf_grads, msf_partials,
// msf_coef (k_s) and msf_out, all rewritten in stream order: one stream.  An enqueue form never waits for the host, except -- at most --
// for the launch that read its ring slot kSfSlots enqueues ago.
#include "ssim3_flow.h"
#include "ssim3w_kernels.h"
#include "ssim3hk_kernels.h"
#include "msssim3h_kernels.h"
#include "msssim3hk_kernels.h"

using namespace ssim_host;
using namespace ssim_host::volumes;      // volume_bytes, take3f, copy_map_back

namespace {

using ssim_hip::Pair3FDesc;
using ssim_hip::Grad3FDesc;
using ssim_hip::Pair3HDesc;
using ssim_hip::Grad3HDesc;
using ssim_hip::GradOut3FDesc;
using ssim_hip::Geometry3F;

// ---- the families ------------------------------------------------------------------------------------------------------------------------------
// Params / Grad / Desc / GradDesc / Sample: the public parameter blocks, the kernels' descriptors of a pair and of its gradient volumes,
// the type of a sample.  The per-call arguments are the members; `win` is filled in once the window is parsed.  check() is what an
// entry checks before it looks at its pairs.  launch() enqueues the walk and the reduction of geo's pairs into sums (device or pinned
// host memory); launch_grad() and launch_map_grad() the coefficient walk into c->s3_coef and the adjoint walk, for a scalar upstream
// gradient per volume and for one per voxel.  Radius 5 runs on the 11-tap kernels, the smaller ones on the k kernels.

int check_call(float range) { return valid_range(range) ? 0 : EINVAL; }
int check_call(uint32_t sampleType, float range)
{
    if (sampleType != RMGR_SSIM_HIP_SAMPLE_F16 && sampleType != RMGR_SSIM_HIP_SAMPLE_BF16) return EINVAL;
    return check_call(range);
}

struct Family3F {
    typedef rmgr_ssim_hip_Params3F Params;
    typedef rmgr_ssim_hip_Grad3F Grad;
    typedef Pair3FDesc Desc;
    typedef Grad3FDesc GradDesc;
    typedef float Sample;
    float range;
    Window win;
    int check() const { return check_call(range); }
    hipError_t launch(rmgr_ssim_hip_Context* c, const Geometry3F& geo, const Desc* dev, double* sums) const
    {
        if (win.radius == 5) return ssim_hip::launch_ssim3f(geo, dev, range, c->sf_partials, sums, c->stream, win.gf);
        return ssim_hip::launch_ssim3k(win.radius, win.gf, geo, dev, range, c->sf_partials, sums, c->stream);
    }
    hipError_t launch_grad(rmgr_ssim_hip_Context* c, const Geometry3F& geo, const Desc* pd, const GradDesc* gd, const float* g_out, int which) const
    {
        if (win.radius == 5) return ssim_hip::launch_ssim3f_grad(geo, pd, gd, g_out, range, which, c->s3_coef, c->stream, win.gf);
        return ssim_hip::launch_ssim3k_grad(win.radius, win.gf, geo, pd, gd, g_out, NULL, range, which, c->s3_coef, c->stream);
    }
    hipError_t launch_map_grad(rmgr_ssim_hip_Context* c, const Geometry3F& geo, const Desc* pd, const GradDesc* gd, const GradOut3FDesc* od, int which) const
    {
        if (win.radius == 5) return ssim_hip::launch_ssim3w_grad(geo, pd, gd, od, range, which, c->s3_coef, c->stream, win.gf);
        return ssim_hip::launch_ssim3k_grad(win.radius, win.gf, geo, pd, gd, NULL, od, range, which, c->s3_coef, c->stream);
    }
};

struct Family3H {
    typedef rmgr_ssim_hip_Params3H Params;
    typedef rmgr_ssim_hip_Grad3H Grad;
    typedef Pair3HDesc Desc;
    typedef Grad3HDesc GradDesc;
    typedef uint16_t Sample;
    uint32_t sampleType;
    float range;
    Window win;
    int check() const { return check_call(sampleType, range); }
    int type() const { return sample_type(sampleType); }        // kSHTypeF16 / kSHTypeBF16
    hipError_t launch(rmgr_ssim_hip_Context* c, const Geometry3F& geo, const Desc* dev, double* sums) const
    {
        if (win.radius == 5) return ssim_hip::launch_ssim3h(geo, dev, type(), range, c->sf_partials, sums, c->stream, win.gf);
        return ssim_hip::launch_ssim3hk(win.radius, win.gf, geo, dev, type(), range, c->sf_partials, sums, c->stream);
    }
    hipError_t launch_grad(rmgr_ssim_hip_Context* c, const Geometry3F& geo, const Desc* pd, const GradDesc* gd, const float* g_out, int which) const
    {
        if (win.radius == 5) return ssim_hip::launch_ssim3h_grad(geo, pd, gd, type(), g_out, range, which, c->s3_coef, c->stream, win.gf);
        return ssim_hip::launch_ssim3hk_grad(win.radius, win.gf, geo, pd, gd, type(), g_out, NULL, range, which, c->s3_coef, c->stream);
    }
    hipError_t launch_map_grad(rmgr_ssim_hip_Context* c, const Geometry3F& geo, const Desc* pd, const GradDesc* gd, const GradOut3FDesc* od, int which) const
    {
        if (win.radius == 5) return ssim_hip::launch_ssim3h_map_grad(geo, pd, gd, od, type(), range, which, c->s3_coef, c->stream, win.gf);
        return ssim_hip::launch_ssim3hk_grad(win.radius, win.gf, geo, pd, gd, type(), NULL, od, range, which, c->s3_coef, c->stream);
    }
};

// ---- validation, before any device is touched -----------------------------------------------------------------------------------------------

// What every entry checks of its call and its pairs; `out` is whichever output the entry requires.  A pair's map is float32 whatever the
// samples are; multi: the multi-scale entries, which write no map.
template <typename F, typename Fam>
int validate_pairs(const Fam& fam, uint32_t count, const typename F::Params* params, const void* out, bool multi)
{
    const int rc = fam.check();
    if (rc) return rc;
    if (count == 0 || params == NULL || out == NULL) return EINVAL;
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    if (W == 0 || H == 0 || D == 0 || W > ssim_hip::kS3MaxDim || H > ssim_hip::kS3MaxDim || D > ssim_hip::kS3MaxDim) return EINVAL;
    const uintptr_t mask = sizeof(typename F::Sample) - 1;
    for (uint32_t i = 0; i < count; ++i) {
        const typename F::Params& p = params[i];
        if (p.width != W || p.height != H || p.depth != D) return EINVAL;
        if (p.imgA.topLeft == NULL || p.imgB.topLeft == NULL) return EINVAL;
        if (((uintptr_t)p.imgA.topLeft & mask) || ((uintptr_t)p.imgB.topLeft & mask)) return EINVAL;
        if (multi ? p.ssimMap != NULL : ((uintptr_t)p.ssimMap & 3u) != 0) return EINVAL;
    }
    return 0;
}

template <typename F>
int validate(const F& fam, uint32_t count, const typename F::Params* params, const void* out)
{
    const int rc = validate_pairs<F>(fam, count, params, out, false);
    if (rc) return rc;
    return ssim_hip::ssim3f_max_count(params[0].width, params[0].height, params[0].depth) == 0 ? EINVAL : 0;
}

// The volumes of a gradient entry: gradA and / or gradB, every volume non-NULL and aligned to its samples.
template <typename G>
int validate_grads(uint32_t count, const G* gradA, const G* gradB)
{
    if (gradA == NULL && gradB == NULL) return EINVAL;
    const uintptr_t mask = sizeof(*gradA->topLeft) - 1;
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 2; ++k) {
            const G* g = k ? gradB : gradA;
            if (g && (g[i].topLeft == NULL || ((uintptr_t)g[i].topLeft & mask))) return EINVAL;
        }
    return 0;
}

// What the map-gradient entries check beyond the _grad entries.
int validate_grad_maps(uint32_t count, const rmgr_ssim_hip_GradOut3F* maps)
{
    if (maps == NULL) return EINVAL;
    for (uint32_t i = 0; i < count; ++i)
        if (maps[i].topLeft == NULL || ((uintptr_t)maps[i].topLeft & 3u)) return EINVAL;
    return 0;
}

// ---- descriptors (the sub-batch rule take3f, the staged bytes and the map copy-back: ssim3_flow.h; the ring launch: ssim_flow.h) -----------

template <typename F>
typename F::Desc make_desc(const typename F::Params& p, bool with_map)
{
    typename F::Desc d;
    d.a = p.imgA.topLeft; d.a_step = p.imgA.step; d.a_stride = p.imgA.stride; d.a_slice = p.imgA.sliceStride;
    d.b = p.imgB.topLeft; d.b_step = p.imgB.step; d.b_stride = p.imgB.stride; d.b_slice = p.imgB.sliceStride;
    const bool m = with_map && p.ssimMap;
    d.map = m ? p.ssimMap : NULL;
    d.map_step = m ? p.ssimStep : 0;
    d.map_stride = m ? p.ssimStride : 0;
    d.map_slice = m ? p.ssimSliceStride : 0;
    return d;
}

// The gradient volumes of pair i: those of gradA / gradB that the caller wants.
template <typename F>
typename F::GradDesc make_grad_desc(const typename F::Grad* gradA, const typename F::Grad* gradB, uint32_t i)
{
    typename F::GradDesc g = {NULL, 0, 0, 0, NULL, 0, 0, 0};
    if (gradA) { const typename F::Grad& s = gradA[i]; g.ga = s.topLeft; g.ga_step = s.step; g.ga_stride = s.stride; g.ga_slice = s.sliceStride; }
    if (gradB) { const typename F::Grad& s = gradB[i]; g.gb = s.topLeft; g.gb_step = s.step; g.gb_stride = s.stride; g.gb_slice = s.sliceStride; }
    return g;
}

template <typename G> int grad_which(const G* gradA, const G* gradB) { return (gradA ? 1 : 0) | (gradB ? 2 : 0); }

// Host pointers: copies the sample range of both volumes of p to c->stage_a + off (off moves on, in steps of 64) on the context's stream
// and points d at the copies.
template <typename F>
int stage_volumes(rmgr_ssim_hip_Context* c, const typename F::Params& p, typename F::Desc& d, uint64_t& off)
{
    for (int k = 0; k < 2; ++k) {
        const auto& im = k ? p.imgB : p.imgA;
        int64_t lo;
        const size_t bytes = volume_bytes(im, p.width, p.height, p.depth, lo);
        HIP_TRY(hipMemcpyAsync(c->stage_a + off, im.topLeft + lo, bytes, hipMemcpyHostToDevice, c->stream));
        (k ? d.b : d.a) = reinterpret_cast<const typename F::Sample*>(c->stage_a + off) - lo;
        off += round64(bytes);
    }
    return 0;
}

// ---- the forward flow -----------------------------------------------------------------------------------------------------------------------------

uint64_t partials_per_volume(uint32_t W, uint32_t H, uint32_t D) { return ssim_hip::plan3f(W, H, D, 1, 0).cells_per_volume() * sizeof(double); }

// Enqueues n pairs (descriptors in host memory, volumes on the device): descriptor upload, walk, reduction into sums[0 .. n-1].
// The cells (and with them the partials) are the same for every radius; a smaller window's chunks pay fewer warm-up slices.
template <typename F>
int enqueue_volumes(rmgr_ssim_hip_Context* c, const F& fam, uint32_t n, const typename F::Desc* d, uint32_t W, uint32_t H, uint32_t D, double* sums)
{
    typedef typename F::Desc Desc;
    const Window& win = fam.win;
    const Geometry3F geo = ssim_hip::plan3k(win.radius, W, H, D, n, c->cu_count);
    int rc;
    if ((rc = c->sf_partials.grow((size_t)(geo.cells_per_volume() * n)))) return rc;
    return ring_launch(c, n * sizeof(Desc),
        [&](uint8_t* pin) { memcpy(pin, d, n * sizeof(Desc)); },
        [&](const uint8_t* dev) { return fam.launch(c, geo, reinterpret_cast<const Desc*>(dev), sums); });
}

// The enqueue entry points: every sub-batch of device-resident pairs into sums[0 .. count-1] (device), no host synchronisation.
template <typename F>
int enqueue_all(rmgr_ssim_hip_Context* c, const F& fam, uint32_t count, const typename F::Params* params, double* sums)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    try {
        std::vector<typename F::Desc> d;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged;
            const uint32_t n = take3f(params, i0, count, ssim_hip::ssim3f_max_count(W, H, D), partials_per_volume(W, H, D), false, staged);
            d.resize(n);
            for (uint32_t i = 0; i < n; ++i) d[i] = make_desc<F>(params[i0 + i], true);
            const int rc = enqueue_volumes(c, fam, n, &d[0], W, H, D, sums + i0);
            if (rc) return rc;
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    return 0;
}

// The blocking entry points: every sub-batch into the pinned sums, then the means.  stage: host pointers -- the volumes are copied (each
// volume's sample range) into c->stage_a, a pair's float32 map is written densely into it as well and copied back at its own strides.
template <typename F>
int blocking(rmgr_ssim_hip_Context* c, const F& fam, uint32_t count, const typename F::Params* params, float* ssim, bool stage)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const double voxels = (double)W * (double)H * (double)D;
    int rc;
    if ((rc = c->sf_sums_pin.grow(count))) return rc;
    try {
        std::vector<typename F::Desc> d;
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
                const typename F::Params& p = params[i0 + i];
                d[i] = make_desc<F>(p, true);
                if (!stage) continue;
                if ((rc = stage_volumes<F>(c, p, d[i], off))) return rc;
                if (p.ssimMap) {
                    map_off[i] = off;
                    d[i].map = reinterpret_cast<float*>(c->stage_a + off);
                    d[i].map_step = 1; d[i].map_stride = W; d[i].map_slice = (int64_t)W * H;
                    off += round64((uint64_t)W * H * D * 4);
                }
            }
            if ((rc = enqueue_volumes(c, fam, n, &d[0], W, H, D, c->sf_sums_pin + i0))) return rc;
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (uint32_t i = 0; i < n && stage; ++i) {
                const typename F::Params& p = params[i0 + i];
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
// Per sub-batch: the walk that writes the float32 coefficient volumes (3 floats per voxel for one gradient, 4 for both) into c->s3_coef,
// then the adjoint walk that reads them (and, for 16-bit samples, rounds each gradient voxel once).  The next sub-batch -- of either
// family: they share the scratch -- rewrites it in stream order.  One flow serves both upstream forms: maps == NULL, the per-volume
// upstream gradient gradOutDevice; else a third table in the descriptor slot, the GradOut3FDesc of the sub-batch, through which the first
// walk reads k per voxel.
template <typename F>
int grad_entry(rmgr_ssim_hip_Context* c, const F& fam, uint32_t count, const typename F::Params* params, const float* gradOutDevice,
               const rmgr_ssim_hip_GradOut3F* maps, const typename F::Grad* gradA, const typename F::Grad* gradB)
{
    typedef typename F::Desc Desc;
    typedef typename F::GradDesc GradDesc;
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const Window& win = fam.win;
    const int which = grad_which(gradA, gradB);
    const uint64_t per_volume = (uint64_t)ssim_hip::ssim3f_coef_planes(which) * W * H * D;
    for (uint32_t i0 = 0; i0 < count;) {
        uint64_t staged;
        const uint32_t n = take3f(params, i0, count, ssim_hip::ssim3f_max_count(W, H, D), per_volume * sizeof(float), false, staged);
        const Geometry3F geo = ssim_hip::plan3k(win.radius, W, H, D, n, c->cu_count);
        int rc;
        if ((rc = c->s3_coef.grow((size_t)(per_volume * n)))) return rc;
        const size_t pair_bytes = n * sizeof(Desc), grad_bytes = n * sizeof(GradDesc);
        rc = ring_launch(c, pair_bytes + grad_bytes + (maps ? n * sizeof(GradOut3FDesc) : 0),
            [&](uint8_t* pin) {
                Desc* pd = reinterpret_cast<Desc*>(pin);
                GradDesc* gd = reinterpret_cast<GradDesc*>(pin + pair_bytes);
                GradOut3FDesc* od = reinterpret_cast<GradOut3FDesc*>(pin + pair_bytes + grad_bytes);
                for (uint32_t i = 0; i < n; ++i) {
                    pd[i] = make_desc<F>(params[i0 + i], false);
                    gd[i] = make_grad_desc<F>(gradA, gradB, i0 + i);
                    if (!maps) continue;
                    const rmgr_ssim_hip_GradOut3F& m = maps[i0 + i];
                    const GradOut3FDesc o = {m.topLeft, (int64_t)m.step, (int64_t)m.stride, (int64_t)m.sliceStride};
                    od[i] = o;
                }
            },
            [&](const uint8_t* dev) {
                const Desc* pd = reinterpret_cast<const Desc*>(dev);
                const GradDesc* gd = reinterpret_cast<const GradDesc*>(dev + pair_bytes);
                if (maps) return fam.launch_map_grad(c, geo, pd, gd, reinterpret_cast<const GradOut3FDesc*>(dev + pair_bytes + grad_bytes), which);
                return fam.launch_grad(c, geo, pd, gd, gradOutDevice + i0, which);
            });
        if (rc) return rc;
        i0 += n;
    }
    return 0;
}

// ---- what a single-scale entry does once its pairs are valid; `window` is NULL (the engine's window) or the caller's -----------------------

template <typename F>
int enqueue_entry(rmgr_ssim_hip_Context* c, F fam, uint32_t count, const typename F::Params* params, const rmgr_ssim_hip_Window* window, double* sumsDevice)
{
    const int rc = window_validate(window, fam.win);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return enqueue_all(c, fam, count, params, sumsDevice);
}

template <typename F>
int device_entry(rmgr_ssim_hip_Context* c, F fam, uint32_t count, const typename F::Params* params, const rmgr_ssim_hip_Window* window, float* ssim)
{
    const int rc = window_validate(window, fam.win);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return blocking(c, fam, count, params, ssim, false);
}

template <typename F>
int host_entry(rmgr_ssim_hip_Context* c, F fam, uint32_t count, const typename F::Params* params, const rmgr_ssim_hip_Window* window, float* ssim)
{
    int rc = window_validate(window, fam.win);
    if (rc) return rc;
    Lease lease;                         // ctx == NULL: one of the default contexts, for this call only
    if ((rc = lease.take(c))) return rc;
    USE_DEVICE(lease.c);
    return blocking(lease.c, fam, count, params, ssim, true);
}

// gradOutDevice == NULL: the per-voxel upstream form, `maps`.
template <typename F>
int grad_entry_checked(rmgr_ssim_hip_Context* c, F fam, uint32_t count, const typename F::Params* params, const rmgr_ssim_hip_Window* window,
                       const float* gradOutDevice, const rmgr_ssim_hip_GradOut3F* maps, const typename F::Grad* gradA, const typename F::Grad* gradB)
{
    int rc = validate_grads(count, gradA, gradB);
    if (rc) return rc;
    if (gradOutDevice == NULL && (rc = validate_grad_maps(count, maps))) return rc;
    if ((rc = window_validate(window, fam.win))) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return grad_entry(c, fam, count, params, gradOutDevice, gradOutDevice ? NULL : maps, gradA, gradB);
}

// ---- multi-scale SSIM of float32 and of float16 / bfloat16 volumes -----------------------------------------------------------------------
// The flow of msssimf / msssimh (ssim_samples_abi.cpp) written for three strides.  Scale 0 is read where the caller has it; the volumes of
// scales >= 1 (and, in the backward, their gradient volumes) are dense float32 volumes of the context's scratch, one set per pair,
// rewritten by every sub-batch in stream order; the sub-batches are msssim3f_per_sub_batch's and msssim3f_scratch_bytes', the same for
// both families since all of the scratch is float32 / float64.  The two families differ in scale 0 alone -- its samples, its descriptors
// and the kernels that read and write them -- and each is described by a small struct (Multi3F / Multi3H).  The window, the engine's or
// the caller's (_win), is one more member of it: the same at every scale, and nothing of the flow -- pyramid, scratch, sub-batches,
// tables -- depends on it.  Radius 5 runs on the 11-tap kernels with the window's taps, the smaller ones on the k kernels.
//
// A launch reads one table of pair descriptors, scales x n Pair3FDesc as [scale][pair] (rows >= 1: the pyramid), and -- backward -- one
// of gradient descriptors behind it, scales x n Grad3FDesc.  Multi3F: row 0 holds the caller's volumes.  Multi3H: the caller's n
// Pair3HDesc / Grad3HDesc stand in front of each table, whose row 0 nobody reads (zeroed).  kPair0 / kGrad0: the bytes per pair of such
// a scale-0 row of its own.

struct Multi3F {
    typedef Family3F Single;
    float range;
    Window win;
    int check() const { return check_call(range); }
    static constexpr size_t kPair0 = 0, kGrad0 = 0;
    hipError_t forward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, uint32_t n, uint32_t W, uint32_t H, uint32_t D, uint32_t scales, const double* w,
                       double* means, double* values) const
    {
        const Pair3FDesc* pd = reinterpret_cast<const Pair3FDesc*>(pairs);
        if (win.radius == 5)
            return ssim_hip::launch_msssim3f_from(0, win.radius, win.gf, pd, n, W, H, D, scales, range, w, c->cu_count, c->msf_partials, means, values, c->stream);
        return ssim_hip::launch_msssim3k_from(0, win.radius, win.gf, pd, n, W, H, D, scales, range, w, c->cu_count, c->msf_partials, means, values, c->stream);
    }
    hipError_t backward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, const uint8_t* grads, uint32_t n, uint32_t W, uint32_t H, uint32_t D,
                        uint32_t scales, const double* w, const double* means, const float* g_out, int which) const
    {
        const Pair3FDesc* pd = reinterpret_cast<const Pair3FDesc*>(pairs);
        const Grad3FDesc* gd = reinterpret_cast<const Grad3FDesc*>(grads);
        if (win.radius == 5)
            return ssim_hip::launch_msssim3f_grad_from(0, win.radius, win.gf, pd, gd, n, W, H, D, scales, range, w, c->cu_count, means, g_out, c->msf_coef,
                                                       c->s3_coef, which, c->stream);
        return ssim_hip::launch_msssim3k_grad_from(0, win.radius, win.gf, pd, gd, n, W, H, D, scales, range, w, c->cu_count, means, g_out, c->msf_coef,
                                                   c->s3_coef, which, c->stream);
    }
};

struct Multi3H {
    typedef Family3H Single;
    uint32_t sampleType;
    float range;
    Window win;
    int check() const { return check_call(sampleType, range); }
    static constexpr size_t kPair0 = sizeof(Pair3HDesc), kGrad0 = sizeof(Grad3HDesc);
    hipError_t forward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, uint32_t n, uint32_t W, uint32_t H, uint32_t D, uint32_t scales, const double* w,
                       double* means, double* values) const
    {
        const Pair3HDesc* pd0 = reinterpret_cast<const Pair3HDesc*>(pairs);
        const Pair3FDesc* pd = reinterpret_cast<const Pair3FDesc*>(pairs + n * kPair0);
        if (win.radius == 5)
            return ssim_hip::launch_msssim3h(pd0, pd, n, W, H, D, scales, sample_type(sampleType), range, win.radius, win.gf, w, c->cu_count,
                                             c->msf_partials, means, values, c->stream);
        return ssim_hip::launch_msssim3hk(pd0, pd, n, W, H, D, scales, sample_type(sampleType), range, win.radius, win.gf, w, c->cu_count,
                                          c->msf_partials, means, values, c->stream);
    }
    hipError_t backward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, const uint8_t* grads, uint32_t n, uint32_t W, uint32_t H, uint32_t D,
                        uint32_t scales, const double* w, const double* means, const float* g_out, int which) const
    {
        const Pair3HDesc* pd0 = reinterpret_cast<const Pair3HDesc*>(pairs);
        const Pair3FDesc* pd = reinterpret_cast<const Pair3FDesc*>(pairs + n * kPair0);
        const Grad3HDesc* gd0 = reinterpret_cast<const Grad3HDesc*>(grads);
        const Grad3FDesc* gd = reinterpret_cast<const Grad3FDesc*>(grads + n * kGrad0);
        if (win.radius == 5)
            return ssim_hip::launch_msssim3h_grad(pd0, pd, gd0, gd, n, W, H, D, scales, sample_type(sampleType), range, win.radius, win.gf, w, c->cu_count,
                                                  means, g_out, c->msf_coef, c->s3_coef, which, c->stream);
        return ssim_hip::launch_msssim3hk_grad(pd0, pd, gd0, gd, n, W, H, D, scales, sample_type(sampleType), range, win.radius, win.gf, w, c->cu_count,
                                               means, g_out, c->msf_coef, c->s3_coef, which, c->stream);
    }
};

// Every check the multi-scale entries share: the single-scale checks of the call and its pairs, a non-NULL map refused with them, then
// scales and weights, then the launch limit.
template <typename M>
int ms_validate(const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales, const double* weights, const void* out)
{
    const int rc = validate_pairs<typename M::Single>(fam, count, params, out, true);
    if (rc) return rc;
    if (scales < 1 || scales > RMGR_SSIM_HIP_MSSSIM_MAX_SCALES) return EINVAL;
    if (weights == NULL) {
        if (scales != 5) return EINVAL;
    } else {
        for (uint32_t s = 0; s < scales; ++s)
            if (!std::isfinite(weights[s]) || weights[s] < 0.0) return EINVAL;
    }
    return ssim_hip::msssim3f_max_count(params[0].width, params[0].height, params[0].depth) == 0 ? EINVAL : 0;
}

// Fills rows 1 .. scales-1 of table[scale][pair] (scales x n; row 0 is the caller's to write): dense volumes of `pyramid`, scale by
// scale, A then B of each pair.
void fill_coarse(Pair3FDesc* table, uint32_t n, uint32_t W, uint32_t H, uint32_t D, uint32_t scales, float* pyramid)
{
    float* at = pyramid;
    for (uint32_t s = 1; s < scales; ++s) {
        const uint64_t voxels = ssim_hip::ms3_voxels(W, H, D, s);
        const int64_t stride = ssim_hip::ms3_dim(W, s), slice = stride * (int64_t)ssim_hip::ms3_dim(H, s);
        for (uint32_t i = 0; i < n; ++i) {
            Pair3FDesc& t = table[(size_t)s * n + i];
            t.a = at; t.a_step = 1; t.a_stride = stride; t.a_slice = slice; at += voxels;
            t.b = at; t.b_step = 1; t.b_stride = stride; t.b_slice = slice; at += voxels;
            t.map = NULL; t.map_step = t.map_stride = t.map_slice = 0;
        }
    }
}

// The same for the gradient table: dense volumes of `grads`, scale by scale, dA (with_a) then dB (with_b) of each pair.
void fill_coarse_grads(Grad3FDesc* table, uint32_t n, uint32_t W, uint32_t H, uint32_t D, uint32_t scales, float* grads, bool with_a, bool with_b)
{
    float* at = grads;
    for (uint32_t s = 1; s < scales; ++s) {
        const uint64_t voxels = ssim_hip::ms3_voxels(W, H, D, s);
        const int64_t stride = ssim_hip::ms3_dim(W, s), slice = stride * (int64_t)ssim_hip::ms3_dim(H, s);
        for (uint32_t i = 0; i < n; ++i) {
            Grad3FDesc g = {NULL, 0, 0, 0, NULL, 0, 0, 0};
            if (with_a) { g.ga = at; g.ga_step = 1; g.ga_stride = stride; g.ga_slice = slice; at += voxels; }
            if (with_b) { g.gb = at; g.gb_step = 1; g.gb_stride = stride; g.gb_slice = slice; at += voxels; }
            table[(size_t)s * n + i] = g;
        }
    }
}

// Enqueues the forward of n pairs (scale-0 descriptors without maps in host memory, volumes on the device): n x scales x 2 means and n
// values into device memory.
template <typename M>
int ms_enqueue(rmgr_ssim_hip_Context* c, const M& fam, uint32_t n, const typename M::Single::Desc* d, uint32_t W, uint32_t H, uint32_t D,
               uint32_t scales, const double* w, double* means, double* values)
{
    int rc;
    if ((rc = c->msf_pyramid.grow((size_t)(2 * ssim_hip::ms3_pyramid_floats(W, H, D, scales) * n)))) return rc;
    if ((rc = c->msf_partials.grow((size_t)ssim_hip::ms3_partials(W, H, D, n, scales)))) return rc;
    return ring_launch(c, n * M::kPair0 + (size_t)scales * n * sizeof(Pair3FDesc),
        [&](uint8_t* pin) {
            Pair3FDesc* table = reinterpret_cast<Pair3FDesc*>(pin + n * M::kPair0);
            if (M::kPair0) memset(table, 0, n * sizeof(Pair3FDesc));
            memcpy(pin, d, n * sizeof(*d));
            fill_coarse(table, n, W, H, D, scales, c->msf_pyramid);
        },
        [&](const uint8_t* dev) { return fam.forward(c, dev, n, W, H, D, scales, w, means, values); });
}

// Every sub-batch of the forward into values[0 .. count-1] and means[count x scales x 2] (device).  stage: host pointers -- each
// sub-batch's volumes are copied (each volume's sample range) into c->stage_a first.
template <typename M>
int ms_forward(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales, const double* w,
               double* means, double* values, bool stage)
{
    typedef typename M::Single F;
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const uint32_t per = ssim_hip::msssim3f_per_sub_batch(W, H, D, scales, 0, kScratchCap);
    const uint64_t scratch = ssim_hip::msssim3f_scratch_bytes(W, H, D, scales, 0);
    int rc;
    try {
        std::vector<typename F::Desc> d;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged, off = 0;
            const uint32_t n = take3f(params, i0, count, per, scratch, stage, staged);
            if (stage && (rc = c->stage_a.grow((size_t)staged))) return rc;
            d.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                d[i] = make_desc<F>(params[i0 + i], false);
                if (stage && (rc = stage_volumes<F>(c, params[i0 + i], d[i], off))) return rc;
            }
            if ((rc = ms_enqueue(c, fam, n, &d[0], W, H, D, scales, w, means + (size_t)i0 * scales * 2, values + i0))) return rc;
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    return 0;
}

// The blocking entry points: every sub-batch into c->msf_out (count values, then count x scales x 2 means), one copy back, one wait.
template <typename M>
int ms_blocking(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales, const double* w,
                float* msssim, double* scaleMeans, bool stage)
{
    const size_t total = (1 + 2 * (size_t)scales) * count;
    int rc;
    if ((rc = c->msf_out.grow(total))) return rc;
    if ((rc = c->msf_out_pin.grow(total))) return rc;
    if ((rc = ms_forward(c, fam, count, params, scales, w, c->msf_out + count, c->msf_out, stage))) return rc;
    HIP_TRY(hipMemcpyAsync(c->msf_out_pin, c->msf_out, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < count; ++i) msssim[i] = (float)c->msf_out_pin[i];
    if (scaleMeans) memcpy(scaleMeans, c->msf_out_pin + count, (size_t)count * scales * 2 * sizeof(double));
    return 0;
}

// What the three forward entries do once ms_validate has passed.
template <typename M>
int ms_enqueue_entry(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales,
                     const double* weights, double* valuesDevice, double* scaleMeansDevice)
{
    if (scaleMeansDevice == NULL || !c) return EINVAL;
    USE_DEVICE(c);
    return ms_forward(c, fam, count, params, scales, weights ? weights : kWangWeights, scaleMeansDevice, valuesDevice, false);
}

template <typename M>
int ms_device_entry(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales,
                    const double* weights, float* msssim, double* scaleMeans)
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return ms_blocking(c, fam, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, false);
}

template <typename M>
int ms_host_entry(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales,
                  const double* weights, float* msssim, double* scaleMeans)
{
    Lease lease;                         // ctx == NULL: one of the default contexts, for this call only
    const int rc = lease.take(c);
    if (rc) return rc;
    USE_DEVICE(lease.c);
    return ms_blocking(lease.c, fam, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, true);
}

// The gradient entry once ms_validate has passed.  Per sub-batch: the coefficients k_s, the pyramid again, then from the coarsest scale
// down the walk that writes the coefficient volumes into c->s3_coef (sized for scale 0, reused by every scale) and the adjoint walk, the
// caller's gradient volumes (float32, or the samples' encoding) at scale 0 and dense float32 scratch volumes below.
template <typename M>
int ms_grad_entry(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales,
                  const double* weights, const double* scaleMeansDevice, const float* gradOutDevice, const typename M::Single::Grad* gradA,
                  const typename M::Single::Grad* gradB)
{
    typedef typename M::Single F;
    int rc;
    if (scaleMeansDevice == NULL) return EINVAL;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const int which = grad_which(gradA, gradB), planes = (gradA ? 1 : 0) + (gradB ? 1 : 0);
    const uint64_t pyr = ssim_hip::ms3_pyramid_floats(W, H, D, scales);
    const uint64_t coef_per_volume = (uint64_t)ssim_hip::ssim3f_coef_planes(which) * W * H * D;
    const uint32_t per = ssim_hip::msssim3f_per_sub_batch(W, H, D, scales, planes, kScratchCap);
    const uint64_t scratch = ssim_hip::msssim3f_scratch_bytes(W, H, D, scales, planes);
    const double* w = weights ? weights : kWangWeights;
    for (uint32_t i0 = 0; i0 < count;) {
        uint64_t staged;
        const uint32_t n = take3f(params, i0, count, per, scratch, false, staged);
        if ((rc = c->msf_pyramid.grow((size_t)(2 * pyr * n)))) return rc;
        if ((rc = c->msf_grads.grow((size_t)((uint64_t)planes * pyr * n)))) return rc;
        if ((rc = c->msf_coef.grow((size_t)n * scales))) return rc;
        if ((rc = c->s3_coef.grow((size_t)(coef_per_volume * n)))) return rc;
        const size_t pair_bytes = n * M::kPair0 + (size_t)scales * n * sizeof(Pair3FDesc);
        const size_t grad_bytes = n * M::kGrad0 + (size_t)scales * n * sizeof(Grad3FDesc);
        rc = ring_launch(c, pair_bytes + grad_bytes,
            [&](uint8_t* pin) {
                typename F::Desc* pd0 = reinterpret_cast<typename F::Desc*>(pin);
                typename F::GradDesc* gd0 = reinterpret_cast<typename F::GradDesc*>(pin + pair_bytes);
                Pair3FDesc* pd = reinterpret_cast<Pair3FDesc*>(pin + n * M::kPair0);
                Grad3FDesc* gd = reinterpret_cast<Grad3FDesc*>(pin + pair_bytes + n * M::kGrad0);
                if (M::kPair0) memset(pd, 0, n * sizeof(Pair3FDesc));
                if (M::kGrad0) memset(gd, 0, n * sizeof(Grad3FDesc));
                for (uint32_t i = 0; i < n; ++i) {
                    pd0[i] = make_desc<F>(params[i0 + i], false);
                    gd0[i] = make_grad_desc<F>(gradA, gradB, i0 + i);
                }
                fill_coarse(pd, n, W, H, D, scales, c->msf_pyramid);
                fill_coarse_grads(gd, n, W, H, D, scales, c->msf_grads, gradA != NULL, gradB != NULL);
            },
            [&](const uint8_t* dev) {
                return fam.backward(c, dev, dev + pair_bytes, n, W, H, D, scales, w, scaleMeansDevice + (size_t)i0 * scales * 2, gradOutDevice + i0, which);
            });
        if (rc) return rc;
        i0 += n;
    }
    return 0;
}

} // namespace

extern "C" {

// ---- SSIM of float32 volumes, its gradient and the gradient of its map ---------------------------------------------------------------------
// Every entry exists twice: under the engine's window and, _win, under the caller's (include/rmgr/ssim-hip.h: rmgr_ssim_hip_Window).
// Both run the same flow; the window is one more input of the family.

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                          float dataRange, double* sumsDevice) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, sumsDevice);
    return rc ? rc : enqueue_entry(c, fam, count, params, NULL, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                              float dataRange, const rmgr_ssim_hip_Window* window, double* sumsDevice) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, sumsDevice);
    return rc ? rc : enqueue_entry(c, fam, count, params, window, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                 float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : device_entry(c, fam, count, params, NULL, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                     float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : device_entry(c, fam, count, params, window, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                               float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : host_entry(c, fam, count, params, NULL, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : host_entry(c, fam, count, params, window, ssim);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                               float dataRange, const float* gradOutDevice,
                                               const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, gradOutDevice);
    return rc ? rc : grad_entry_checked(c, fam, count, params, NULL, gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_Window* window, const float* gradOutDevice,
                                                   const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, gradOutDevice);
    return rc ? rc : grad_entry_checked(c, fam, count, params, window, gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                   const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, gradOutMaps);
    return rc ? rc : grad_entry_checked(c, fam, count, params, NULL, NULL, gradOutMaps, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                       float dataRange, const rmgr_ssim_hip_Window* window, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                       const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const Family3F fam = {dataRange};
    const int rc = validate(fam, count, params, gradOutMaps);
    return rc ? rc : grad_entry_checked(c, fam, count, params, window, NULL, gradOutMaps, gradA, gradB);
}

// ---- SSIM of float16 / bfloat16 volumes: the same ten entries, with the sample type ---------------------------------------------------------

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                          rmgr_uint32_t sampleType, float dataRange, double* sumsDevice) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, sumsDevice);
    return rc ? rc : enqueue_entry(c, fam, count, params, NULL, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                              rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                              double* sumsDevice) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, sumsDevice);
    return rc ? rc : enqueue_entry(c, fam, count, params, window, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : device_entry(c, fam, count, params, NULL, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                     rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                     float* ssim) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : device_entry(c, fam, count, params, window, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                               rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : host_entry(c, fam, count, params, NULL, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                   float* ssim) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, ssim);
    return rc ? rc : host_entry(c, fam, count, params, window, ssim);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                               rmgr_uint32_t sampleType, float dataRange, const float* gradOutDevice,
                                               const rmgr_ssim_hip_Grad3H* gradA, const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, gradOutDevice);
    return rc ? rc : grad_entry_checked(c, fam, count, params, NULL, gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                   const float* gradOutDevice, const rmgr_ssim_hip_Grad3H* gradA,
                                                   const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, gradOutDevice);
    return rc ? rc : grad_entry_checked(c, fam, count, params, window, gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                   const rmgr_ssim_hip_Grad3H* gradA, const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, gradOutMaps);
    return rc ? rc : grad_entry_checked(c, fam, count, params, NULL, NULL, gradOutMaps, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_win_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                       rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                       const rmgr_ssim_hip_GradOut3F* gradOutMaps, const rmgr_ssim_hip_Grad3H* gradA,
                                                       const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT
{
    const Family3H fam = {sampleType, dataRange};
    const int rc = validate(fam, count, params, gradOutMaps);
    return rc ? rc : grad_entry_checked(c, fam, count, params, window, NULL, gradOutMaps, gradA, gradB);
}

// ---- multi-scale SSIM of float32 volumes and its gradient ---------------------------------------------------------------------------------------

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                            rmgr_uint32_t scales, const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    const Multi3F fam = {dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    return rc ? rc : ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                                   rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const Multi3F fam = {dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                                 rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const Multi3F fam = {dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                                 rmgr_uint32_t scales, const double* weights, const double* scaleMeansDevice,
                                                 const float* gradOutDevice, const rmgr_ssim_hip_Grad3F* gradA,
                                                 const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    const Multi3F fam = {dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    return rc ? rc : ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

// ---- multi-scale SSIM of float16 / bfloat16 volumes and its gradient: the same four entries, with the sample type ---------------------------

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                            rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                            double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    const Multi3H fam = {sampleType, dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    return rc ? rc : ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                   float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const Multi3H fam = {sampleType, dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                 float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const Multi3H fam = {sampleType, dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                 const double* scaleMeansDevice, const float* gradOutDevice, const rmgr_ssim_hip_Grad3H* gradA,
                                                 const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT
{
    const Multi3H fam = {sampleType, dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    return rc ? rc : ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

// ---- the same under the caller's window: both run the same flow; the window is one more input of the family -------------------------------
// The checks of the entry without _win come first (sample type, data range, pairs, scales, weights), then the window, then the remaining
// pointers; all of them before the context or any device is touched.

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    Multi3F fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                       float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                       const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    Multi3F fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                     float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                     const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    Multi3F fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                     float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                     const double* weights, const double* scaleMeansDevice, const float* gradOutDevice,
                                                     const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    Multi3F fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    Multi3H fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                       rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                       const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    Multi3H fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                     rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                     const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    Multi3H fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                     rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                     const double* weights, const double* scaleMeansDevice, const float* gradOutDevice,
                                                     const rmgr_ssim_hip_Grad3H* gradA, const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT
{
    Multi3H fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

} // extern "C"
