// ssim_samples_abi.cpp -- the entry points of the C ABI for samples other than 8-bit ones (the 8-bit path: ssim_hip_abi.cpp): SSIM of
// 9- to 16-bit integers (ssim16), of float32 (ssimf) and of float16 / bfloat16 samples (ssimh), the gradients of the latter two for a
// scalar and for a per-pixel upstream gradient (ssimw), and multi-scale SSIM of float32 (msssimf) and of float16 / bfloat16 samples
// (msssimh) with its gradient.  The definitions are in include/rmgr/ssim-hip.h, the kernels in ssim16_ / ssimf_ / ssimh_ / ssimw_ /
// ssimk_ / ssimhk_ / msssimf_ / msssimh_ / msssimk_ / msssimhk_kernels.hip.
//
// The three single-scale families differ in their sample type and in what a launch is told (bit depth; data range; encoding and data
// range); each is described once by a small struct (Family16 / FamilyF / FamilyH) and the host flow -- validation, sub-batches, staging
// of host images, enqueue, strided map copy-back -- is written once over it.  The multi-scale path uses the same pieces.
//
// Every pair's sum runs over fixed cells in a fixed order, every gradient pixel belongs to one fixed tile, and every pyramid plane, cell
// and tile of the multi-scale path belongs to one pair: neither the sub-batches (kScratchCap of partials, pyramids, staged images and
// maps per sub-batch) nor the launch a pair lands in change a bit.
//
// Every family runs on one ring of descriptor tables, one buffer of cell partials and one of pinned sums (sf_slots, sf_partials,
// sf_sums_pin of the context): one stream, stream order.  An enqueue form therefore never waits for the host, except -- at most -- for
// the launch that read its ring slot kSfSlots enqueues ago.
#include "ssim_flow.h"
#include "msssimh_kernels.h"
#include "msssimk_kernels.h"
#include "ssimhk_kernels.h"
#include "ssimw_kernels.h"

using namespace ssim_host;

namespace {

using ssim_hip::Pair16Desc;
using ssim_hip::PairFDesc;
using ssim_hip::GradFDesc;
using ssim_hip::PairHDesc;
using ssim_hip::GradHDesc;
using ssim_hip::GradOutFDesc;

// ---- the families ------------------------------------------------------------------------------------------------------------------------------
// Params / Desc / Sample: the public parameter block, the kernels' descriptor of a pair, the type of a sample.  launch() enqueues the
// strip kernel and the reduction of geo.count pairs into sums (device or pinned host memory); the per-call arguments are its members.

struct Family16 {
    typedef rmgr_ssim_hip_Params16 Params;
    typedef Pair16Desc Desc;
    typedef uint16_t Sample;
    typedef ssim_hip::Geometry16 Geometry;
    static constexpr uint32_t kMaxDim = ssim_hip::kS16MaxDim;
    static uint32_t max_count(uint32_t W, uint32_t H) { return ssim_hip::ssim16_max_count(W, H); }
    static Geometry plan(uint32_t W, uint32_t H, uint32_t n, int cus) { return ssim_hip::plan16(W, H, n, cus); }
    static bool fits_narrow(const Desc& d) { return ssim_hip::fits16_narrow(d); }
    uint32_t depth;
    hipError_t launch(rmgr_ssim_hip_Context* c, const Geometry& geo, const Desc* dev, bool map, bool unit, bool wide, double* sums) const
    { return ssim_hip::launch_ssim16(geo, dev, map, unit, wide, depth, c->xcd_count, c->sf_partials, sums, c->stream); }
};

struct FamilyF {
    typedef rmgr_ssim_hip_ParamsF Params;
    typedef rmgr_ssim_hip_GradF Grad;
    typedef PairFDesc Desc;
    typedef GradFDesc GradDesc;
    typedef float Sample;
    typedef ssim_hip::GeometryF Geometry;
    static constexpr uint32_t kMaxDim = ssim_hip::kSFMaxDim;
    static uint32_t max_count(uint32_t W, uint32_t H) { return ssim_hip::ssimf_max_count(W, H); }
    static Geometry plan(uint32_t W, uint32_t H, uint32_t n, int cus) { return ssim_hip::planf(W, H, n, cus); }
    static bool fits_narrow(const Desc& d) { return ssim_hip::fitsf_narrow(d); }
    float range;
    Window win;
    // geo is planf()'s: the cells (and with them the partials) are the same for every radius; a smaller window re-plans its strips, which
    // pay fewer warm-up rows
    hipError_t launch(rmgr_ssim_hip_Context* c, const Geometry& geo, const Desc* dev, bool map, bool unit, bool wide, double* sums) const
    {
        if (win.radius == 5)
            return ssim_hip::launch_ssimf(geo, dev, map, unit, wide, range, win.gf, c->xcd_count, c->sf_partials, sums, c->stream);
        return ssim_hip::launch_ssimk(win.radius, win.gf, ssim_hip::plank(win.radius, geo.width, geo.height, geo.count, c->cu_count), dev, map, wide,
                                      range, c->xcd_count, c->sf_partials, sums, c->stream);
    }
};

struct FamilyH {
    typedef rmgr_ssim_hip_Params16 Params;
    typedef rmgr_ssim_hip_GradH Grad;
    typedef PairHDesc Desc;
    typedef GradHDesc GradDesc;
    typedef uint16_t Sample;
    typedef ssim_hip::GeometryH Geometry;
    static constexpr uint32_t kMaxDim = ssim_hip::kSHMaxDim;
    static uint32_t max_count(uint32_t W, uint32_t H) { return ssim_hip::ssimh_max_count(W, H); }
    static Geometry plan(uint32_t W, uint32_t H, uint32_t n, int cus) { return ssim_hip::planh(W, H, n, cus); }
    static bool fits_narrow(const Desc& d) { return ssim_hip::fitsh_narrow(d); }
    int type;           // kSHTypeF16 / kSHTypeBF16
    float range;
    Window win;
    // as FamilyF::launch: geo is planh()'s, a smaller window re-plans its strips
    hipError_t launch(rmgr_ssim_hip_Context* c, const Geometry& geo, const Desc* dev, bool map, bool unit, bool wide, double* sums) const
    {
        if (win.radius == 5)
            return ssim_hip::launch_ssimh(geo, dev, type, map, unit, wide, range, win.gf, c->xcd_count, c->sf_partials, sums, c->stream);
        return ssim_hip::launch_ssimhk(win.radius, win.gf, ssim_hip::plank(win.radius, geo.width, geo.height, geo.count, c->cu_count), dev, type, map,
                                       wide, range, c->xcd_count, c->sf_partials, sums, c->stream);
    }
};

// ---- validation, before any device is touched -----------------------------------------------------------------------------------------------

// What every entry point checks of its pairs; `out` is whichever output the entry requires.
template <typename F>
int validate_pairs(uint32_t count, const typename F::Params* params, const void* out)
{
    if (count == 0 || params == NULL || out == NULL) return EINVAL;
    const uint32_t W = params[0].width, H = params[0].height;
    if (W == 0 || H == 0 || W > F::kMaxDim || H > F::kMaxDim) return EINVAL;
    const uintptr_t mask = sizeof(typename F::Sample) - 1;
    for (uint32_t i = 0; i < count; ++i) {
        const typename F::Params& p = params[i];
        if (p.width != W || p.height != H) return EINVAL;
        if (p.imgA.topLeft == NULL || p.imgB.topLeft == NULL) return EINVAL;
        if (((uintptr_t)p.imgA.topLeft & mask) || ((uintptr_t)p.imgB.topLeft & mask)) return EINVAL;
    }
    if (F::max_count(W, H) == 0) return EINVAL;
    return 0;
}

int ssim16_validate(uint32_t count, const rmgr_ssim_hip_Params16* params, uint32_t bitDepth, const void* out)
{
    if (bitDepth < RMGR_SSIM_HIP_SSIM16_MIN_DEPTH || bitDepth > RMGR_SSIM_HIP_SSIM16_MAX_DEPTH) return EINVAL;
    return validate_pairs<Family16>(count, params, out);
}

int ssimf_validate(uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const void* out)
{
    if (!valid_range(dataRange)) return EINVAL;
    return validate_pairs<FamilyF>(count, params, out);
}

int ssimh_validate(uint32_t count, const rmgr_ssim_hip_Params16* params, uint32_t sampleType, float dataRange, const void* out)
{
    if (sampleType != RMGR_SSIM_HIP_SAMPLE_F16 && sampleType != RMGR_SSIM_HIP_SAMPLE_BF16) return EINVAL;
    if (!valid_range(dataRange)) return EINVAL;
    return validate_pairs<FamilyH>(count, params, out);
}

// The planes of a gradient entry: gradA and / or gradB, every plane non-NULL and aligned to its samples.
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
int validate_grad_maps(uint32_t count, const rmgr_ssim_hip_GradOutF* maps)
{
    for (uint32_t i = 0; i < count; ++i)
        if (maps[i].topLeft == NULL || ((uintptr_t)maps[i].topLeft & 3u)) return EINVAL;
    return 0;
}

// ---- descriptors ---------------------------------------------------------------------------------------------------------------------------------

template <typename F>
typename F::Desc make_desc(const typename F::Params& p, bool with_map)
{
    typename F::Desc d;
    d.a = p.imgA.topLeft; d.a_step = p.imgA.step; d.a_stride = p.imgA.stride;
    d.b = p.imgB.topLeft; d.b_step = p.imgB.step; d.b_stride = p.imgB.stride;
    const bool m = with_map && p.ssimMap;
    d.map = m ? p.ssimMap : NULL;
    d.map_step = m ? p.ssimStep : 0;
    d.map_stride = m ? p.ssimStride : 0;
    return d;
}

// The gradient planes of pair i: those of gradA / gradB that the caller wants.
template <typename F>
typename F::GradDesc make_grad_desc(const typename F::Grad* gradA, const typename F::Grad* gradB, uint32_t i)
{
    typename F::GradDesc g = {NULL, 0, 0, NULL, 0, 0};
    if (gradA) { g.ga = gradA[i].topLeft; g.ga_step = gradA[i].step; g.ga_stride = gradA[i].stride; }
    if (gradB) { g.gb = gradB[i].topLeft; g.gb_step = gradB[i].step; g.gb_stride = gradB[i].stride; }
    return g;
}

template <typename G> int grad_which(const G* gradA, const G* gradB) { return (gradA ? 1 : 0) | (gradB ? 2 : 0); }

GradOutFDesc make_gout(const rmgr_ssim_hip_GradOutF& m)
{
    const GradOutFDesc o = {m.topLeft, (int64_t)m.step, (int64_t)m.stride};
    return o;
}

// ---- sub-batches and staging -------------------------------------------------------------------------------------------------------------------

// The bytes of the sample range of a width x height image; lo: where the range starts, in samples relative to topLeft (<= 0).
template <typename F, typename Img>
size_t image_bytes(const Img& im, uint32_t w, uint32_t h, int64_t& lo)
{
    const int64_t dx = (int64_t)(w - 1) * (int64_t)im.step, dy = (int64_t)(h - 1) * (int64_t)im.stride;
    lo = (dx < 0 ? dx : 0) + (dy < 0 ? dy : 0);
    const int64_t hi = (dx > 0 ? dx : 0) + (dy > 0 ? dy : 0);
    return (size_t)(hi - lo + 1) * sizeof(typename F::Sample);
}

template <typename F> uint64_t partials_per_pair(uint32_t W, uint32_t H) { return F::plan(W, H, 1, 0).cells_per_image() * sizeof(double); }

// Pairs of params[i0 ..] that one sub-batch takes: at least one; at most nmax (the launch limit) and, with `scratch` bytes per pair and
// -- stage: host pointers -- the staged images (with_maps: and maps) of each pair, kScratchCap of device scratch.  staged: the bytes
// its staged images and maps take, each rounded up to 64.
template <typename F>
uint32_t take(const typename F::Params* params, uint32_t i0, uint32_t count, uint32_t nmax, uint64_t scratch, bool stage, bool with_maps,
              uint64_t& staged)
{
    const uint32_t W = params[0].width, H = params[0].height;
    uint32_t n = 0;
    staged = 0;
    while (i0 + n < count && n < nmax) {
        uint64_t bytes = 0;
        if (stage) {
            const typename F::Params& p = params[i0 + n];
            int64_t lo;
            bytes += round64(image_bytes<F>(p.imgA, W, H, lo)) + round64(image_bytes<F>(p.imgB, W, H, lo));
            if (with_maps && p.ssimMap) bytes += round64((uint64_t)W * H * 4);
        }
        if (n > 0 && scratch * (n + 1) + staged + bytes > kScratchCap) break;
        staged += bytes;
        ++n;
    }
    return n;
}

// Host pointers: copies the sample range of both images of p to c->stage_a + off (off moves on, in steps of 64) on the context's stream
// and points d at the copies.
template <typename F>
int stage_images(rmgr_ssim_hip_Context* c, const typename F::Params& p, uint32_t W, uint32_t H, typename F::Desc& d, uint64_t& off)
{
    for (int k = 0; k < 2; ++k) {
        const auto& im = k ? p.imgB : p.imgA;
        int64_t lo;
        const size_t bytes = image_bytes<F>(im, W, H, lo);
        HIP_TRY(hipMemcpyAsync(c->stage_a + off, im.topLeft + lo, bytes, hipMemcpyHostToDevice, c->stream));
        (k ? d.b : d.a) = reinterpret_cast<const typename F::Sample*>(c->stage_a + off) - lo;
        off += round64(bytes);
    }
    return 0;
}

// Copies a dense W x H map in device memory to the caller's map at its own step and stride (blocking).
int copy_map_back(const float* src, float* map, ptrdiff_t step, ptrdiff_t stride, uint32_t W, uint32_t H, std::vector<float>& back)
{
    if (step == 1 && stride == (ptrdiff_t)W) {
        HIP_TRY(hipMemcpy(map, src, (size_t)W * H * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    back.resize((size_t)W * H);
    HIP_TRY(hipMemcpy(&back[0], src, (size_t)W * H * 4, hipMemcpyDeviceToHost));
    for (uint32_t y = 0; y < H; ++y) {
        float* row = map + (ptrdiff_t)y * stride;
        const float* s = &back[(size_t)y * W];
        for (uint32_t x = 0; x < W; ++x) row[(ptrdiff_t)x * step] = s[x];
    }
    return 0;
}

// ---- the forward flow -----------------------------------------------------------------------------------------------------------------------------

// Enqueues n pairs (descriptors in host memory, images on the device) on the context's stream: descriptor upload, strip kernel,
// reduction into sums[0 .. n-1] (device or pinned host memory).  n <= F::max_count and its partials within the cap.
template <typename F>
int enqueue_pairs(rmgr_ssim_hip_Context* c, const F& fam, uint32_t n, const typename F::Desc* d, uint32_t W, uint32_t H, double* sums)
{
    typedef typename F::Desc Desc;
    const typename F::Geometry geo = F::plan(W, H, n, c->cu_count);
    int rc;
    if ((rc = c->sf_partials.grow((size_t)(geo.cells_per_image() * n)))) return rc;
    bool map = false, unit = (W % 2) == 0, wide = false;
    for (uint32_t i = 0; i < n; ++i) {
        map = map || d[i].map != NULL;
        unit = unit && (d[i].map == NULL || d[i].map_step == 1);
        wide = wide || !F::fits_narrow(d[i]);
    }
    return ring_launch(c, n * sizeof(Desc),
        [&](uint8_t* pin) { memcpy(pin, d, n * sizeof(Desc)); },
        [&](const uint8_t* dev) { return fam.launch(c, geo, reinterpret_cast<const Desc*>(dev), map, unit, wide, sums); });
}

// The enqueue entry points: every sub-batch of device-resident pairs into sums[0 .. count-1] (device), no host synchronisation.
template <typename F>
int enqueue_all(rmgr_ssim_hip_Context* c, const F& fam, uint32_t count, const typename F::Params* params, double* sums)
{
    const uint32_t W = params[0].width, H = params[0].height;
    try {
        std::vector<typename F::Desc> d;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged;
            const uint32_t n = take<F>(params, i0, count, F::max_count(W, H), partials_per_pair<F>(W, H), false, false, staged);
            d.resize(n);
            for (uint32_t i = 0; i < n; ++i) d[i] = make_desc<F>(params[i0 + i], true);
            const int rc = enqueue_pairs(c, fam, n, &d[0], W, H, sums + i0);
            if (rc) return rc;
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    return 0;
}

// The blocking entry points: every sub-batch into the pinned sums, then the means.  stage: host pointers -- the images are copied
// (each image's sample range) into c->stage_a, a pair's map is written densely into it as well and copied back at its own step and stride.
template <typename F>
int blocking(rmgr_ssim_hip_Context* c, const F& fam, uint32_t count, const typename F::Params* params, float* ssim, bool stage)
{
    const uint32_t W = params[0].width, H = params[0].height;
    const double px = (double)W * (double)H;
    int rc;
    if ((rc = c->sf_sums_pin.grow(count))) return rc;
    try {
        std::vector<typename F::Desc> d;
        std::vector<uint64_t> map_off;
        std::vector<float> back;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged;
            const uint32_t n = take<F>(params, i0, count, F::max_count(W, H), partials_per_pair<F>(W, H), stage, true, staged);
            d.resize(n);
            map_off.assign(n, 0);
            if (stage && (rc = c->stage_a.grow((size_t)staged))) return rc;
            uint64_t off = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const typename F::Params& p = params[i0 + i];
                d[i] = make_desc<F>(p, true);
                if (!stage) continue;
                if ((rc = stage_images<F>(c, p, W, H, d[i], off))) return rc;
                if (p.ssimMap) {
                    map_off[i] = off;
                    d[i].map = reinterpret_cast<float*>(c->stage_a + off);
                    d[i].map_step = 1; d[i].map_stride = W;
                    off += round64((uint64_t)W * H * 4);
                }
            }
            if ((rc = enqueue_pairs(c, fam, n, &d[0], W, H, c->sf_sums_pin + i0))) return rc;
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (uint32_t i = 0; i < n && stage; ++i) {
                const typename F::Params& p = params[i0 + i];
                if (!p.ssimMap) continue;
                const float* src = reinterpret_cast<const float*>(c->stage_a + map_off[i]);
                if ((rc = copy_map_back(src, p.ssimMap, p.ssimStep, p.ssimStride, W, H, back))) return rc;
            }
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    for (uint32_t i = 0; i < count; ++i) ssim[i] = (float)(c->sf_sums_pin[i] / px);
    return 0;
}

// The blocking entry point of host pointers: ctx == NULL runs on one of the default contexts, for this call only.
template <typename F>
int blocking_host(rmgr_ssim_hip_Context* c, const F& fam, uint32_t count, const typename F::Params* params, float* ssim)
{
    Lease lease;
    int rc = lease.take(c);
    if (rc) return rc;
    USE_DEVICE(lease.c);
    return blocking(lease.c, fam, count, params, ssim, true);
}

// ---- the single-scale gradients -----------------------------------------------------------------------------------------------------------------

// The gradient entries of one scale: one fused launch per sub-batch of at most F::max_count pairs, without scratch.  Its ring slot holds
// the pair descriptors, the gradient descriptors and -- maps != NULL: the map gradient -- the descriptors of the upstream planes;
// launch(n, i0, pairs, grads, maps) enqueues the kernel on the device copies of the three tables.
template <typename F, typename Launch>
int enqueue_grads(rmgr_ssim_hip_Context* c, uint32_t count, const typename F::Params* params, const typename F::Grad* gradA,
                  const typename F::Grad* gradB, const rmgr_ssim_hip_GradOutF* maps, Launch launch)
{
    typedef typename F::Desc Desc;
    typedef typename F::GradDesc GradDesc;
    const uint32_t nmax = F::max_count(params[0].width, params[0].height);
    for (uint32_t i0 = 0; i0 < count;) {
        const uint32_t n = std::min(count - i0, nmax);
        const size_t pair_bytes = n * sizeof(Desc), grad_bytes = n * sizeof(GradDesc), bytes = pair_bytes + grad_bytes + (maps ? n * sizeof(GradOutFDesc) : 0);
        const int rc = ring_launch(c, bytes,
            [&](uint8_t* pin) {
                Desc* pd = reinterpret_cast<Desc*>(pin);
                GradDesc* gd = reinterpret_cast<GradDesc*>(pin + pair_bytes);
                GradOutFDesc* od = reinterpret_cast<GradOutFDesc*>(pin + pair_bytes + grad_bytes);
                for (uint32_t i = 0; i < n; ++i) {
                    pd[i] = make_desc<F>(params[i0 + i], false);
                    gd[i] = make_grad_desc<F>(gradA, gradB, i0 + i);
                    if (maps) od[i] = make_gout(maps[i0 + i]);
                }
            },
            [&](const uint8_t* dev) {
                return launch(n, i0, reinterpret_cast<const Desc*>(dev), reinterpret_cast<const GradDesc*>(dev + pair_bytes),
                              reinterpret_cast<const GradOutFDesc*>(dev + pair_bytes + grad_bytes));
            });
        if (rc) return rc;
        i0 += n;
    }
    return 0;
}

// ---- multi-scale SSIM of float32 and of float16 / bfloat16 samples ---------------------------------------------------------------------------
// Scale 0 is read where the caller has it; the planes of scales >= 1 (and, in the backward, their gradient planes) are dense float32
// planes of the context's scratch, one set per pair, rewritten by every sub-batch in stream order.  The two families differ in scale 0
// alone -- its samples, its descriptors and the kernels that read and write them -- and each is described by a small struct (MultiF /
// MultiH) over which the flow is written once.  The window, the engine's or the caller's (_win), is one more member of it: the same at
// every scale, and nothing of the flow -- pyramid, scratch, sub-batches, tables -- depends on it.
//
// A launch reads one table of pair descriptors, scales x n PairFDesc as [scale][pair] (rows >= 1: the pyramid), and -- backward -- one of
// gradient descriptors, scales x n GradFDesc.  MultiF: row 0 holds the caller's planes.  MultiH: row 0 is not read (zeroed), and the
// caller's n PairHDesc / GradHDesc follow the table.

struct MultiF {
    typedef FamilyF Single;
    float range;
    Window win;
    int validate(uint32_t count, const rmgr_ssim_hip_ParamsF* params, const void* out) const { return ssimf_validate(count, params, range, out); }
    static size_t pair_bytes(uint32_t scales, uint32_t n) { return (size_t)scales * n * sizeof(PairFDesc); }
    static size_t grad_bytes(uint32_t scales, uint32_t n) { return (size_t)scales * n * sizeof(GradFDesc); }
    // Where the n scale-0 descriptors of a table go.
    static PairFDesc* pairs0(uint8_t* table, uint32_t, uint32_t) { return reinterpret_cast<PairFDesc*>(table); }
    static GradFDesc* grads0(uint8_t* table, uint32_t, uint32_t) { return reinterpret_cast<GradFDesc*>(table); }
    hipError_t forward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, uint32_t n, uint32_t W, uint32_t H, uint32_t scales, bool wide, const double* w,
                       double* means, double* values) const
    {
        // as FamilyF::launch: windows of 11 taps on the kernels of msssimf_kernels.hip, smaller ones on kernels of their radius
        return (win.radius == 5 ? ssim_hip::launch_msssimf_from : ssim_hip::launch_msssimk_from)(
            0, win.radius, win.gf, reinterpret_cast<const PairFDesc*>(pairs), n, W, H, scales, wide, range, w, c->cu_count, c->xcd_count, c->msf_partials,
            means, values, c->stream);
    }
    hipError_t backward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, const uint8_t* grads, uint32_t n, uint32_t W, uint32_t H, uint32_t scales,
                        const double* w, const double* means, const float* g_out, int which) const
    {
        return (win.radius == 5 ? ssim_hip::launch_msssimf_grad_from : ssim_hip::launch_msssimk_grad_from)(
            0, win.radius, win.gf, reinterpret_cast<const PairFDesc*>(pairs), reinterpret_cast<const GradFDesc*>(grads), n, W, H, scales, range, w, means,
            g_out, c->msf_coef, which, c->stream);
    }
};

struct MultiH {
    typedef FamilyH Single;
    uint32_t sampleType;
    float range;
    Window win;
    int validate(uint32_t count, const rmgr_ssim_hip_Params16* params, const void* out) const { return ssimh_validate(count, params, sampleType, range, out); }
    static size_t pair_bytes(uint32_t scales, uint32_t n) { return (size_t)scales * n * sizeof(PairFDesc) + n * sizeof(PairHDesc); }
    static size_t grad_bytes(uint32_t scales, uint32_t n) { return (size_t)scales * n * sizeof(GradFDesc) + n * sizeof(GradHDesc); }
    static PairHDesc* pairs0(uint8_t* table, uint32_t scales, uint32_t n)
    {
        memset(table, 0, n * sizeof(PairFDesc));
        return reinterpret_cast<PairHDesc*>(table + (size_t)scales * n * sizeof(PairFDesc));
    }
    static GradHDesc* grads0(uint8_t* table, uint32_t scales, uint32_t n)
    {
        memset(table, 0, n * sizeof(GradFDesc));
        return reinterpret_cast<GradHDesc*>(table + (size_t)scales * n * sizeof(GradFDesc));
    }
    hipError_t forward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, uint32_t n, uint32_t W, uint32_t H, uint32_t scales, bool wide, const double* w,
                       double* means, double* values) const
    {
        return (win.radius == 5 ? ssim_hip::launch_msssimh : ssim_hip::launch_msssimhk)(reinterpret_cast<const PairHDesc*>(pairs + (size_t)scales * n * sizeof(PairFDesc)),
                                        reinterpret_cast<const PairFDesc*>(pairs), n, W, H, scales, sample_type(sampleType), wide, range, win.radius,
                                        win.gf, w, c->cu_count, c->xcd_count, c->msf_partials, means, values, c->stream);
    }
    hipError_t backward(rmgr_ssim_hip_Context* c, const uint8_t* pairs, const uint8_t* grads, uint32_t n, uint32_t W, uint32_t H, uint32_t scales,
                        const double* w, const double* means, const float* g_out, int which) const
    {
        return (win.radius == 5 ? ssim_hip::launch_msssimh_grad : ssim_hip::launch_msssimhk_grad)(reinterpret_cast<const PairHDesc*>(pairs + (size_t)scales * n * sizeof(PairFDesc)),
                                             reinterpret_cast<const PairFDesc*>(pairs),
                                             reinterpret_cast<const GradHDesc*>(grads + (size_t)scales * n * sizeof(GradFDesc)),
                                             reinterpret_cast<const GradFDesc*>(grads), n, W, H, scales, sample_type(sampleType), range, win.radius, win.gf,
                                             w, means, g_out, c->msf_coef, which, c->stream);
    }
};

// Every check the entry points share.
template <typename M>
int ms_validate(const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales, const double* weights, const void* out)
{
    int rc = fam.validate(count, params, out);
    if (rc) return rc;
    if (scales < 1 || scales > RMGR_SSIM_HIP_MSSSIM_MAX_SCALES) return EINVAL;
    if (weights == NULL) {
        if (scales != 5) return EINVAL;
    } else {
        for (uint32_t s = 0; s < scales; ++s)
            if (!std::isfinite(weights[s]) || weights[s] < 0.0) return EINVAL;
    }
    for (uint32_t i = 0; i < count; ++i)
        if (params[i].ssimMap != NULL) return EINVAL;
    if (ssim_hip::msssimf_max_count(params[0].width, params[0].height) == 0) return EINVAL;
    return 0;
}

// Device scratch one pair needs: the pyramid of both images, grad_planes (0 forward, 1 or 2 backward) coarse gradient pyramids, its
// cell partials (forward) or coefficients (backward).  The same for both families: all of it is float32 / float64.
uint64_t msf_pair_bytes(uint32_t W, uint32_t H, uint32_t scales, int grad_planes)
{
    const uint64_t pyr = ssim_hip::msf_pyramid_floats(W, H, scales);
    return (2 + (uint64_t)grad_planes) * pyr * sizeof(float) +
           (grad_planes ? scales * sizeof(float) : ssim_hip::msf_partials(W, H, 1, scales) * sizeof(double));
}

// Pairs of params[i0 ..] one sub-batch takes (take() with a pair's multi-scale scratch; staged images count against the same cap).
template <typename M>
uint32_t msf_take(const typename M::Single::Params* params, uint32_t i0, uint32_t count, uint32_t scales, int grad_planes, bool stage, uint64_t& staged)
{
    const uint32_t W = params[0].width, H = params[0].height;
    return take<typename M::Single>(params, i0, count, ssim_hip::msssimf_max_count(W, H), msf_pair_bytes(W, H, scales, grad_planes), stage, false, staged);
}


// Fills rows 1 .. scales-1 of table[scale][pair] (scales x n; row 0 is the caller's to write): dense planes of `pyramid`, scale by
// scale, A then B of each pair.
void msf_fill_coarse(PairFDesc* table, uint32_t n, uint32_t W, uint32_t H, uint32_t scales, float* pyramid)
{
    float* at = pyramid;
    for (uint32_t s = 1; s < scales; ++s) {
        const uint64_t plane = ssim_hip::msf_plane(W, H, s);
        const int64_t stride = ssim_hip::msf_dim(W, s);
        for (uint32_t i = 0; i < n; ++i) {
            PairFDesc& t = table[(size_t)s * n + i];
            t.a = at; t.a_step = 1; t.a_stride = stride; at += plane;
            t.b = at; t.b_step = 1; t.b_stride = stride; at += plane;
            t.map = NULL; t.map_step = t.map_stride = 0;
        }
    }
}

// Enqueues the forward of n pairs (scale-0 descriptors without maps in host memory, images on the device) on the context's stream:
// n x scales x 2 means and n values into device memory.
template <typename M>
int ms_enqueue(rmgr_ssim_hip_Context* c, const M& fam, uint32_t n, const typename M::Single::Desc* d, uint32_t W, uint32_t H, uint32_t scales,
               const double* w, double* means, double* values)
{
    int rc;
    if ((rc = c->msf_pyramid.grow((size_t)(2 * ssim_hip::msf_pyramid_floats(W, H, scales) * n)))) return rc;
    if ((rc = c->msf_partials.grow((size_t)ssim_hip::msf_partials(W, H, n, scales)))) return rc;
    bool wide = false;
    for (uint32_t i = 0; i < n; ++i) wide = wide || !M::Single::fits_narrow(d[i]);
    return ring_launch(c, M::pair_bytes(scales, n),
        [&](uint8_t* pin) {
            memcpy(M::pairs0(pin, scales, n), d, n * sizeof(*d));
            msf_fill_coarse(reinterpret_cast<PairFDesc*>(pin), n, W, H, scales, c->msf_pyramid);
        },
        [&](const uint8_t* dev) { return fam.forward(c, dev, n, W, H, scales, wide, w, means, values); });
}

// Every sub-batch of the forward into values[0 .. count-1] and means[count x scales x 2] (device).  stage: host pointers -- each
// sub-batch's images are copied (each image's sample range) into c->stage_a first.
template <typename M>
int ms_forward(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales, const double* w,
               double* means, double* values, bool stage)
{
    typedef typename M::Single F;
    const uint32_t W = params[0].width, H = params[0].height;
    int rc;
    try {
        std::vector<typename F::Desc> d;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged, off = 0;
            const uint32_t n = msf_take<M>(params, i0, count, scales, 0, stage, staged);
            if (stage && (rc = c->stage_a.grow((size_t)staged))) return rc;
            d.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                d[i] = make_desc<F>(params[i0 + i], false);
                if (stage && (rc = stage_images<F>(c, params[i0 + i], W, H, d[i], off))) return rc;
            }
            if ((rc = ms_enqueue(c, fam, n, &d[0], W, H, scales, w, means + (size_t)i0 * scales * 2, values + i0))) return rc;
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
    int rc = lease.take(c);
    if (rc) return rc;
    USE_DEVICE(lease.c);
    return ms_blocking(lease.c, fam, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, true);
}

// The gradient entry, arguments valid: per sub-batch the coefficients, the pyramid again and the gradient kernels from the coarsest scale
// down, the caller's planes (float32, or the samples' encoding) at scale 0 and dense float32 scratch planes below.
template <typename M>
int ms_grad_entry(rmgr_ssim_hip_Context* c, const M& fam, uint32_t count, const typename M::Single::Params* params, uint32_t scales,
                  const double* weights, const double* scaleMeansDevice, const float* gradOutDevice, const typename M::Single::Grad* gradA,
                  const typename M::Single::Grad* gradB)
{
    typedef typename M::Single F;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    int rc;
    const uint32_t W = params[0].width, H = params[0].height;
    const int which = grad_which(gradA, gradB), planes = (gradA ? 1 : 0) + (gradB ? 1 : 0);
    const uint64_t pyr = ssim_hip::msf_pyramid_floats(W, H, scales);
    const double* w = weights ? weights : kWangWeights;
    for (uint32_t i0 = 0; i0 < count;) {
        uint64_t staged;
        const uint32_t n = msf_take<M>(params, i0, count, scales, planes, false, staged);
        if ((rc = c->msf_pyramid.grow((size_t)(2 * pyr * n)))) return rc;
        if ((rc = c->msf_grads.grow((size_t)((uint64_t)planes * pyr * n)))) return rc;
        if ((rc = c->msf_coef.grow((size_t)n * scales))) return rc;
        const size_t pair_bytes = M::pair_bytes(scales, n);
        rc = ring_launch(c, pair_bytes + M::grad_bytes(scales, n),
            [&](uint8_t* pin) {
                typename F::Desc* pd = M::pairs0(pin, scales, n);
                typename F::GradDesc* gd = M::grads0(pin + pair_bytes, scales, n);
                for (uint32_t i = 0; i < n; ++i) {
                    pd[i] = make_desc<F>(params[i0 + i], false);
                    gd[i] = make_grad_desc<F>(gradA, gradB, i0 + i);
                }
                msf_fill_coarse(reinterpret_cast<PairFDesc*>(pin), n, W, H, scales, c->msf_pyramid);
                // gradient planes of scales >= 1: dense scratch, scale by scale, dA then dB of each pair
                GradFDesc* coarse = reinterpret_cast<GradFDesc*>(pin + pair_bytes);
                float* at = c->msf_grads;
                for (uint32_t sc = 1; sc < scales; ++sc) {
                    const uint64_t plane = ssim_hip::msf_plane(W, H, sc);
                    const int64_t stride = ssim_hip::msf_dim(W, sc);
                    for (uint32_t i = 0; i < n; ++i) {
                        GradFDesc g = {NULL, 0, 0, NULL, 0, 0};
                        if (gradA) { g.ga = at; g.ga_step = 1; g.ga_stride = stride; at += plane; }
                        if (gradB) { g.gb = at; g.gb_step = 1; g.gb_stride = stride; at += plane; }
                        coarse[(size_t)sc * n + i] = g;
                    }
                }
            },
            [&](const uint8_t* dev) {
                return fam.backward(c, dev, dev + pair_bytes, n, W, H, scales, w, scaleMeansDevice + (size_t)i0 * scales * 2, gradOutDevice + i0, which);
            });
        if (rc) return rc;
        i0 += n;
    }
    return 0;
}

// ---- SSIM of float32 samples: what an entry does once its arguments are valid; `win` is the engine's window or the caller's ------------------

int ssimf_enqueue_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const Window& win,
                        double* sumsDevice)
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return enqueue_all(c, FamilyF{dataRange, win}, count, params, sumsDevice);
}

int ssimf_device_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const Window& win, float* ssim)
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return blocking(c, FamilyF{dataRange, win}, count, params, ssim, false);
}

// gradOutDevice: the scalar upstream form; gradOutMaps: the per-pixel form.  Exactly one is given.
int ssimf_grad_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const Window& win,
                     const float* gradOutDevice, const rmgr_ssim_hip_GradOutF* gradOutMaps, const rmgr_ssim_hip_GradF* gradA,
                     const rmgr_ssim_hip_GradF* gradB)
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    const uint32_t W = params[0].width, H = params[0].height;
    const int which = grad_which(gradA, gradB);
    return enqueue_grads<FamilyF>(c, count, params, gradA, gradB, gradOutMaps,
        [&](uint32_t n, uint32_t i0, const PairFDesc* pd, const GradFDesc* gd, const GradOutFDesc* od) {
            const float* g_out = gradOutMaps ? NULL : gradOutDevice + i0;
            if (win.radius != 5) return ssim_hip::launch_ssimk_grad(win.radius, win.gf, W, H, n, pd, gd, g_out, gradOutMaps ? od : NULL, dataRange, which, c->stream);
            if (gradOutMaps)     return ssim_hip::launch_ssimw_grad_f(W, H, n, pd, gd, od, dataRange, win.gf, which, c->stream);
            return ssim_hip::launch_ssimf_grad(W, H, n, pd, gd, g_out, dataRange, win.gf, which, c->stream);
        });
}

// ---- SSIM of float16 / bfloat16 samples: the same, with the encoding as one more input ---------------------------------------------------------

int ssimh_enqueue_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params16* params, uint32_t sampleType, float dataRange,
                        const Window& win, double* sumsDevice)
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return enqueue_all(c, FamilyH{sample_type(sampleType), dataRange, win}, count, params, sumsDevice);
}

int ssimh_device_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params16* params, uint32_t sampleType, float dataRange,
                       const Window& win, float* ssim)
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return blocking(c, FamilyH{sample_type(sampleType), dataRange, win}, count, params, ssim, false);
}

int ssimh_grad_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params16* params, uint32_t sampleType, float dataRange,
                     const Window& win, const float* gradOutDevice, const rmgr_ssim_hip_GradOutF* gradOutMaps, const rmgr_ssim_hip_GradH* gradA,
                     const rmgr_ssim_hip_GradH* gradB)
{
    if (!c) return EINVAL;
    USE_DEVICE(c);
    const uint32_t W = params[0].width, H = params[0].height;
    const int which = grad_which(gradA, gradB), type = sample_type(sampleType);
    return enqueue_grads<FamilyH>(c, count, params, gradA, gradB, gradOutMaps,
        [&](uint32_t n, uint32_t i0, const PairHDesc* pd, const GradHDesc* gd, const GradOutFDesc* od) {
            const float* g_out = gradOutMaps ? NULL : gradOutDevice + i0;
            if (win.radius != 5) return ssim_hip::launch_ssimhk_grad(win.radius, win.gf, W, H, n, pd, gd, type, g_out, gradOutMaps ? od : NULL, dataRange, which, c->stream);
            if (gradOutMaps)     return ssim_hip::launch_ssimw_grad_h(W, H, n, pd, gd, type, od, dataRange, win.gf, which, c->stream);
            return ssim_hip::launch_ssimh_grad(W, H, n, pd, gd, type, g_out, dataRange, win.gf, which, c->stream);
        });
}

} // namespace

extern "C" {

// ---- SSIM of 9- to 16-bit samples ---------------------------------------------------------------------------------------------------------------

rmgr_int32_t rmgr_ssim_hip_enqueue_ssim16(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                          rmgr_uint32_t bitDepth, double* sumsDevice) RMGR_NOEXCEPT
{
    const int rc = ssim16_validate(count, params, bitDepth, sumsDevice);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return enqueue_all(c, Family16{bitDepth}, count, params, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim16_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                 rmgr_uint32_t bitDepth, float* ssim) RMGR_NOEXCEPT
{
    const int rc = ssim16_validate(count, params, bitDepth, ssim);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return blocking(c, Family16{bitDepth}, count, params, ssim, false);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssim16_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                               rmgr_uint32_t bitDepth, float* ssim) RMGR_NOEXCEPT
{
    const int rc = ssim16_validate(count, params, bitDepth, ssim);
    return rc ? rc : blocking_host(c, Family16{bitDepth}, count, params, ssim);
}

// ---- SSIM of float32 samples and its gradient (one fused launch without scratch) ------------------------------------------------------------------
// Every entry exists twice: under the engine's window and, _win, under the caller's (include/rmgr/ssim-hip.h: rmgr_ssim_hip_Window).
// Both run the same flow; the window is one more input of the family.

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                         float dataRange, double* sumsDevice) RMGR_NOEXCEPT
{
    const int rc = ssimf_validate(count, params, dataRange, sumsDevice);
    return rc ? rc : ssimf_enqueue_entry(c, count, params, dataRange, default_window(), sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                             float dataRange, const rmgr_ssim_hip_Window* window, double* sumsDevice) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimf_validate(count, params, dataRange, sumsDevice);
    if (rc || (rc = window_validate(window, win))) return rc;
    return ssimf_enqueue_entry(c, count, params, dataRange, win, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimf_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const int rc = ssimf_validate(count, params, dataRange, ssim);
    return rc ? rc : ssimf_device_entry(c, count, params, dataRange, default_window(), ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimf_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                    float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimf_validate(count, params, dataRange, ssim);
    if (rc || (rc = window_validate(window, win))) return rc;
    return ssimf_device_entry(c, count, params, dataRange, win, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimf_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                              float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const int rc = ssimf_validate(count, params, dataRange, ssim);
    return rc ? rc : blocking_host(c, FamilyF{dataRange, default_window()}, count, params, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimf_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                  float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimf_validate(count, params, dataRange, ssim);
    if (rc || (rc = window_validate(window, win))) return rc;
    return blocking_host(c, FamilyF{dataRange, win}, count, params, ssim);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                              float dataRange, const float* gradOutDevice,
                                              const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT
{
    int rc = ssimf_validate(count, params, dataRange, gradOutDevice);
    if (rc) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimf_grad_entry(c, count, params, dataRange, default_window(), gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                  float dataRange, const rmgr_ssim_hip_Window* window, const float* gradOutDevice,
                                                  const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimf_validate(count, params, dataRange, gradOutDevice);
    if (rc || (rc = window_validate(window, win))) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimf_grad_entry(c, count, params, dataRange, win, gradOutDevice, NULL, gradA, gradB);
}

// ---- SSIM of float16 / bfloat16 samples and its gradient: the ssimf flow with 2-byte samples ---------------------------------------------------
// As for float32 samples, every entry exists under the engine's window and, _win, under the caller's.

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                         rmgr_uint32_t sampleType, float dataRange, double* sumsDevice) RMGR_NOEXCEPT
{
    const int rc = ssimh_validate(count, params, sampleType, dataRange, sumsDevice);
    return rc ? rc : ssimh_enqueue_entry(c, count, params, sampleType, dataRange, default_window(), sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                             rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                             double* sumsDevice) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimh_validate(count, params, sampleType, dataRange, sumsDevice);
    if (rc || (rc = window_validate(window, win))) return rc;
    return ssimh_enqueue_entry(c, count, params, sampleType, dataRange, win, sumsDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimh_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const int rc = ssimh_validate(count, params, sampleType, dataRange, ssim);
    return rc ? rc : ssimh_device_entry(c, count, params, sampleType, dataRange, default_window(), ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimh_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                    rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                    float* ssim) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimh_validate(count, params, sampleType, dataRange, ssim);
    if (rc || (rc = window_validate(window, win))) return rc;
    return ssimh_device_entry(c, count, params, sampleType, dataRange, win, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimh_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                              rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT
{
    const int rc = ssimh_validate(count, params, sampleType, dataRange, ssim);
    return rc ? rc : blocking_host(c, FamilyH{sample_type(sampleType), dataRange, default_window()}, count, params, ssim);
}

rmgr_int32_t rmgr_ssim_hip_compute_ssimh_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                  float* ssim) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimh_validate(count, params, sampleType, dataRange, ssim);
    if (rc || (rc = window_validate(window, win))) return rc;
    return blocking_host(c, FamilyH{sample_type(sampleType), dataRange, win}, count, params, ssim);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                              rmgr_uint32_t sampleType, float dataRange, const float* gradOutDevice,
                                              const rmgr_ssim_hip_GradH* gradA, const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT
{
    int rc = ssimh_validate(count, params, sampleType, dataRange, gradOutDevice);
    if (rc) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimh_grad_entry(c, count, params, sampleType, dataRange, default_window(), gradOutDevice, NULL, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                  const float* gradOutDevice, const rmgr_ssim_hip_GradH* gradA,
                                                  const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimh_validate(count, params, sampleType, dataRange, gradOutDevice);
    if (rc || (rc = window_validate(window, win))) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimh_grad_entry(c, count, params, sampleType, dataRange, win, gradOutDevice, NULL, gradA, gradB);
}

// ---- gradient of the SSIM map for a per-pixel upstream gradient: the _grad flow with one more descriptor per pair, the gMap plane ----------------

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                  float dataRange, const rmgr_ssim_hip_GradOutF* gradOutMaps,
                                                  const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT
{
    int rc = ssimf_validate(count, params, dataRange, gradOutMaps);
    if (rc) return rc;
    if ((rc = validate_grad_maps(count, gradOutMaps))) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimf_grad_entry(c, count, params, dataRange, default_window(), NULL, gradOutMaps, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_win_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                      float dataRange, const rmgr_ssim_hip_Window* window, const rmgr_ssim_hip_GradOutF* gradOutMaps,
                                                      const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimf_validate(count, params, dataRange, gradOutMaps);
    if (rc || (rc = window_validate(window, win))) return rc;
    if ((rc = validate_grad_maps(count, gradOutMaps))) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimf_grad_entry(c, count, params, dataRange, win, NULL, gradOutMaps, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_GradOutF* gradOutMaps,
                                                  const rmgr_ssim_hip_GradH* gradA, const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT
{
    int rc = ssimh_validate(count, params, sampleType, dataRange, gradOutMaps);
    if (rc) return rc;
    if ((rc = validate_grad_maps(count, gradOutMaps))) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimh_grad_entry(c, count, params, sampleType, dataRange, default_window(), NULL, gradOutMaps, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_win_map_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                      rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                      const rmgr_ssim_hip_GradOutF* gradOutMaps, const rmgr_ssim_hip_GradH* gradA,
                                                      const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT
{
    Window win;
    int rc = ssimh_validate(count, params, sampleType, dataRange, gradOutMaps);
    if (rc || (rc = window_validate(window, win))) return rc;
    if ((rc = validate_grad_maps(count, gradOutMaps))) return rc;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ssimh_grad_entry(c, count, params, sampleType, dataRange, win, NULL, gradOutMaps, gradA, gradB);
}

// ---- multi-scale SSIM of float32 samples and its gradient -------------------------------------------------------------------------------------

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange,
                                           rmgr_uint32_t scales, const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    const MultiF fam = {dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    return rc ? rc : ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimf_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange,
                                                  rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const MultiF fam = {dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimf_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange,
                                                rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const MultiF fam = {dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange,
                                                rmgr_uint32_t scales, const double* weights, const double* scaleMeansDevice, const float* gradOutDevice,
                                                const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT
{
    const MultiF fam = {dataRange, default_window()};
    int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    if (rc) return rc;
    if (scaleMeansDevice == NULL) return EINVAL;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

// ---- multi-scale SSIM of float16 / bfloat16 samples and its gradient: the msssimf flow with 2-byte samples at scale 0 -------------------------

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                           rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                           double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    const MultiH fam = {sampleType, dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    return rc ? rc : ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimh_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                  float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const MultiH fam = {sampleType, dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimh_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const MultiH fam = {sampleType, dataRange, default_window()};
    const int rc = ms_validate(fam, count, params, scales, weights, msssim);
    return rc ? rc : ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                const double* scaleMeansDevice, const float* gradOutDevice, const rmgr_ssim_hip_GradH* gradA,
                                                const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT
{
    const MultiH fam = {sampleType, dataRange, default_window()};
    int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    if (rc) return rc;
    if (scaleMeansDevice == NULL) return EINVAL;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

// ---- the same under the caller's window: both run the same flow; the window is one more input of the family -----------------------------------

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const rmgr_ssim_hip_Window* window,
                                           rmgr_uint32_t scales, const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    MultiF fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimf_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const rmgr_ssim_hip_Window* window,
                                                  rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    MultiF fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimf_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const rmgr_ssim_hip_Window* window,
                                                rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    MultiF fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params, float dataRange, const rmgr_ssim_hip_Window* window,
                                                rmgr_uint32_t scales, const double* weights, const double* scaleMeansDevice, const float* gradOutDevice,
                                                const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT
{
    MultiF fam = {dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    if (scaleMeansDevice == NULL) return EINVAL;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh_win(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                           rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales, const double* weights,
                                           double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    MultiH fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, valuesDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_enqueue_entry(c, fam, count, params, scales, weights, valuesDevice, scaleMeansDevice);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimh_win_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales, const double* weights,
                                                  float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    MultiH fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_device_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssimh_win_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales, const double* weights,
                                                float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    MultiH fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, msssim);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    return ms_host_entry(c, fam, count, params, scales, weights, msssim, scaleMeans);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh_win_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales, const double* weights,
                                                const double* scaleMeansDevice, const float* gradOutDevice, const rmgr_ssim_hip_GradH* gradA,
                                                const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT
{
    MultiH fam = {sampleType, dataRange, Window()};
    int rc = ms_validate(fam, count, params, scales, weights, gradOutDevice);
    if (rc || (rc = window_validate(window, fam.win))) return rc;
    if (scaleMeansDevice == NULL) return EINVAL;
    if ((rc = validate_grads(count, gradA, gradB))) return rc;
    return ms_grad_entry(c, fam, count, params, scales, weights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

} // extern "C"
