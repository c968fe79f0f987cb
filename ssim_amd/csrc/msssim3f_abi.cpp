// msssim3f_abi.cpp -- the entry points of the C ABI for multi-scale SSIM of float32 VOLUMES and its gradient
// (rmgr_ssim_hip_*_msssim3f*).  The definition is in include/rmgr/ssim-hip.h, the kernels in msssim3f_kernels.hip.
//
// The flow is msssimf's (ssim_samples_abi.cpp) written for three strides on top of ssim3_flow.h: validation before any device is touched;
// scale 0 read where the caller has it; the volumes of scales >= 1 (and, in the backward, their gradient volumes) dense float32 volumes of
// the context's scratch, one set per pair; one table of scales x n Pair3FDesc as [scale][pair] (and, backward, one of Grad3FDesc) per
// sub-batch through the context's ring; sub-batches under kScratchCap of device scratch (msssim3f_scratch_bytes per pair) with at least
// one pair each.  Every sum runs over fixed cells in a fixed order and every gradient voxel belongs to one fixed tile: neither the
// sub-batches nor the launch a pair lands in change a bit.
//
// The scratch is the context's and is rewritten in stream order: msf_pyramid, msf_grads, msf_partials, msf_coef (k_s) and msf_out, which
// the 2-D multi-scale family uses as well, and s3_coef, the coefficient volumes of the volume family.
#include "ssim_context.h"
#include "ssim3_flow.h"
#include "msssim3f_kernels.h"

#include <cmath>

using namespace ssim_host;
using namespace ssim_host::volumes;      // kScratchCap, round64, volume_bytes, take3f, ring_launch

namespace {

using ssim_hip::Pair3FDesc;
using ssim_hip::Grad3FDesc;

// ---- validation, before any device is touched -------------------------------------------------------------------------------------------

int validate_ms3f(uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange, uint32_t scales, const double* weights, const void* out)
{
    if (!(dataRange > 0.0f) || !std::isfinite(dataRange)) return EINVAL;
    if (count == 0 || params == NULL || out == NULL) return EINVAL;
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    if (W == 0 || H == 0 || D == 0 || W > ssim_hip::kS3MaxDim || H > ssim_hip::kS3MaxDim || D > ssim_hip::kS3MaxDim) return EINVAL;
    for (uint32_t i = 0; i < count; ++i) {
        const rmgr_ssim_hip_Params3F& p = params[i];
        if (p.width != W || p.height != H || p.depth != D) return EINVAL;
        if (p.imgA.topLeft == NULL || p.imgB.topLeft == NULL) return EINVAL;
        if (((uintptr_t)p.imgA.topLeft & 3u) || ((uintptr_t)p.imgB.topLeft & 3u)) return EINVAL;
        if (p.ssimMap != NULL) return EINVAL;
    }
    if (scales < 1 || scales > RMGR_SSIM_HIP_MSSSIM_MAX_SCALES) return EINVAL;
    if (weights == NULL) {
        if (scales != 5) return EINVAL;
    } else {
        for (uint32_t s = 0; s < scales; ++s)
            if (!std::isfinite(weights[s]) || weights[s] < 0.0) return EINVAL;
    }
    if (ssim_hip::msssim3f_max_count(W, H, D) == 0) return EINVAL;
    return 0;
}

int validate_grads_ms3f(uint32_t count, const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB)
{
    if (gradA == NULL && gradB == NULL) return EINVAL;
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 2; ++k) {
            const rmgr_ssim_hip_Grad3F* g = k ? gradB : gradA;
            if (g && (g[i].topLeft == NULL || ((uintptr_t)g[i].topLeft & 3u))) return EINVAL;
        }
    return 0;
}

// ---- descriptors ------------------------------------------------------------------------------------------------------------------------

Pair3FDesc make_desc(const rmgr_ssim_hip_Params3F& p)
{
    Pair3FDesc d;
    d.a = p.imgA.topLeft; d.a_step = p.imgA.step; d.a_stride = p.imgA.stride; d.a_slice = p.imgA.sliceStride;
    d.b = p.imgB.topLeft; d.b_step = p.imgB.step; d.b_stride = p.imgB.stride; d.b_slice = p.imgB.sliceStride;
    d.map = NULL; d.map_step = d.map_stride = d.map_slice = 0;
    return d;
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

// ---- the forward flow -------------------------------------------------------------------------------------------------------------------

// Enqueues the forward of n pairs (scale-0 descriptors in host memory, volumes on the device): n x scales x 2 means and n values into
// device memory.
int enqueue_pairs(rmgr_ssim_hip_Context* c, float range, uint32_t n, const Pair3FDesc* d, uint32_t W, uint32_t H, uint32_t D, uint32_t scales,
                  const double* w, double* means, double* values)
{
    int rc;
    if ((rc = c->msf_pyramid.grow((size_t)(2 * ssim_hip::ms3_pyramid_floats(W, H, D, scales) * n)))) return rc;
    if ((rc = c->msf_partials.grow((size_t)ssim_hip::ms3_partials(W, H, D, n, scales)))) return rc;
    return ring_launch(c, (size_t)scales * n * sizeof(Pair3FDesc),
        [&](uint8_t* pin) {
            Pair3FDesc* table = reinterpret_cast<Pair3FDesc*>(pin);
            memcpy(table, d, n * sizeof(Pair3FDesc));
            fill_coarse(table, n, W, H, D, scales, c->msf_pyramid);
        },
        [&](const uint8_t* dev) {
            return ssim_hip::launch_msssim3f(reinterpret_cast<const Pair3FDesc*>(dev), n, W, H, D, scales, range, w, c->cu_count, c->msf_partials,
                                             means, values, c->stream);
        });
}

// Every sub-batch of the forward into values[0 .. count-1] and means[count x scales x 2] (device).  stage: host pointers -- each
// sub-batch's volumes are copied (each volume's sample range) into c->stage_a first.
int forward(rmgr_ssim_hip_Context* c, float range, uint32_t count, const rmgr_ssim_hip_Params3F* params, uint32_t scales, const double* w,
            double* means, double* values, bool stage)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const uint32_t per = ssim_hip::msssim3f_per_sub_batch(W, H, D, scales, 0, kScratchCap);
    const uint64_t scratch = ssim_hip::msssim3f_scratch_bytes(W, H, D, scales, 0);
    int rc;
    try {
        std::vector<Pair3FDesc> d;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged, off = 0;
            const uint32_t n = take3f(params, i0, count, per, scratch, stage, staged);
            if (stage && (rc = c->stage_a.grow((size_t)staged))) return rc;
            d.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                const rmgr_ssim_hip_Params3F& p = params[i0 + i];
                d[i] = make_desc(p);
                if (!stage) continue;
                for (int k = 0; k < 2; ++k) {
                    const rmgr_ssim_hip_Img3F& im = k ? p.imgB : p.imgA;
                    int64_t lo;
                    const size_t bytes = volume_bytes(im, W, H, D, lo);
                    HIP_TRY(hipMemcpyAsync(c->stage_a + off, im.topLeft + lo, bytes, hipMemcpyHostToDevice, c->stream));
                    (k ? d[i].b : d[i].a) = reinterpret_cast<const float*>(c->stage_a + off) - lo;
                    off += round64(bytes);
                }
            }
            if ((rc = enqueue_pairs(c, range, n, &d[0], W, H, D, scales, w, means + (size_t)i0 * scales * 2, values + i0))) return rc;
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    return 0;
}

// The blocking entry points: every sub-batch into c->msf_out (count values, then count x scales x 2 means), one copy back, one wait.
int blocking(rmgr_ssim_hip_Context* c, float range, uint32_t count, const rmgr_ssim_hip_Params3F* params, uint32_t scales, const double* w,
             float* msssim, double* scaleMeans, bool stage)
{
    const size_t total = (1 + 2 * (size_t)scales) * count;
    int rc;
    if ((rc = c->msf_out.grow(total))) return rc;
    if ((rc = c->msf_out_pin.grow(total))) return rc;
    if ((rc = forward(c, range, count, params, scales, w, c->msf_out + count, c->msf_out, stage))) return rc;
    HIP_TRY(hipMemcpyAsync(c->msf_out_pin, c->msf_out, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < count; ++i) msssim[i] = (float)c->msf_out_pin[i];
    if (scaleMeans) memcpy(scaleMeans, c->msf_out_pin + count, (size_t)count * scales * 2 * sizeof(double));
    return 0;
}

// ---- the gradient -----------------------------------------------------------------------------------------------------------------------
// Per sub-batch: the coefficients k_s, the pyramid again, then from the coarsest scale down the walk that writes the coefficient volumes
// into c->s3_coef (sized for scale 0, reused by every scale) and the adjoint walk, the caller's gradient volumes at scale 0 and dense
// float32 scratch volumes below.
int grad_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params3F* params, float range, uint32_t scales, const double* w,
               const double* scaleMeansDevice, const float* gradOutDevice, const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const int which = (gradA ? 1 : 0) | (gradB ? 2 : 0), planes = (gradA ? 1 : 0) + (gradB ? 1 : 0);
    const uint64_t pyr = ssim_hip::ms3_pyramid_floats(W, H, D, scales);
    const uint64_t coef_per_volume = (uint64_t)ssim_hip::ssim3f_coef_planes(which) * W * H * D;
    const uint32_t per = ssim_hip::msssim3f_per_sub_batch(W, H, D, scales, planes, kScratchCap);
    const uint64_t scratch = ssim_hip::msssim3f_scratch_bytes(W, H, D, scales, planes);
    for (uint32_t i0 = 0; i0 < count;) {
        uint64_t staged;
        const uint32_t n = take3f(params, i0, count, per, scratch, false, staged);
        int rc;
        if ((rc = c->msf_pyramid.grow((size_t)(2 * pyr * n)))) return rc;
        if ((rc = c->msf_grads.grow((size_t)((uint64_t)planes * pyr * n)))) return rc;
        if ((rc = c->msf_coef.grow((size_t)n * scales))) return rc;
        if ((rc = c->s3_coef.grow((size_t)(coef_per_volume * n)))) return rc;
        const size_t pair_bytes = (size_t)scales * n * sizeof(Pair3FDesc), grad_bytes = (size_t)scales * n * sizeof(Grad3FDesc);
        rc = ring_launch(c, pair_bytes + grad_bytes,
            [&](uint8_t* pin) {
                Pair3FDesc* pd = reinterpret_cast<Pair3FDesc*>(pin);
                Grad3FDesc* gd = reinterpret_cast<Grad3FDesc*>(pin + pair_bytes);
                for (uint32_t i = 0; i < n; ++i) {
                    pd[i] = make_desc(params[i0 + i]);
                    Grad3FDesc g = {NULL, 0, 0, 0, NULL, 0, 0, 0};
                    if (gradA) { const rmgr_ssim_hip_Grad3F& s = gradA[i0 + i]; g.ga = s.topLeft; g.ga_step = s.step; g.ga_stride = s.stride; g.ga_slice = s.sliceStride; }
                    if (gradB) { const rmgr_ssim_hip_Grad3F& s = gradB[i0 + i]; g.gb = s.topLeft; g.gb_step = s.step; g.gb_stride = s.stride; g.gb_slice = s.sliceStride; }
                    gd[i] = g;
                }
                fill_coarse(pd, n, W, H, D, scales, c->msf_pyramid);
                // gradient volumes of scales >= 1: dense scratch, scale by scale, dA then dB of each pair
                float* at = c->msf_grads;
                for (uint32_t sc = 1; sc < scales; ++sc) {
                    const uint64_t voxels = ssim_hip::ms3_voxels(W, H, D, sc);
                    const int64_t stride = ssim_hip::ms3_dim(W, sc), slice = stride * (int64_t)ssim_hip::ms3_dim(H, sc);
                    for (uint32_t i = 0; i < n; ++i) {
                        Grad3FDesc g = {NULL, 0, 0, 0, NULL, 0, 0, 0};
                        if (gradA) { g.ga = at; g.ga_step = 1; g.ga_stride = stride; g.ga_slice = slice; at += voxels; }
                        if (gradB) { g.gb = at; g.gb_step = 1; g.gb_stride = stride; g.gb_slice = slice; at += voxels; }
                        gd[(size_t)sc * n + i] = g;
                    }
                }
            },
            [&](const uint8_t* dev) {
                return ssim_hip::launch_msssim3f_grad(reinterpret_cast<const Pair3FDesc*>(dev), reinterpret_cast<const Grad3FDesc*>(dev + pair_bytes), n,
                                                      W, H, D, scales, range, w, c->cu_count, scaleMeansDevice + (size_t)i0 * scales * 2,
                                                      gradOutDevice + i0, c->msf_coef, c->s3_coef, which, c->stream);
            });
        if (rc) return rc;
        i0 += n;
    }
    return 0;
}

} // namespace

extern "C" {

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                            rmgr_uint32_t scales, const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    const int rc = validate_ms3f(count, params, dataRange, scales, weights, valuesDevice);
    if (rc) return rc;
    if (scaleMeansDevice == NULL || !c) return EINVAL;
    USE_DEVICE(c);
    return forward(c, dataRange, count, params, scales, weights ? weights : kWangWeights, scaleMeansDevice, valuesDevice, false);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                                   rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const int rc = validate_ms3f(count, params, dataRange, scales, weights, msssim);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return blocking(c, dataRange, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, false);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                                 rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    int rc = validate_ms3f(count, params, dataRange, scales, weights, msssim);
    if (rc) return rc;
    Lease lease;                         // ctx == NULL: one of the default contexts, for this call only
    if ((rc = lease.take(c))) return rc;
    USE_DEVICE(lease.c);
    return blocking(lease.c, dataRange, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, true);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params, float dataRange,
                                                 rmgr_uint32_t scales, const double* weights, const double* scaleMeansDevice,
                                                 const float* gradOutDevice, const rmgr_ssim_hip_Grad3F* gradA,
                                                 const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT
{
    int rc = validate_ms3f(count, params, dataRange, scales, weights, gradOutDevice);
    if (rc) return rc;
    if (scaleMeansDevice == NULL) return EINVAL;
    if ((rc = validate_grads_ms3f(count, gradA, gradB))) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return grad_entry(c, count, params, dataRange, scales, weights ? weights : kWangWeights, scaleMeansDevice, gradOutDevice, gradA, gradB);
}

} // extern "C"
