// msssim3h_abi.cpp -- the entry points of the C ABI for multi-scale SSIM of float16 / bfloat16 VOLUMES and its gradient
// (rmgr_ssim_hip_*_msssim3h*).  The definition is in include/rmgr/ssim-hip.h, the kernels in msssim3h_kernels.hip (scale 0) and
// msssim3f_kernels.hip (scales >= 1, the reduction, the product, k_s).
//
// The flow is the one of msssim3f_abi.cpp, written for 2-byte samples at scale 0: the same validation in the same order (plus the sample
// type; 2-byte alignment), the same sub-batches (msssim3f_per_sub_batch, msssim3f_scratch_bytes: the scratch is float32 / float64 whatever
// the samples are), staging of host volumes at 2 bytes per sample.  Each sub-batch sends ONE ring table: the scale-0 row of Pair3HDesc,
// the scales x n Pair3FDesc as [scale][pair] whose row 0 nobody reads, and -- backward -- the scale-0 row of Grad3HDesc and the
// scales x n Grad3FDesc likewise.
//
// The scratch is the context's and is rewritten in stream order: msf_pyramid, msf_grads, msf_partials, msf_coef (k_s), msf_out and
// s3_coef, exactly those of msssim3f_abi.cpp.
#include "ssim_context.h"
#include "ssim3_flow.h"
#include "msssim3h_kernels.h"

#include <cmath>

using namespace ssim_host;
using namespace ssim_host::volumes;      // kScratchCap, round64, volume_bytes, take3f, ring_launch

namespace {

using ssim_hip::Pair3FDesc;
using ssim_hip::Grad3FDesc;
using ssim_hip::Pair3HDesc;
using ssim_hip::Grad3HDesc;

// ---- validation, before any device is touched -------------------------------------------------------------------------------------------

int validate_ms3h(uint32_t count, const rmgr_ssim_hip_Params3H* params, uint32_t sampleType, float dataRange, uint32_t scales,
                  const double* weights, const void* out)
{
    if (sampleType != RMGR_SSIM_HIP_SAMPLE_F16 && sampleType != RMGR_SSIM_HIP_SAMPLE_BF16) return EINVAL;
    if (!(dataRange > 0.0f) || !std::isfinite(dataRange)) return EINVAL;
    if (count == 0 || params == NULL || out == NULL) return EINVAL;
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    if (W == 0 || H == 0 || D == 0 || W > ssim_hip::kS3MaxDim || H > ssim_hip::kS3MaxDim || D > ssim_hip::kS3MaxDim) return EINVAL;
    for (uint32_t i = 0; i < count; ++i) {
        const rmgr_ssim_hip_Params3H& p = params[i];
        if (p.width != W || p.height != H || p.depth != D) return EINVAL;
        if (p.imgA.topLeft == NULL || p.imgB.topLeft == NULL) return EINVAL;
        if (((uintptr_t)p.imgA.topLeft & 1u) || ((uintptr_t)p.imgB.topLeft & 1u)) return EINVAL;
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

int validate_grads_ms3h(uint32_t count, const rmgr_ssim_hip_Grad3H* gradA, const rmgr_ssim_hip_Grad3H* gradB)
{
    if (gradA == NULL && gradB == NULL) return EINVAL;
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 2; ++k) {
            const rmgr_ssim_hip_Grad3H* g = k ? gradB : gradA;
            if (g && (g[i].topLeft == NULL || ((uintptr_t)g[i].topLeft & 1u))) return EINVAL;
        }
    return 0;
}

int type_of(uint32_t sampleType) { return sampleType == RMGR_SSIM_HIP_SAMPLE_BF16 ? ssim_hip::kSHTypeBF16 : ssim_hip::kSHTypeF16; }

// ---- descriptors ------------------------------------------------------------------------------------------------------------------------

Pair3HDesc make_desc(const rmgr_ssim_hip_Params3H& p)
{
    Pair3HDesc d;
    d.a = p.imgA.topLeft; d.a_step = p.imgA.step; d.a_stride = p.imgA.stride; d.a_slice = p.imgA.sliceStride;
    d.b = p.imgB.topLeft; d.b_step = p.imgB.step; d.b_stride = p.imgB.stride; d.b_slice = p.imgB.sliceStride;
    d.map = NULL; d.map_step = d.map_stride = d.map_slice = 0;
    return d;
}

// table[scale][pair], scales x n: row 0 all NULL (scale 0 has a table of its own), rows 1 .. scales-1 dense volumes of `pyramid`, scale
// by scale, A then B of each pair -- msssim3f_abi.cpp's layout.
void fill_coarse(Pair3FDesc* table, uint32_t n, uint32_t W, uint32_t H, uint32_t D, uint32_t scales, float* pyramid)
{
    memset(table, 0, n * sizeof(Pair3FDesc));
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
int enqueue_pairs(rmgr_ssim_hip_Context* c, int type, float range, uint32_t n, const Pair3HDesc* d, uint32_t W, uint32_t H, uint32_t D,
                  uint32_t scales, const double* w, double* means, double* values)
{
    int rc;
    if ((rc = c->msf_pyramid.grow((size_t)(2 * ssim_hip::ms3_pyramid_floats(W, H, D, scales) * n)))) return rc;
    if ((rc = c->msf_partials.grow((size_t)ssim_hip::ms3_partials(W, H, D, n, scales)))) return rc;
    const size_t row0_bytes = n * sizeof(Pair3HDesc);
    return ring_launch(c, row0_bytes + (size_t)scales * n * sizeof(Pair3FDesc),
        [&](uint8_t* pin) {
            memcpy(pin, d, row0_bytes);
            fill_coarse(reinterpret_cast<Pair3FDesc*>(pin + row0_bytes), n, W, H, D, scales, c->msf_pyramid);
        },
        [&](const uint8_t* dev) {
            return ssim_hip::launch_msssim3h(reinterpret_cast<const Pair3HDesc*>(dev), reinterpret_cast<const Pair3FDesc*>(dev + row0_bytes), n, W, H,
                                             D, scales, type, range, w, c->cu_count, c->msf_partials, means, values, c->stream);
        });
}

// Every sub-batch of the forward into values[0 .. count-1] and means[count x scales x 2] (device).  stage: host pointers -- each
// sub-batch's volumes are copied (each volume's sample range, 2 bytes per sample) into c->stage_a first.
int forward(rmgr_ssim_hip_Context* c, int type, float range, uint32_t count, const rmgr_ssim_hip_Params3H* params, uint32_t scales,
            const double* w, double* means, double* values, bool stage)
{
    const uint32_t W = params[0].width, H = params[0].height, D = params[0].depth;
    const uint32_t per = ssim_hip::msssim3f_per_sub_batch(W, H, D, scales, 0, kScratchCap);
    const uint64_t scratch = ssim_hip::msssim3f_scratch_bytes(W, H, D, scales, 0);
    int rc;
    try {
        std::vector<Pair3HDesc> d;
        for (uint32_t i0 = 0; i0 < count;) {
            uint64_t staged, off = 0;
            const uint32_t n = take3f(params, i0, count, per, scratch, stage, staged);
            if (stage && (rc = c->stage_a.grow((size_t)staged))) return rc;
            d.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                const rmgr_ssim_hip_Params3H& p = params[i0 + i];
                d[i] = make_desc(p);
                if (!stage) continue;
                for (int k = 0; k < 2; ++k) {
                    const rmgr_ssim_hip_Img3H& im = k ? p.imgB : p.imgA;
                    int64_t lo;
                    const size_t bytes = volume_bytes(im, W, H, D, lo);
                    HIP_TRY(hipMemcpyAsync(c->stage_a + off, im.topLeft + lo, bytes, hipMemcpyHostToDevice, c->stream));
                    (k ? d[i].b : d[i].a) = reinterpret_cast<const uint16_t*>(c->stage_a + off) - lo;
                    off += round64(bytes);
                }
            }
            if ((rc = enqueue_pairs(c, type, range, n, &d[0], W, H, D, scales, w, means + (size_t)i0 * scales * 2, values + i0))) return rc;
            i0 += n;
        }
    } catch (...) {
        return ENOMEM;
    }
    return 0;
}

// The blocking entry points: every sub-batch into c->msf_out (count values, then count x scales x 2 means), one copy back, one wait.
int blocking(rmgr_ssim_hip_Context* c, int type, float range, uint32_t count, const rmgr_ssim_hip_Params3H* params, uint32_t scales,
             const double* w, float* msssim, double* scaleMeans, bool stage)
{
    const size_t total = (1 + 2 * (size_t)scales) * count;
    int rc;
    if ((rc = c->msf_out.grow(total))) return rc;
    if ((rc = c->msf_out_pin.grow(total))) return rc;
    if ((rc = forward(c, type, range, count, params, scales, w, c->msf_out + count, c->msf_out, stage))) return rc;
    HIP_TRY(hipMemcpyAsync(c->msf_out_pin, c->msf_out, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < count; ++i) msssim[i] = (float)c->msf_out_pin[i];
    if (scaleMeans) memcpy(scaleMeans, c->msf_out_pin + count, (size_t)count * scales * 2 * sizeof(double));
    return 0;
}

// ---- the gradient -----------------------------------------------------------------------------------------------------------------------
// Per sub-batch: the pyramid step out of the 16-bit volumes, the float32 backward of scales >= 1 (msssim3f_abi.cpp: grad_entry), then scale
// 0's coefficient walk into c->s3_coef and its adjoint walk into the caller's 16-bit gradient volumes.
int grad_entry(rmgr_ssim_hip_Context* c, uint32_t count, const rmgr_ssim_hip_Params3H* params, int type, float range, uint32_t scales,
               const double* w, const double* scaleMeansDevice, const float* gradOutDevice, const rmgr_ssim_hip_Grad3H* gradA,
               const rmgr_ssim_hip_Grad3H* gradB)
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
        const size_t pair0_bytes = n * sizeof(Pair3HDesc), pair_bytes = (size_t)scales * n * sizeof(Pair3FDesc);
        const size_t grad0_bytes = n * sizeof(Grad3HDesc), grad_bytes = (size_t)scales * n * sizeof(Grad3FDesc);
        rc = ring_launch(c, pair0_bytes + pair_bytes + grad0_bytes + grad_bytes,
            [&](uint8_t* pin) {
                Pair3HDesc* pd0 = reinterpret_cast<Pair3HDesc*>(pin);
                Pair3FDesc* pd = reinterpret_cast<Pair3FDesc*>(pin + pair0_bytes);
                Grad3HDesc* gd0 = reinterpret_cast<Grad3HDesc*>(pin + pair0_bytes + pair_bytes);
                Grad3FDesc* gd = reinterpret_cast<Grad3FDesc*>(pin + pair0_bytes + pair_bytes + grad0_bytes);
                for (uint32_t i = 0; i < n; ++i) {
                    pd0[i] = make_desc(params[i0 + i]);
                    Grad3HDesc g = {NULL, 0, 0, 0, NULL, 0, 0, 0};
                    if (gradA) { const rmgr_ssim_hip_Grad3H& s = gradA[i0 + i]; g.ga = s.topLeft; g.ga_step = s.step; g.ga_stride = s.stride; g.ga_slice = s.sliceStride; }
                    if (gradB) { const rmgr_ssim_hip_Grad3H& s = gradB[i0 + i]; g.gb = s.topLeft; g.gb_step = s.step; g.gb_stride = s.stride; g.gb_slice = s.sliceStride; }
                    gd0[i] = g;
                }
                fill_coarse(pd, n, W, H, D, scales, c->msf_pyramid);
                // gradient volumes of scales >= 1: dense float32 scratch, scale by scale, dA then dB of each pair; row 0 all NULL
                memset(gd, 0, n * sizeof(Grad3FDesc));
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
                return ssim_hip::launch_msssim3h_grad(reinterpret_cast<const Pair3HDesc*>(dev), reinterpret_cast<const Pair3FDesc*>(dev + pair0_bytes),
                                                      reinterpret_cast<const Grad3HDesc*>(dev + pair0_bytes + pair_bytes),
                                                      reinterpret_cast<const Grad3FDesc*>(dev + pair0_bytes + pair_bytes + grad0_bytes), n, W, H, D,
                                                      scales, type, range, w, c->cu_count, scaleMeansDevice + (size_t)i0 * scales * 2,
                                                      gradOutDevice + i0, c->msf_coef, c->s3_coef, which, c->stream);
            });
        if (rc) return rc;
        i0 += n;
    }
    return 0;
}

} // namespace

extern "C" {

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                            rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                            double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT
{
    const int rc = validate_ms3h(count, params, sampleType, dataRange, scales, weights, valuesDevice);
    if (rc) return rc;
    if (scaleMeansDevice == NULL || !c) return EINVAL;
    USE_DEVICE(c);
    return forward(c, type_of(sampleType), dataRange, count, params, scales, weights ? weights : kWangWeights, scaleMeansDevice, valuesDevice, false);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_device(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                   float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    const int rc = validate_ms3h(count, params, sampleType, dataRange, scales, weights, msssim);
    if (rc) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return blocking(c, type_of(sampleType), dataRange, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, false);
}

rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_host(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                 float* msssim, double* scaleMeans) RMGR_NOEXCEPT
{
    int rc = validate_ms3h(count, params, sampleType, dataRange, scales, weights, msssim);
    if (rc) return rc;
    Lease lease;                         // ctx == NULL: one of the default contexts, for this call only
    if ((rc = lease.take(c))) return rc;
    USE_DEVICE(lease.c);
    return blocking(lease.c, type_of(sampleType), dataRange, count, params, scales, weights ? weights : kWangWeights, msssim, scaleMeans, true);
}

rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h_grad(rmgr_ssim_hip_Context* c, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                 const double* scaleMeansDevice, const float* gradOutDevice, const rmgr_ssim_hip_Grad3H* gradA,
                                                 const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT
{
    int rc = validate_ms3h(count, params, sampleType, dataRange, scales, weights, gradOutDevice);
    if (rc) return rc;
    if (scaleMeansDevice == NULL) return EINVAL;
    if ((rc = validate_grads_ms3h(count, gradA, gradB))) return rc;
    if (!c) return EINVAL;
    USE_DEVICE(c);
    return grad_entry(c, count, params, type_of(sampleType), dataRange, scales, weights ? weights : kWangWeights, scaleMeansDevice, gradOutDevice,
                      gradA, gradB);
}

} // extern "C"
