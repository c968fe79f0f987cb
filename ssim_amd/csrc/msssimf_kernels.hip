// msssimf_kernels.hip -- gfx950 kernels of multi-scale SSIM on float32 samples and of its gradient, behind
// rmgr_ssim_hip_enqueue_msssimf, rmgr_ssim_hip_compute_msssimf_device / _host and rmgr_ssim_hip_enqueue_msssimf_grad.  The definition
// they implement is in include/rmgr/ssim-hip.h; tests/msssimf_model.py restates it in float64 and restates the arithmetic in fp32.
//
// Kept apart from ssimf_kernels.hip and msssim_kernels.hip on purpose: tests count and budget the kernels of those files, and the
// uint8 multi-scale path's bits are pinned.  The strip walk and the gradient tile are those of ssimf_kernels.hip in their multi-scale
// forms; see ssim2_walk.h.
//
//  * msssimf_down_kernel: one step of the pyramid, a launch of its own: scale s + 1 = ((P(2x,2y) + P(2x+1,2y)) + (P(2x,2y+1) +
//    P(2x+1,2y+1))) * 0.25f of scale s, coordinates clamped, every operation rounded to fp32 in that order; A and B of a pair in one
//    work-item.  Scale 0 is read at the caller's steps and strides, every coarser scale is a dense plane of the context's scratch.
//  * msssimf_strip_kernel: strip_body in the form kFormMulti: no map, TWO fp64 sums per cell, cs = A2 / B2 and
//    ssim = A1 A2 / (B1 B2).  One launch per scale over that scale's descriptors.
//  * msssimf_reduce_kernel: every (pair, scale, kind) sum of cell partials in a fixed order, divided by double(W_s) * double(H_s).
//  * msssimf_finalise_kernel: the ReLU'd weighted product of a pair's means, in double.
//  * msssimf_coef_kernel: k_s = gOut w_s MS / m_s / (double(W_s) * double(H_s)) per pair and scale, all 0 when MS = 0.
//  * msssimf_grad_kernel: grad_body with k_s read from device memory (kKCoef), in a cs form (kMsUp), whose epilogue adds the coarser
//    scale's gradient through the adjoint of the clamped box filter, and an ssim form (kMsLast).
//
// Centring, per-pixel values and cells: see the top of ssim2_walk.h; the rules hold at every scale on that scale's planes.
#include "ssim2_walk.h"

namespace ssim_hip {
namespace {

// WIDE: 64-bit lane offsets for the samples (scale-0 pairs that fail fitsf_narrow()).
template <bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void msssimf_strip_kernel(const Strip2Args<PairFDesc> args) { strip_body<SampleF32, 5, kFormMulti, 0, WIDE>(args); }

// ---- pyramid, reduction, product, coefficients ---------------------------------------------------------------------------------

// One step of the pyramid: work-item = one pixel of scale s + 1 of one pair, A and B.  dst planes are dense (step 1, stride dst_w).
__global__ __launch_bounds__(256)
void msssimf_down_kernel(const PairFDesc* __restrict__ src, const PairFDesc* __restrict__ dst, uint32_t src_w, uint32_t src_h,
                         uint32_t dst_w, uint32_t dst_h, uint32_t blocks_per_image)
{
    const uint32_t img = blockIdx.x / blocks_per_image, blk = blockIdx.x - img * blocks_per_image;
    const uint64_t idx = (uint64_t)blk * 256 + threadIdx.x;
    if (idx >= (uint64_t)dst_w * dst_h) return;
    const uint32_t y = (uint32_t)(idx / dst_w), x = (uint32_t)(idx - (uint64_t)y * dst_w);
    const PairFDesc s = src[img];
    const PairFDesc d = dst[img];
    const int64_t x0 = 2 * (int64_t)x, x1 = x0 + 1 < (int64_t)src_w ? x0 + 1 : (int64_t)src_w - 1;
    const int64_t y0 = 2 * (int64_t)y, y1 = y0 + 1 < (int64_t)src_h ? y0 + 1 : (int64_t)src_h - 1;
    {
        const gptr_cf32 p = (gptr_cf32)s.a;
        const float top = p[x0 * s.a_step + y0 * s.a_stride] + p[x1 * s.a_step + y0 * s.a_stride];
        const float bot = p[x0 * s.a_step + y1 * s.a_stride] + p[x1 * s.a_step + y1 * s.a_stride];
        ((gptr_f32)const_cast<float*>(d.a))[idx] = (top + bot) * 0.25f;
    }
    {
        const gptr_cf32 p = (gptr_cf32)s.b;
        const float top = p[x0 * s.b_step + y0 * s.b_stride] + p[x1 * s.b_step + y0 * s.b_stride];
        const float bot = p[x0 * s.b_step + y1 * s.b_stride] + p[x1 * s.b_step + y1 * s.b_stride];
        ((gptr_f32)const_cast<float*>(d.b))[idx] = (top + bot) * 0.25f;
    }
}

struct KRArgs {
    const double* partials;
    double*       means;                      // [pair][scale]{mcs, mssim}
    uint32_t      count, scales;
    uint64_t      offset[kMSFMaxScales];      // of a scale's partials, in doubles
    uint64_t      cells[kMSFMaxScales];       // per image
    double        pixels[kMSFMaxScales];      // double(W_s) * double(H_s)
};

// Workgroup (pair, scale, kind): thread t of 256 adds cells t, t + 256, ... in that order, each wave runs a fixed xor butterfly, and
// the four wave totals are added in wave order.
constexpr int kReduceThreads = 256;

__global__ __launch_bounds__(kReduceThreads) void msssimf_reduce_kernel(const KRArgs args)
{
    __shared__ double sh[kReduceThreads / 64];
    const uint32_t kind = blockIdx.x & 1u, rest = blockIdx.x >> 1;
    const uint32_t s = rest % args.scales, img = rest / args.scales;
    const uint64_t cells = args.cells[s];
    const double* p = args.partials + args.offset[s] + (uint64_t)img * cells * 2 + kind;
    double acc = 0.0;
    for (uint64_t i = threadIdx.x; i < cells; i += kReduceThreads)
        acc += p[2 * i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63u) == 0)
        sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
#pragma unroll
        for (int w = 1; w < kReduceThreads / 64; ++w)
            t += sh[w];
        args.means[((size_t)img * args.scales + s) * 2 + kind] = t / args.pixels[s];
    }
}

struct KWArgs {
    uint32_t count, scales;
    double   weights[kMSFMaxScales];
    double   pixels[kMSFMaxScales];
};

// The mean scale s contributes: mcs_s, or mssim_s for the last scale.
__device__ __forceinline__ double scale_mean(const double* means, uint32_t s, uint32_t scales) { return means[2 * s + (s + 1 == scales ? 1 : 0)]; }

// prod max(m_s, 0)^w_s with x^0 = 1; a NaN mean stays a NaN.
__device__ __forceinline__ double ms_product(const double* means, const KWArgs& a)
{
    double r = 1.0;
    for (uint32_t s = 0; s < a.scales; ++s) {
        if (a.weights[s] == 0.0) continue;
        const double m = scale_mean(means, s, a.scales);
        r *= pow(m <= 0.0 ? 0.0 : m, a.weights[s]);
    }
    return r;
}

__global__ __launch_bounds__(64) void msssimf_finalise_kernel(const KWArgs args, const double* __restrict__ means, double* __restrict__ values)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= args.count) return;
    values[i] = ms_product(means + (size_t)i * args.scales * 2, args);
}

// k_s of every pair and scale, rounded to float once; all 0 when MS = 0 (the ReLU's subgradient) and where w_s = 0.
__global__ __launch_bounds__(64) void msssimf_coef_kernel(const KWArgs args, const double* __restrict__ means, const float* __restrict__ g_out,
                                                          float* __restrict__ coef)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= args.count) return;
    const double* m = means + (size_t)i * args.scales * 2;
    const double ms = ms_product(m, args);
    const double g = (double)g_out[i];
    for (uint32_t s = 0; s < args.scales; ++s) {
        double k = 0.0;
        if (ms != 0.0 && args.weights[s] != 0.0)
            k = g * args.weights[s] * ms / scale_mean(m, s, args.scales) / args.pixels[s];
        coef[(size_t)i * args.scales + s] = (float)k;
    }
}

// LAST: the coarsest scale (the ssim form, no coarser gradient to add); otherwise the cs form.
template <int WHICH, bool LAST>
__global__ __launch_bounds__(256)
void msssimf_grad_kernel(const Grad2Args<PairFDesc, GradFDesc> args) { grad_body<SampleF32, 5, WHICH, kKCoef, LAST ? kMsLast : kMsUp>(args); }

bool valid_call(uint32_t count, uint32_t width, uint32_t height, uint32_t scales, float data_range, const double* weights)
{
    if (!(data_range > 0.0f) || !std::isfinite(data_range) || scales < 1 || scales > kMSFMaxScales || weights == nullptr) return false;
    for (uint32_t s = 0; s < scales; ++s)
        if (!std::isfinite(weights[s]) || weights[s] < 0.0) return false;
    return count <= msssimf_max_count(width, height);
}

KWArgs weight_args(uint32_t count, uint32_t width, uint32_t height, uint32_t scales, const double* weights)
{
    KWArgs a;
    a.count = count; a.scales = scales;
    for (uint32_t s = 0; s < kMSFMaxScales; ++s) {
        a.weights[s] = s < scales ? weights[s] : 0.0;
        a.pixels[s] = (double)msf_dim(width, s) * (double)msf_dim(height, s);
    }
    return a;
}

// The pyramid of `count` pairs from scale `first` on: one launch per step, finest first.
hipError_t launch_pyramid(uint32_t first, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, hipStream_t stream)
{
    for (uint32_t s = first; s + 1 < scales; ++s) {
        const uint32_t sw = msf_dim(width, s), sh = msf_dim(height, s), dw = msf_dim(width, s + 1), dh = msf_dim(height, s + 1);
        const uint32_t per = (uint32_t)(((uint64_t)dw * dh + 255) / 256);
        hipLaunchKernelGGL(msssimf_down_kernel, dim3(per * count), dim3(256), 0, stream, descs_dev + (size_t)s * count,
                           descs_dev + (size_t)(s + 1) * count, sw, sh, dw, dh, per);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

// Strip height of one scale's launch: planf()'s.  Results do not depend on it.
uint32_t strip_rows_of(uint32_t width, uint32_t height, uint32_t count, int cu_count) { return planf(width, height, count, cu_count).strip_rows; }

uint64_t msf_cells(uint32_t W, uint32_t H, uint32_t s)
{
    const uint32_t w = msf_dim(W, s), h = msf_dim(H, s), cr = cell_rows_of(h);
    return (uint64_t)((w + 63) / 64) * ((h + cr - 1) / cr);
}

uint32_t msssimf_max_count(uint32_t width, uint32_t height)
{
    // scale 0 has the largest grids: strips of the smallest height, gradient tiles; a pyramid step has a quarter of the tiles' lanes
    return ssimf_max_count(width, height);
}

hipError_t launch_msssimf(const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, bool wide,
                          float data_range, const double* weights, int cu_count, int xcd_count, double* partials, double* means,
                          double* values, hipStream_t stream)
{
    float taps[MAXR + 1];
    default_taps(taps);
    return launch_msssimf_from(0, MAXR, taps, descs_dev, count, width, height, scales, wide, data_range, weights, cu_count, xcd_count, partials, means,
                               values, stream);
}

// ---- the steps that do not depend on the window, for this file's launchers and for msssimk_kernels.hip's --------------------------

hipError_t launch_msssimf_pyramid(uint32_t first, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales,
                                  hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (first > 1 || scales < 1 || scales > kMSFMaxScales || count > msssimf_max_count(width, height)) return hipErrorInvalidValue;
    return launch_pyramid(first, descs_dev, count, width, height, scales, stream);
}

hipError_t launch_msssimf_means(uint32_t count, uint32_t width, uint32_t height, uint32_t scales, const double* weights, const double* partials,
                                double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(count, width, height, scales, 1.0f, weights)) return hipErrorInvalidValue;
    KRArgs kr;
    kr.partials = partials; kr.means = means; kr.count = count; kr.scales = scales;
    uint64_t offset = 0;
    for (uint32_t s = 0; s < kMSFMaxScales; ++s) { kr.offset[s] = 0; kr.cells[s] = 0; kr.pixels[s] = 1.0; }
    for (uint32_t s = 0; s < scales; ++s) {
        kr.offset[s] = offset; kr.cells[s] = msf_cells(width, height, s); kr.pixels[s] = (double)msf_dim(width, s) * (double)msf_dim(height, s);
        offset += kr.cells[s] * 2 * count;
    }
    hipLaunchKernelGGL(msssimf_reduce_kernel, dim3(count * scales * 2), dim3(kReduceThreads), 0, stream, kr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(msssimf_finalise_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, weight_args(count, width, height, scales, weights), means, values);
    return hipGetLastError();
}

hipError_t launch_msssimf_coef(uint32_t count, uint32_t width, uint32_t height, uint32_t scales, const double* weights, const double* means,
                               const float* g_out, float* coef, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(count, width, height, scales, 1.0f, weights)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(msssimf_coef_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, weight_args(count, width, height, scales, weights), means, g_out, coef);
    return hipGetLastError();
}

// ---- the launchers of the 11-tap window ---------------------------------------------------------------------------------------------

hipError_t launch_msssimf_from(uint32_t first, uint32_t radius, const float (&taps)[kSKMaxRadius + 1], const PairFDesc* descs_dev, uint32_t count,
                               uint32_t width, uint32_t height, uint32_t scales, bool wide, float data_range, const double* weights, int cu_count,
                               int xcd_count, double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(count, width, height, scales, data_range, weights) || first > 1 || radius != MAXR) return hipErrorInvalidValue;
    hipError_t e = launch_pyramid(first, descs_dev, count, width, height, scales, stream);
    if (e != hipSuccess) return e;
    uint64_t offset = 0;
    for (uint32_t s = 0; s < scales; ++s) {
        const GeometryF geo = planf(msf_dim(width, s), msf_dim(height, s), count, cu_count);
        const Strip2Args<PairFDesc> ka = fill_strip(geo, descs_dev + (size_t)s * count, data_range, taps, xcd_count, partials + offset);
        offset += geo.cells_per_image() * 2 * count;
        if (s < first) continue;                  // the caller's own strip kernel fills this scale's partials
        pick_bool(wide && s == 0, [&](auto w) { hipLaunchKernelGGL((msssimf_strip_kernel<decltype(w)::value>), strip_grid(geo), dim3(64), 0, stream, ka); });
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_msssimf_means(count, width, height, scales, weights, partials, means, values, stream);
}

hipError_t launch_msssimf_grad(const PairFDesc* descs_dev, const GradFDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height,
                               uint32_t scales, float data_range, const double* weights, const double* means, const float* g_out,
                               float* coef, int which, hipStream_t stream)
{
    float taps[MAXR + 1];
    default_taps(taps);
    return launch_msssimf_grad_from(0, MAXR, taps, descs_dev, grads_dev, count, width, height, scales, data_range, weights, means, g_out, coef, which,
                                    stream);
}

hipError_t launch_msssimf_grad_from(uint32_t first, uint32_t radius, const float (&taps)[kSKMaxRadius + 1], const PairFDesc* descs_dev,
                                    const GradFDesc* grads_dev, uint32_t count, uint32_t width, uint32_t height, uint32_t scales, float data_range,
                                    const double* weights, const double* means, const float* g_out, float* coef, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_call(count, width, height, scales, data_range, weights) || which < 1 || which > 3 || first > 1 || radius != MAXR)
        return hipErrorInvalidValue;
    hipError_t e = launch_msssimf_coef(count, width, height, scales, weights, means, g_out, coef, stream);
    if (e != hipSuccess) return e;
    if ((e = launch_pyramid(first, descs_dev, count, width, height, scales, stream)) != hipSuccess) return e;
    for (uint32_t s = scales; s-- > first;) {
        const bool last = s + 1 == scales;
        Grad2Args<PairFDesc, GradFDesc> ka = fill_grad(msf_dim(width, s), msf_dim(height, s), descs_dev + (size_t)s * count, grads_dev + (size_t)s * count,
                                                       data_range, MAXR, taps);
        ka.up = last ? nullptr : grads_dev + (size_t)(s + 1) * count;
        ka.g_out = coef + s; ka.g_out_stride = scales;      // k_s of pair i at coef[i * scales + s]
        pick_bool(last, [&](auto l) {
            pick_which(which, [&](auto wh) {
                hipLaunchKernelGGL((msssimf_grad_kernel<decltype(wh)::value, decltype(l)::value>), grad_grid(ka, count), dim3(256), 0, stream, ka);
            });
        });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace ssim_hip
