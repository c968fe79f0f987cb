// msssimh_kernels.hip -- gfx950 kernels of multi-scale SSIM on float16 / bfloat16 samples and of its gradient, behind
// rmgr_ssim_hip_enqueue_msssimh, rmgr_ssim_hip_compute_msssimh_device / _host and rmgr_ssim_hip_enqueue_msssimh_grad.  The definition
// they implement is in include/rmgr/ssim-hip.h: msssimf's, applied to the samples widened to float32, with the gradient rounded once into
// the samples' encoding.
//
// Only scale 0 touches 16-bit memory -- the pyramid is float32 from scale 1 on -- so only scale 0 has kernels here: its strip kernel, its
// pyramid step and its gradient kernel.  The strip kernel and the gradient kernel are those of msssimf_kernels.hip (DESIGN.md sections 12
// to 14 and 17) under the sample policy SampleH<TYPE>; see ssim2_walk.h.  The pyramid step is msssimf_down_kernel with widened loads: from
// the four widened samples on every instruction is msssimf's, and the scale-1 plane has the bits of msssimf on the widened planes.
// Scales >= 1, the reduction, the product and the coefficients run on msssimf_kernels.hip's kernels (launch_msssimf_from,
// launch_msssimf_grad_from) over the same partials layout, pyramid and coarse gradient planes.
//
// Centring, per-pixel values and cells: see the top of ssim2_walk.h; the rules are the same, on the widened samples.
#include "ssim2_walk.h"

namespace ssim_hip {
namespace {

// TYPE: kSHTypeF16 or kSHTypeBF16, the encoding of the samples.  WIDE: 64-bit lane offsets for the samples (pairs that fail fitsh_narrow()).
template <int TYPE, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void msssimh_strip_kernel(const Strip2Args<PairHDesc> args) { strip_body<SampleH<TYPE>, 5, kFormMulti, 0, WIDE>(args); }

// ---- the pyramid step ----------------------------------------------------------------------------------------------------------------

// The pyramid step from scale 0 to scale 1 (msssimf_down_kernel with widened loads): work-item = one pixel of scale 1 of one pair, A
// and B; four widened samples per image at the caller's steps and strides, (top + bot) * 0.25f in that order; dst planes are dense float32
// (step 1, stride dst_w).
template <int TYPE>
__global__ __launch_bounds__(256)
void msssimh_down_kernel(const PairHDesc* __restrict__ src, const PairFDesc* __restrict__ dst, uint32_t src_w, uint32_t src_h,
                         uint32_t dst_w, uint32_t dst_h, uint32_t blocks_per_image)
{
    const uint32_t img = blockIdx.x / blocks_per_image, blk = blockIdx.x - img * blocks_per_image;
    const uint64_t idx = (uint64_t)blk * 256 + threadIdx.x;
    if (idx >= (uint64_t)dst_w * dst_h) return;
    const uint32_t y = (uint32_t)(idx / dst_w), x = (uint32_t)(idx - (uint64_t)y * dst_w);
    const PairHDesc s = src[img];
    const PairFDesc d = dst[img];
    const int64_t x0 = 2 * (int64_t)x, x1 = x0 + 1 < (int64_t)src_w ? x0 + 1 : (int64_t)src_w - 1;
    const int64_t y0 = 2 * (int64_t)y, y1 = y0 + 1 < (int64_t)src_h ? y0 + 1 : (int64_t)src_h - 1;
    {
        const gptr_cu16 p = (gptr_cu16)s.a;
        const float top = widen<TYPE>(p[x0 * s.a_step + y0 * s.a_stride]) + widen<TYPE>(p[x1 * s.a_step + y0 * s.a_stride]);
        const float bot = widen<TYPE>(p[x0 * s.a_step + y1 * s.a_stride]) + widen<TYPE>(p[x1 * s.a_step + y1 * s.a_stride]);
        ((gptr_f32)const_cast<float*>(d.a))[idx] = (top + bot) * 0.25f;
    }
    {
        const gptr_cu16 p = (gptr_cu16)s.b;
        const float top = widen<TYPE>(p[x0 * s.b_step + y0 * s.b_stride]) + widen<TYPE>(p[x1 * s.b_step + y0 * s.b_stride]);
        const float bot = widen<TYPE>(p[x0 * s.b_step + y1 * s.b_stride]) + widen<TYPE>(p[x1 * s.b_step + y1 * s.b_stride]);
        ((gptr_f32)const_cast<float*>(d.b))[idx] = (top + bot) * 0.25f;
    }
}
// LAST: scales == 1, scale 0 is the coarsest (the ssim form, no coarser gradient to add); otherwise the cs form, which adds scale 1's.
template <int TYPE, int WHICH, bool LAST>
__global__ __launch_bounds__(256)
void msssimh_grad_kernel(const Grad2Args<PairHDesc, GradHDesc> args) { grad_body<SampleH<TYPE>, 5, WHICH, kKCoef, LAST ? kMsLast : kMsUp>(args); }

bool valid_type(int type) { return type == kSHTypeF16 || type == kSHTypeBF16; }

// The pyramid step from the caller's planes into row 1 of descs_dev.
template <int TYPE>
void launch_down(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, hipStream_t stream)
{
    const uint32_t dw = msf_dim(width, 1), dh = msf_dim(height, 1);
    const uint32_t per = (uint32_t)(((uint64_t)dw * dh + 255) / 256);
    hipLaunchKernelGGL((msssimh_down_kernel<TYPE>), dim3(per * count), dim3(256), 0, stream, descs0_dev, descs_dev + (size_t)count, width, height, dw, dh, per);
}

} // namespace

hipError_t launch_msssimh_down(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, int type,
                               hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_type(type) || count > msssimf_max_count(width, height)) return hipErrorInvalidValue;
    pick_type(type, [&](auto t) { launch_down<decltype(t)::value>(descs0_dev, descs_dev, count, width, height, stream); });
    return hipGetLastError();
}

hipError_t launch_msssimh(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                          uint32_t scales, int type, bool wide, float data_range, uint32_t radius, const float (&taps)[kSKMaxRadius + 1],
                          const double* weights, int cu_count, int xcd_count, double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_type(type) || !valid_range(data_range) || radius != MAXR || scales < 1 || scales > kMSFMaxScales || count > msssimf_max_count(width, height))
        return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1) {
        pick_type(type, [&](auto t) { launch_down<decltype(t)::value>(descs0_dev, descs_dev, count, width, height, stream); });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // scale 0's strips and cells, as launch_msssimf_from lays them out: its partials come first
    const GeometryF geo = planf(width, height, count, cu_count);
    const Strip2Args<PairHDesc> ka = fill_strip(geo, descs0_dev, data_range, taps, xcd_count, partials);
    pick_type(type, [&](auto t) {
        pick_bool(wide, [&](auto w) {
            hipLaunchKernelGGL((msssimh_strip_kernel<decltype(t)::value, decltype(w)::value>), strip_grid(geo), dim3(64), 0, stream, ka);
        });
    });
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_msssimf_from(1, radius, taps, descs_dev, count, width, height, scales, false, data_range, weights, cu_count, xcd_count, partials, means,
                               values, stream);
}

hipError_t launch_msssimh_grad(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, const GradHDesc* grads0_dev, const GradFDesc* grads_dev,
                               uint32_t count, uint32_t width, uint32_t height, uint32_t scales, int type, float data_range, uint32_t radius,
                               const float (&taps)[kSKMaxRadius + 1], const double* weights, const double* means, const float* g_out, float* coef,
                               int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_type(type) || !valid_range(data_range) || radius != MAXR || scales < 1 || scales > kMSFMaxScales || which < 1 || which > 3 ||
        count > msssimf_max_count(width, height))
        return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1) {
        pick_type(type, [&](auto t) { launch_down<decltype(t)::value>(descs0_dev, descs_dev, count, width, height, stream); });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // the coefficients of every scale, the rest of the pyramid, the float32 gradients from the coarsest scale down to scale 1
    if ((e = launch_msssimf_grad_from(1, radius, taps, descs_dev, grads_dev, count, width, height, scales, data_range, weights, means, g_out, coef, which,
                                      stream)) != hipSuccess)
        return e;
    const bool last = scales == 1;
    Grad2Args<PairHDesc, GradHDesc> ka = fill_grad(width, height, descs0_dev, grads0_dev, data_range, MAXR, taps);
    ka.up = last ? nullptr : grads_dev + (size_t)count;
    ka.g_out = coef; ka.g_out_stride = scales;              // k_0 of pair i at coef[i * scales]
    pick_type(type, [&](auto t) {
        pick_bool(last, [&](auto l) {
            pick_which(which, [&](auto wh) {
                hipLaunchKernelGGL((msssimh_grad_kernel<decltype(t)::value, decltype(wh)::value, decltype(l)::value>), grad_grid(ka, count), dim3(256), 0, stream, ka);
            });
        });
    });
    return hipGetLastError();
}

} // namespace ssim_hip
