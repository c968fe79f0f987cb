// ssimk_kernels.hip -- gfx950 kernels of SSIM on float32 samples, and of its gradient, under a window of 3, 5, 7 or 9 taps (radius
// R = 1 .. 4), behind rmgr_ssim_hip_enqueue_ssimf_win, rmgr_ssim_hip_compute_ssimf_win_device / _host, rmgr_ssim_hip_enqueue_ssimf_win_grad
// and rmgr_ssim_hip_enqueue_ssimf_win_map_grad.  The definition they implement is in include/rmgr/ssim-hip.h (rmgr_ssim_hip_Window);
// tests/ssimk_model.py restates it in float64 and restates the arithmetic below in fp32.  Windows of 11 taps run on ssimf_kernels.hip and
// ssimw_kernels.hip with the window's taps; this file also holds the taps rule of every window (window_taps).
//
// This is the flow of ssimf_kernels.hip, copied -- not included: that file's kernels are counted by its tests -- and templated on the
// radius, and built with the same flags (-ffp-contract=off).  What the radius changes:
//  * ssimk_strip_kernel<R, MAP, WIDE>: register rings of 2R + 1 entries, 2R warm-up rows from source row y0 - R on, the finished row is
//    r - R; a lane reads its 2R + 2 window pixels (columns x - R .. x + R + 1 of its first column x) as R + 1 aligned 16-byte LDS reads from
//    a slot that starts R columns left of the strip (PAD = R keeps 2 lane + PAD - R even).  A window never reads beyond its radius: a NaN
//    sample reaches the (2R + 1)^2 map pixels around it and no others.
//  * ssimk_grad_kernel<R, WHICH>: the tile + 2R of samples, the tile + R of statistics, adjoint weights over |j| <= R.  One kernel serves
//    both upstream forms: k = float(double(gOut) / (double(W) double(H))) for the whole launch, or k(p) = gMap(p) read per pixel -- a
//    branch on a kernel argument; the product k d is the same instruction in both, so a constant plane gives the scalar form's bits.
//  * ssimk_reduce_kernel: a copy of ssimf_reduce_kernel.
// Centring, cells, tiles and summation orders: see the top of ssimf_kernels.hip; they are position-based and do not depend on the radius.
#include "ssimk_kernels.h"
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace ssim_hip {
namespace {

typedef float  f2 __attribute__((ext_vector_type(2)));
typedef float  f4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

typedef const uint8_t __attribute__((address_space(1)))*    gptr_u8;
typedef const float __attribute__((address_space(1)))*      gptr_cf32;
typedef float __attribute__((address_space(1)))*            gptr_f32;
typedef double __attribute__((address_space(1)))*           gptr_f64;
typedef const PairFDesc __attribute__((address_space(1)))* gptr_descf;

__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float opaque(float v) { asm("" : "+v"(v)); return v; }

__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Row pass of the lane's two columns, centre tap first, the two dependent chains interleaved.
template <int R>
__device__ __forceinline__ void rows_pair(f2& hA, f2& hB, const f2 (&a)[R + 1], const f2 (&b)[R + 1], const float (&g)[R + 1])
{
    hA = a[0] * f2{g[0], g[0]};
    hB = b[0] * f2{g[0], g[0]};
#pragma unroll
    for (int k = 1; k <= R; ++k) {
        hA = fma_(a[k], f2{g[k], g[k]}, hA);
        hB = fma_(b[k], f2{g[k], g[k]}, hB);
    }
}
// Column pass: the ring scatter.  acc[k] is the running sum of output row (r - R + k) while source row r is processed.
// KMIN (warm-up rows only): ring entries below KMIN stand for rows above the strip and are never read.
template <int R, int KMIN>
__device__ __forceinline__ void columns_pair(f2 (&accA)[2 * R + 1], f2 (&accB)[2 * R + 1], f2 hA, f2 hB, const float (&g)[R + 1])
{
#pragma unroll
    for (int k = 0; k < 2 * R; ++k) {
        const int t = k < R ? R - k : k - R;
        if (k >= KMIN) {
            accA[k] = fma_(hA, f2{g[t], g[t]}, accA[k + 1]);
            accB[k] = fma_(hB, f2{g[t], g[t]}, accB[k + 1]);
        }
    }
    accA[2 * R] = hA * f2{g[R], g[R]};
    accB[2 * R] = hB * f2{g[R], g[R]};
}
template <int R, int KMIN>
__device__ __forceinline__ void blur_pair(f2 (&accA)[2 * R + 1], f2 (&accB)[2 * R + 1], const f2 (&a)[R + 1], const f2 (&b)[R + 1], const float (&g)[R + 1])
{
    f2 hA, hB;
    rows_pair<R>(hA, hB, a, b, g);
    columns_pair<R, KMIN>(accA, accB, hA, hB, g);
}

// SSIM of the lane's two columns from the centred moments (ssim_px2 of ssimf_kernels.hip).
__device__ __forceinline__ f2 ssim_px2(f2 m0, f2 m1, f2 e0, f2 e1, f2 cen, float c1, float c2)
{
    const f2 q0 = m0 * m0, q1 = m1 * m1;
    const f2 pc = {opaque(m0.x * m0.y), opaque(m1.x * m1.y)};
    const f2 tc = {opaque(q0.x + q0.y), opaque(q1.x + q1.y)};
    const f2 sS = {opaque(e0.x - tc.x), opaque(e1.x - tc.y)};
    const f2 sAB = {opaque(e0.y - pc.x), opaque(e1.y - pc.y)};
    const f2 u0 = m0 + cen, u1 = m1 + cen;
    const f2 v0 = u0 * u0, v1 = u1 * u1;
    const f2 muAB = {opaque(u0.x * u0.y), opaque(u1.x * u1.y)};
    const f2 tm = {opaque(v0.x + v0.y), opaque(v1.x + v1.y)};
    const f2 two = {2.0f, 2.0f}, C1 = {c1, c1}, C2 = {c2, c2};
    const f2 n = fma_(two, muAB, C1) * fma_(two, sAB, C2);
    const f2 den = (tm + C1) * (sS + C2);
    const f2 r = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    return n * r;
}

enum { MAXR = 4 };

struct KKArgs {
    const PairFDesc* descs;
    uint32_t width, height, strip_rows, strips_x, strips_y;
    uint32_t cells_x, cells_y, cell_shift;
    uint32_t count, xcds;
    double*  partials;            // [image][cell_y][cell_x]
    float    c1, c2, range;
    float    gf[MAXR + 1];
};

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Workgroup g of `total` -> its place in the strip list when each XCD walks one contiguous share of it (ssimf_kernels.hip).
__device__ __forceinline__ uint32_t xcd_order(uint32_t g, uint32_t total, uint32_t xcds)
{
    uint32_t xcd, slot, q, rem;
    if (xcds == 8) { xcd = g & 7u; slot = g >> 3; q = total >> 3; rem = total & 7u; }
    else           { slot = g / xcds; xcd = g - slot * xcds; q = total / xcds; rem = total - q * xcds; }
    return xcd * q + (xcd < rem ? xcd : rem) + slot;
}

// Cells are reduced eight at a time, as fixed trees (ssimf_kernels.hip; ssim_kernels.hip has the long form).
enum { CELL_BATCH = 8 };
struct CellBatch { double leaf[CELL_BATCH][64]; };

#define SK_DPP_ADD(t, CTRL) do {                                                                             \
        const int lo_ = __builtin_amdgcn_update_dpp(0, __double2loint(t), (CTRL), 0xF, 0xF, false);           \
        const int hi_ = __builtin_amdgcn_update_dpp(0, __double2hiint(t), (CTRL), 0xF, 0xF, false);           \
        (t) += __hiloint2double(hi_, lo_);                                                                    \
    } while (0)
enum { DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E };

__device__ __forceinline__ double cell_batch_local(const CellBatch& cb, int lane)
{
    const d2* p = reinterpret_cast<const d2*>(&cb.leaf[0][0]) + 4 * lane;
    d2 v = p[0];
    double a = v.x + v.y;
    __builtin_amdgcn_sched_barrier(0);
    v = p[1];
    a = a + (v.x + v.y);
    __builtin_amdgcn_sched_barrier(0);
    v = p[2];
    double b = v.x + v.y;
    __builtin_amdgcn_sched_barrier(0);
    v = p[3];
    b = b + (v.x + v.y);
    return a + b;
}

// A leaf is the lane's column pair; leaves 0-31 of a batch row are cell 2 sx, leaves 32-63 cell 2 sx + 1.
__device__ __forceinline__ void cell_batch_flush(const KKArgs& args, uint32_t img, uint32_t sx, const CellBatch& cb, uint32_t cell_y_first, uint32_t n)
{
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    double t = cell_batch_local(cb, lane);
    SK_DPP_ADD(t, DPP_QUAD_XOR1);
    SK_DPP_ADD(t, DPP_QUAD_XOR2);
    const uint32_t c = (uint32_t)lane >> 3, cx = 2u * sx + (((uint32_t)lane >> 2) & 1u);
    if ((lane & 3) == 0 && c < n && cx < args.cells_x)
        ((gptr_f64)args.partials)[((size_t)img * args.cells_y + cell_y_first + c) * args.cells_x + cx] = t;
}

// LDS slot = one source row of 128 + 2R pixels starting R columns left of the strip: a lane's 2R + 2 window pixels (columns x - R ..
// x + R + 1 of its first column x) start on the even slot pixel 2 lane and are R + 1 aligned 16-byte reads per plane; the last lane's
// window ends on the slot's last pixel.
template <int R>
struct Slot {
    static constexpr int STRIP_W = kSFStripW, PAD = R, ROW_PX = STRIP_W + 2 * R;
    f2 ab[ROW_PX];   // (a', b')
    f2 q[ROW_PX];    // (a'^2 + b'^2, a'b')
};

enum { ROW_WARMUP = 0, ROW_MAIN = 1, ROW_LAST = 2 };

// R: the window's radius.  MAP: 0 no map; 1 a map of any ssimStep (one 4-byte store per column).
// WIDE: 64-bit lane offsets for the samples and the map (pairs that fail fitsf_narrow()); the map then goes out as plain guarded stores.
template <int R, int MAP, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void ssimk_strip_kernel(const KKArgs args)
{
    static_assert(R >= 1 && R <= MAXR, "radius");
    constexpr int PAD = Slot<R>::PAD, ROW_PX = Slot<R>::ROW_PX;
    constexpr int N = 2 * R + 1;                     // ring entries
    constexpr int NWIN = 2 * R + 2;                  // window pixels of a lane's two columns
    constexpr int NLOAD = 3;                         // samples each lane stages per row and image (192 >= ROW_PX)
    static_assert((PAD - R) % 2 == 0 && 126 + PAD - R + NWIN <= ROW_PX && ROW_PX <= 64 * NLOAD, "slot");
    typedef typename std::conditional<WIDE, int64_t, uint32_t>::type Off;

    __shared__ __attribute__((aligned(16))) Slot<R> ring[2];
    __shared__ __attribute__((aligned(16))) CellBatch cells;

    const int lane = threadIdx.x;
    float gf[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) gf[i] = args.gf[i];

    // the strip: image-major, then strip row, then strip column, each XCD walking a contiguous share of that list
    const uint32_t per_img = args.strips_x * args.strips_y;
    const uint32_t id = xcd_order(blockIdx.x, per_img * args.count, args.xcds);
    const uint32_t img = id / per_img, lin = id - img * per_img;
    const uint32_t sy = lin / args.strips_x, sx = lin - sy * args.strips_x;
    PairFDesc pd;
    {
        const gptr_descf gd = (gptr_descf)args.descs + img;
        pd.a = (const float*)uniform64((int64_t)gd->a); pd.a_step = uniform64(gd->a_step); pd.a_stride = uniform64(gd->a_stride);
        pd.b = (const float*)uniform64((int64_t)gd->b); pd.b_step = uniform64(gd->b_step); pd.b_stride = uniform64(gd->b_stride);
        pd.map = (float*)uniform64((int64_t)gd->map); pd.map_step = uniform64(gd->map_step); pd.map_stride = uniform64(gd->map_stride);
    }
    const int W = (int)args.width, H = (int)args.height;
    const int x0 = (int)(sx * Slot<R>::STRIP_W), y0 = (int)(sy * args.strip_rows);
    const int y_end = y0 + (int)args.strip_rows < H ? y0 + (int)args.strip_rows : H;

    // the strip column's centre (top of ssimf_kernels.hip), per image
    f2 cen;
    {
        const int64_t cx = x0 + 64 < W ? x0 + 64 : W - 1, cy = (H - 1) / 2;
        const float sa = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, ((gptr_cf32)pd.a)[cx * pd.a_step + cy * pd.a_stride])));
        const float sb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, ((gptr_cf32)pd.b)[cx * pd.b_step + cy * pd.b_stride])));
        cen = f2{__builtin_fabsf(sa) <= args.range ? sa : 0.0f, __builtin_fabsf(sb) <= args.range ? sb : 0.0f};
    }

    // Per-lane staging columns: pixel p of the slot is image column clamp(x0 - PAD + p).  Addresses: a wave-uniform row base plus
    // a non-negative lane offset in bytes from the strip's lowest-addressed column.
    auto clampx = [&](int x) { return x < 0 ? 0 : (x > W - 1 ? W - 1 : x); };
    const int x_lo = clampx(x0 - PAD), x_hi = clampx(x0 - PAD + ROW_PX - 1);
    const int refA = pd.a_step >= 0 ? x_lo : x_hi, refB = pd.b_step >= 0 ? x_lo : x_hi;
    const gptr_u8 baseA = (gptr_u8)(pd.a + (int64_t)refA * pd.a_step);
    const gptr_u8 baseB = (gptr_u8)(pd.b + (int64_t)refB * pd.b_step);
    int sp[NLOAD];
    Off offA[NLOAD], offB[NLOAD];
#pragma unroll
    for (int t = 0; t < NLOAD; ++t) {
        int p = lane + 64 * t;
        p = p < ROW_PX ? p : ROW_PX - 1;
        const int xg = clampx(x0 - PAD + p);
        sp[t] = p;
        offA[t] = (Off)((int64_t)(xg - refA) * pd.a_step * 4);
        offB[t] = (Off)((int64_t)(xg - refB) * pd.b_step * 4);
    }

    float va[NLOAD], vb[NLOAD];
    auto fetch_to = [&](int r, float (&oa)[NLOAD], float (&ob)[NLOAD]) {     // row r (clamped) -> registers
        const int ry = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
        const gptr_u8 ra = baseA + (int64_t)ry * pd.a_stride * 4;
        const gptr_u8 rb = baseB + (int64_t)ry * pd.b_stride * 4;
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            if constexpr (!WIDE) asm volatile("" : "+v"(offA[t]), "+v"(offB[t]));   // keeps the zero-extension foldable into the load
            oa[t] = *(gptr_cf32)(ra + offA[t]);
            ob[t] = *(gptr_cf32)(rb + offB[t]);
        }
    };
    auto fetch = [&](int r) { fetch_to(r, va, vb); };
    auto stage_from = [&](Slot<R>& s, const float (&ia)[NLOAD], const float (&ib)[NLOAD]) {   // registers -> the two planes of a slot
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            const f2 ab = f2{ia[t], ib[t]} - cen;         // (a', b')
            const float a = ab.x, b = ab.y;
            const int p = sp[t];
            s.ab[p] = ab;
            s.q[p] = f2{__builtin_fmaf(b, b, a * a), a * b};
        }
    };
    auto stage = [&](Slot<R>& s) { stage_from(s, va, vb); };

    f2 accAB[2][N], accQ[2][N];
#pragma unroll
    for (int k = 0; k < N; ++k) accAB[0][k] = accAB[1][k] = accQ[0][k] = accQ[1][k] = f2{0.0f, 0.0f};
    double colsum[2] = {0.0, 0.0};

    const int r_begin = y0 - R;
    {
        float a0[NLOAD], b0[NLOAD], a1[NLOAD], b1[NLOAD];
        fetch_to(r_begin, a0, b0);
        fetch_to(r_begin + 1, a1, b1);
        fetch(r_begin + 2);
        stage_from(ring[0], a0, b0);
        stage_from(ring[1], a1, b1);
    }
    wave_sync();

    // Map addressing: uniform row base + non-negative per-column offset (bytes; WIDE: elements).
    const int refM = pd.map_step >= 0 ? x0 : (x0 + Slot<R>::STRIP_W - 1 < W ? x0 + Slot<R>::STRIP_W - 1 : W - 1);
    const bool has_map = pd.map != nullptr;
    const int  map_records = has_map ? 0x7FFFFFFF : 0;
    Off  offM[2] = {0, 0};
    bool col_ok[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int x = x0 + 2 * lane + c;
        col_ok[c] = x < W;
        if constexpr (MAP != 0) {
            if constexpr (WIDE) offM[c] = (Off)((int64_t)(x - refM) * pd.map_step);
            else                offM[c] = col_ok[c] ? (Off)((int64_t)(x - refM) * pd.map_step * 4) : (Off)0x80000000u;
        }
    }

    f2 wab[NWIN], wq[NWIN];
    const int e = 2 * lane + PAD - R;                     // even: the 16-byte reads are aligned
    auto load_ab = [&](const Slot<R>& s) {
#pragma unroll
        for (int t = 0; t <= R; ++t) {
            const f4 v = *reinterpret_cast<const f4*>(&s.ab[e + 2 * t]);
            wab[2 * t] = v.xy; wab[2 * t + 1] = v.zw;
        }
    };
    // The folded sums of a window, centre first: column c of the lane's pair has its centre at window pixel R + c.
    auto fold = [&](f2 (&s)[2][R + 1], const f2 (&w)[NWIN]) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int m = R + c;
            s[c][0] = w[m];
#pragma unroll
            for (int i = 1; i <= R; ++i) s[c][i] = w[m + i] + w[m - i];
        }
    };
    // The (a', b') row pass of the row about to be blurred: computed at the end of the previous iteration and carried over.
    f2 hab[2];
    auto fold_ab = [&]() {
        f2 s[2][R + 1];
        fold(s, wab);
        rows_pair<R>(hab[0], hab[1], s[0], s[1], gf);
    };
    load_ab(ring[0]);
    fold_ab();

    auto row = [&](const int r, auto slot, auto phase_tag, auto kmin_tag) {
        constexpr int cur = decltype(slot)::value;
        constexpr int phase = decltype(phase_tag)::value;
        constexpr int KMIN = decltype(kmin_tag)::value;
        const Slot<R>& s = ring[cur];
        __builtin_amdgcn_s_setprio(2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t <= R; ++t) {
            const f4 u = *reinterpret_cast<const f4*>(&s.q[e + 2 * t]);
            wq[2 * t] = u.xy;  wq[2 * t + 1] = u.zw;
        }
        __builtin_amdgcn_sched_barrier(0);
        columns_pair<R, KMIN>(accAB[0], accAB[1], hab[0], hab[1], gf);
        __builtin_amdgcn_sched_barrier(0);
        {
            f2 sq[2][R + 1];
            fold(sq, wq);
            blur_pair<R, KMIN>(accQ[0], accQ[1], sq[0], sq[1], gf);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ring entry 0 is now the finished output row r - R
        if constexpr (phase != ROW_WARMUP) {
            const f2 v = ssim_px2(accAB[0][0], accAB[1][0], accQ[0][0], accQ[1][0], cen, args.c1, args.c2);
            colsum[0] += (double)v.x;
            colsum[1] += (double)v.y;
            if constexpr (MAP != 0) {
                const int y = r - R;
                float* mrow = pd.map + ((int64_t)y * pd.map_stride + (int64_t)refM * pd.map_step);
                const float v0 = v.x, v1 = v.y;
                if constexpr (WIDE) {
                    if (has_map && col_ok[0]) ((gptr_f32)mrow)[offM[0]] = v0;
                    if (has_map && col_ok[1]) ((gptr_f32)mrow)[offM[1]] = v1;
                } else {
                    // branch-free: a raw buffer over [row base, +2 GiB) -- empty for a pair without a map in a batch with maps --;
                    // lanes with nothing to store present an offset beyond it
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(mrow, 0, map_records, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v0), rs, offM[0], 0, 2);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v1), rs, offM[1], 0, 2);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (phase != ROW_LAST) {
            __builtin_amdgcn_sched_barrier(0);
            load_ab(ring[cur ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
            wave_sync();
            stage(ring[cur]);                             // row r+2 replaces row r
            fetch(r + 3);
            wave_sync();
            __builtin_amdgcn_sched_barrier(0);
            fold_ab();                                    // row r+1
        }
    };
    typedef std::integral_constant<int, 0> S0;
    typedef std::integral_constant<int, 1> S1;
    typedef std::integral_constant<int, ROW_WARMUP> Warm;
    typedef std::integral_constant<int, 0> K0;
    int r = r_begin;
    // the 2R warm-up rows in pairs (the two LDS slots); warm-up row i only feeds ring entries k >= 2R - i: the first pair skips the
    // others, the later pairs run as one loop over the full ring (what they write below 2R - i stands for rows above the strip and
    // leaves the ring before the first finished row is read)
    row(r, S0(), Warm(), std::integral_constant<int, 2 * R - 1>());
    row(r + 1, S1(), Warm(), std::integral_constant<int, 2 * R - 1>());
    r += 2;
#pragma unroll 1
    for (int i = 1; i < R; ++i, r += 2) {
        row(r, S0(), Warm(), K0());
        row(r + 1, S1(), Warm(), K0());
    }
    // main rows, one reduction cell at a time; only the image's last cell can be shorter (or odd)
    const int cell_rows = 1 << args.cell_shift;
    uint32_t cell_y = (uint32_t)y0 >> args.cell_shift, parked = 0;
#pragma unroll 1
    for (int left = y_end - y0; left > 0; left -= cell_rows) {
        const int rows = left < cell_rows ? left : cell_rows;
#pragma unroll 1
        for (int i = rows >> 1; i > 0; --i, r += 2) {
            row(r, S0(), std::integral_constant<int, ROW_MAIN>(), K0());
            row(r + 1, S1(), std::integral_constant<int, ROW_MAIN>(), K0());
        }
        if (rows & 1)
            row(r, S0(), std::integral_constant<int, ROW_LAST>(), K0());
        cells.leaf[parked][lane] = (col_ok[0] ? colsum[0] : 0.0) + (col_ok[1] ? colsum[1] : 0.0);
        colsum[0] = colsum[1] = 0.0;
        if (++parked == CELL_BATCH) {
            wave_sync();
            cell_batch_flush(args, img, sx, cells, cell_y, parked);
            wave_sync();
            cell_y += parked;
            parked = 0;
        }
    }
    if (parked) {
        wave_sync();
        cell_batch_flush(args, img, sx, cells, cell_y, parked);
    }
}

// Per-image sum of the cell partials in a fixed order (ssimf_reduce_kernel): thread t of 1024 adds cells t, t + 1024, ... in that order,
// each wave runs a fixed xor butterfly, and the 16 wave totals are added in wave order.  One workgroup per image.
constexpr int kReduceThreads = 1024;

__global__ __launch_bounds__(kReduceThreads) void ssimk_reduce_kernel(const double* __restrict__ partials, uint64_t per_image, double* __restrict__ sums)
{
    __shared__ double sh[kReduceThreads / 64];
    const double* p = partials + (size_t)blockIdx.x * per_image;
    double acc = 0.0;
    for (uint64_t i = threadIdx.x; i < per_image; i += kReduceThreads)
        acc += p[i];
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
        sums[blockIdx.x] = t;
    }
}

uint32_t cell_rows_of(uint32_t height) { return height >= 2048 ? 32u : 8u; }       // as ssimf_kernels.hip: the cells are the same

// ---- the gradient ------------------------------------------------------------------------------------------------------------
// ssimk_grad_kernel: ssimf_grad_kernel / ssimw_grad_kernel for radius R.  One 256-lane workgroup = one 32 x 32 tile of gradient pixels
// at an absolute position; everything between the samples and the gradient stays in LDS.
//   1. the centred samples (a', b') of the tile + 2R (edge-clamped coordinates) -> LDS;
//   2. row pass of (a', b') and (a'^2 + b'^2, a'b') on 32 + 4R rows x 32 + 2R columns, folded sums and tap order as the forward kernel;
//   3. column pass on the tile + R, in source-row order as the forward kernel; per pixel the SSIM terms and the weighted partials
//      k d_mu, k d_aa, k d_ab, plain fp32 products (k = 0 does not hide a NaN statistic) -> LDS; a position outside the image holds 0
//      and reads nothing from gMap;
//   4. adjoint row pass, 5. adjoint column pass, both as gathers: gradient pixel q collects w(q, j) v(q + j), j = -R .. R in that
//      order, the first product plain, the others fused; w(q, j) is the tap g|j| in the interior, tail[|j|] = g|j| + ... + gR on the
//      first (last) row or column for j >= 0 (j <= 0), and the sum of all taps on an axis of size 1;
//   6. dLoss/da = Gt(k d_mu_a) + 2 a' Gt(k d_aa) + b' Gt(k d_ab), one store per pixel.
// Every gradient pixel is written by one work-item in a fixed order, and the tile grid is fixed by the image: no atomics, the same
// bits in any batch.
enum { GT = kSFTile };

struct KKGArgs {
    const PairFDesc*    descs;
    const GradFDesc*    grads;
    const float*        g_out;       // the scalar upstream form, or NULL
    const GradOutFDesc* gouts;       // the per-pixel upstream form (g_out == NULL)
    uint32_t width, height, tiles_x, tiles_y;
    float    c1, c2, range;
    float    gf[MAXR + 1], tail[MAXR + 1], total;
};

// w(q, j) above for an axis of n pixels.
template <int R>
__device__ __forceinline__ float adjoint_weight(int q, int n, int j, const float (&g)[R + 1], const float (&tail)[R + 1], float total)
{
    const int aj = j < 0 ? -j : j;
    float w = g[aj];
    if (q == 0) w = j >= 0 ? tail[aj] : 0.0f;
    if (q == n - 1) w = j <= 0 ? tail[aj] : 0.0f;
    if (n == 1) w = j == 0 ? total : 0.0f;
    return w;
}

// WHICH: 1 dLoss/dA, 2 dLoss/dB, 3 both.  The statistics are computed in the same (a, b) order in all three, so a gradient has
// the same bits alone and together with the other.
template <int R, int WHICH>
__global__ __launch_bounds__(256)
void ssimk_grad_kernel(const KKGArgs args)
{
    static_assert(R >= 1 && R <= MAXR, "radius");
    constexpr int GIN = GT + 4 * R, GST = GT + 2 * R, N = 2 * R + 1;
    constexpr int NP = WHICH == 3 ? 4 : 3;                       // partial planes: d_mu (of A, or of the one wanted), d_aa, d_ab, d_mu of B
    constexpr int XN = 2 * GIN * GIN > NP * GST * GST ? 2 * GIN * GIN : NP * GST * GST;
    constexpr int YN = 4 * GIN * GST;                            // >= NP * GST * GT
    static_assert(YN >= NP * GST * GT, "Q fits");
    __shared__ __attribute__((aligned(16))) float lds[XN + YN];
    f2*    in  = reinterpret_cast<f2*>(lds);                     // [GIN][GIN] (a', b')
    float* P   = lds;                                            // [NP][GST][GST], after the row pass has consumed `in`
    f2*    Hab = reinterpret_cast<f2*>(lds + XN);                // [GIN][GST] row pass of (a', b')
    f2*    Hq  = Hab + GIN * GST;                                // [GIN][GST] row pass of (a'^2 + b'^2, a'b')
    float* Q   = lds + XN;                                       // [NP][GST][GT], after the column pass has consumed Hab, Hq

    const int tid = threadIdx.x;
    const int W = (int)args.width, H = (int)args.height;
    const uint32_t per_img = args.tiles_x * args.tiles_y;
    const uint32_t img = blockIdx.x / per_img, lin = blockIdx.x - img * per_img;
    const uint32_t ty = lin / args.tiles_x, tx = lin - ty * args.tiles_x;
    const int x0 = (int)(tx * GT), y0 = (int)(ty * GT);
    const PairFDesc pd = args.descs[img];
    const GradFDesc gd = args.grads[img];
    const gptr_cf32 pa = (gptr_cf32)pd.a, pb = (gptr_cf32)pd.b;
    float gf[R + 1], tail[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) { gf[i] = args.gf[i]; tail[i] = args.tail[i]; }
    // the upstream gradient: one k for the launch's pair, or a plane read per pixel
    const bool per_pixel = args.g_out == nullptr;
    GradOutFDesc go = {nullptr, 0, 0};
    float k_uniform = 0.0f;
    if (per_pixel) go = args.gouts[img];
    else           k_uniform = (float)((double)((gptr_cf32)args.g_out)[img] / ((double)W * (double)H));
    const gptr_cf32 pk = (gptr_cf32)go.g;

    f2 cen;                                                      // the strip column's centre (top of ssimf_kernels.hip)
    {
        const int xs = x0 & ~(kSFStripW - 1);
        const int64_t cx = xs + 64 < W ? xs + 64 : W - 1, cy = (H - 1) / 2;
        const float sa = pa[cx * pd.a_step + cy * pd.a_stride], sb = pb[cx * pd.b_step + cy * pd.b_stride];
        cen = f2{__builtin_fabsf(sa) <= args.range ? sa : 0.0f, __builtin_fabsf(sb) <= args.range ? sb : 0.0f};
    }

    // 1. samples
    for (int idx = tid; idx < GIN * GIN; idx += 256) {
        const int j = idx / GIN, i = idx - j * GIN;
        int x = x0 - 2 * R + i, y = y0 - 2 * R + j;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        const f2 v = {pa[(int64_t)x * pd.a_step + (int64_t)y * pd.a_stride], pb[(int64_t)x * pd.b_step + (int64_t)y * pd.b_stride]};
        in[idx] = v - cen;
    }
    __syncthreads();

    // 2. row pass: H*[j][u] is the blur along x at image column x0 - R + u of source row y0 - 2R + j
    for (int idx = tid; idx < GIN * GST; idx += 256) {
        const int j = idx / GST, u = idx - j * GST;
        const f2* row = in + j * GIN + u;
        f2 ab[N], q[N];
#pragma unroll
        for (int t = 0; t < N; ++t) {
            ab[t] = row[t];
            q[t] = f2{__builtin_fmaf(ab[t].y, ab[t].y, ab[t].x * ab[t].x), ab[t].x * ab[t].y};
        }
        f2 sab[R + 1], sq[R + 1];
        sab[0] = ab[R]; sq[0] = q[R];
#pragma unroll
        for (int i = 1; i <= R; ++i) { sab[i] = ab[R + i] + ab[R - i]; sq[i] = q[R + i] + q[R - i]; }
        f2 hab, hq;
        rows_pair<R>(hab, hq, sab, sq, gf);
        Hab[idx] = hab;
        Hq[idx] = hq;
    }
    __syncthreads();

    // 3. column pass, SSIM terms, weighted partials
    for (int idx = tid; idx < GST * GST; idx += 256) {
        const int v = idx / GST, u = idx - v * GST;
        const int px = x0 - R + u, py = y0 - R + v;
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (px >= 0 && px < W && py >= 0 && py < H) {
            float k = k_uniform;
            if (per_pixel) k = pk[(int64_t)px * go.g_step + (int64_t)py * go.g_stride];     // in flight during the column pass
            const f2* cab = Hab + v * GST + u;
            const f2* cq = Hq + v * GST + u;
            f2 m = cab[0] * f2{gf[R], gf[R]}, e = cq[0] * f2{gf[R], gf[R]};
#pragma unroll
            for (int t = 1; t < N; ++t) {
                const float w = gf[t < R ? R - t : t - R];
                m = fma_(cab[t * GST], f2{w, w}, m);
                e = fma_(cq[t * GST], f2{w, w}, e);
            }
            // the forward kernel's terms (ssim_px2), then the derivative
            const float pc = opaque(m.x * m.y), tc = opaque(opaque(m.x * m.x) + opaque(m.y * m.y));
            const float sS = opaque(e.x - tc), sAB = opaque(e.y - pc);
            const float uA = m.x + cen.x, uB = m.y + cen.y;
            const float muAB = opaque(uA * uB), tm = opaque(opaque(uA * uA) + opaque(uB * uB));
            const float A1 = __builtin_fmaf(2.0f, muAB, args.c1), A2 = __builtin_fmaf(2.0f, sAB, args.c2);
            const float B1 = tm + args.c1, B2 = sS + args.c2;
            const float r1 = __builtin_amdgcn_rcpf(B1), r2 = __builtin_amdgcn_rcpf(B2);
            const float r12 = opaque(r1 * r2);
            const float ssim = opaque(opaque(A1 * A2) * r12);
            const float dab = opaque(opaque(2.0f * A1) * r12);
            const float daa = -opaque(ssim * r2);
            const float f1 = opaque(A2 * r12), f2_ = opaque(ssim * r1);
            const float dmA = opaque(opaque(opaque(opaque(2.0f * uB) * f1) - opaque(opaque(2.0f * uA) * f2_)) - opaque(opaque(2.0f * m.x) * daa)) - opaque(m.y * dab);
            const float dmB = opaque(opaque(opaque(opaque(2.0f * uA) * f1) - opaque(opaque(2.0f * uB) * f2_)) - opaque(opaque(2.0f * m.y) * daa)) - opaque(m.x * dab);
            d[0] = k * (WHICH == 2 ? dmB : dmA);
            d[1] = k * daa;
            d[2] = k * dab;
            d[3] = k * dmB;
        }
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) P[pl * GST * GST + idx] = d[pl];      // `in` is dead: every lane is past the barrier above
    }
    __syncthreads();

    // 4. adjoint row pass: Q[pl][v][x], x = tid % 32 for every position of this lane
    {
        const int x = tid & (GT - 1), qx = x0 + x;
        float wx[N];
#pragma unroll
        for (int j = -R; j <= R; ++j) wx[j + R] = adjoint_weight<R>(qx, W, j, gf, tail, args.total);
        for (int idx = tid; idx < GST * GT; idx += 256) {
            const int v = idx / GT;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
                const float* src = P + pl * GST * GST + v * GST + x;
                float acc = src[0] * wx[0];
#pragma unroll
                for (int t = 1; t < N; ++t) acc = __builtin_fmaf(src[t], wx[t], acc);
                Q[pl * GST * GT + idx] = acc;
            }
        }
    }
    __syncthreads();

    // 5. adjoint column pass, 6. the gradient
    for (int idx = tid; idx < GT * GT; idx += 256) {
        const int y = idx / GT, x = idx - y * GT;
        const int qx = x0 + x, qy = y0 + y;
        if (qx >= W || qy >= H) continue;
        float wy[N];
#pragma unroll
        for (int j = -R; j <= R; ++j) wy[j + R] = adjoint_weight<R>(qy, H, j, gf, tail, args.total);
        float r[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            const float* src = Q + pl * GST * GT + y * GT + x;
            float acc = src[0] * wy[0];
#pragma unroll
            for (int t = 1; t < N; ++t) acc = __builtin_fmaf(src[t * GT], wy[t], acc);
            r[pl] = acc;
        }
        const float a = pa[(int64_t)qx * pd.a_step + (int64_t)qy * pd.a_stride] - cen.x;
        const float b = pb[(int64_t)qx * pd.b_step + (int64_t)qy * pd.b_stride] - cen.y;
        if constexpr (WHICH != 2) {
            const float g = opaque(r[0] + opaque(opaque(2.0f * a) * r[1])) + opaque(b * r[2]);
            ((gptr_f32)gd.ga)[(int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride] = g;
        }
        if constexpr (WHICH != 1) {
            const float g = opaque(r[WHICH == 3 ? 3 : 0] + opaque(opaque(2.0f * b) * r[1])) + opaque(a * r[2]);
            ((gptr_f32)gd.gb)[(int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride] = g;
        }
    }
}

template <int R>
hipError_t launch_strip(const KKArgs& ka, bool map, bool wide, const dim3& grid, hipStream_t stream)
{
    const dim3 block(64);
    if (wide) {
        if (map) hipLaunchKernelGGL((ssimk_strip_kernel<R, 1, true>), grid, block, 0, stream, ka);
        else     hipLaunchKernelGGL((ssimk_strip_kernel<R, 0, true>), grid, block, 0, stream, ka);
    } else if (map) hipLaunchKernelGGL((ssimk_strip_kernel<R, 1, false>), grid, block, 0, stream, ka);
    else            hipLaunchKernelGGL((ssimk_strip_kernel<R, 0, false>), grid, block, 0, stream, ka);
    return hipGetLastError();
}

template <int R>
hipError_t launch_grad(const KKGArgs& ka, int which, const dim3& grid, hipStream_t stream)
{
    const dim3 block(256);
    if (which == 1)      hipLaunchKernelGGL((ssimk_grad_kernel<R, 1>), grid, block, 0, stream, ka);
    else if (which == 2) hipLaunchKernelGGL((ssimk_grad_kernel<R, 2>), grid, block, 0, stream, ka);
    else                 hipLaunchKernelGGL((ssimk_grad_kernel<R, 3>), grid, block, 0, stream, ka);
    return hipGetLastError();
}

} // namespace

bool window_taps(uint32_t radius, uint32_t kind, float sigma, float (&gf)[kSKMaxRadius + 1])
{
    if (radius < 1 || radius > kSKMaxRadius) return false;
    for (int i = 0; i <= kSKMaxRadius; ++i) gf[i] = 0.0f;
    if (kind == kSKUniform) {
        for (uint32_t i = 0; i <= radius; ++i) gf[i] = (float)(1.0 / (double)(2 * radius + 1));
        return true;
    }
    if (kind != kSKGaussian || !(sigma > 0.0f) || !std::isfinite(sigma)) return false;
    const double s = (double)sigma;
    double g[kSKMaxRadius + 1], norm = 0.0;
    for (int i = 0; i <= (int)radius; ++i) {
        g[i] = exp(-(double)(i * i) / (2.0 * s * s));
        norm += (i == 0) ? g[i] : 2.0 * g[i];
    }
    for (int i = 0; i <= (int)radius; ++i) gf[i] = (float)(g[i] / norm);
    return true;
}

void window_tails(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], float (&tail)[kSKMaxRadius + 1], float& total)
{
    for (int i = 0; i <= kSKMaxRadius; ++i) tail[i] = 0.0f;
    double t = 0.0;
    for (int i = (int)radius; i >= 0; --i) { t += (double)gf[i]; tail[i] = (float)t; }
    total = (float)(2.0 * t - (double)gf[0]);
}

GeometryF plank(uint32_t radius, uint32_t width, uint32_t height, uint32_t count, int cu_count)
{
    GeometryF g;
    g.width = width; g.height = height; g.count = count;
    g.cell_rows = cell_rows_of(height);
    g.cells_x = (width + 63) / 64;
    g.cells_y = (height + g.cell_rows - 1) / g.cell_rows;
    g.strips_x = (width + kSFStripW - 1) / kSFStripW;
    // planf()'s choice of the strip height with 2 * radius warm-up rows
    const uint64_t slots = (uint64_t)(cu_count > 0 ? cu_count : 256) * 4 * 3;
    const uint64_t cols = (uint64_t)g.strips_x * count;
    uint64_t best = ~uint64_t(0);
    uint32_t best_rows = g.cell_rows;
    for (uint32_t rows = g.cell_rows; rows <= std::max<uint32_t>(g.cell_rows, 2048); rows += g.cell_rows) {
        const uint64_t per_col = (height + rows - 1) / rows;
        const uint64_t rounds = (cols * per_col + slots - 1) / slots;
        const uint64_t cost = rounds * (std::min<uint64_t>(rows, height) + 2 * radius);
        if (cost <= best) { best = cost; best_rows = rows; }
        if (rows >= height) break;
    }
    g.strip_rows = best_rows;
    g.strips_y = (height + best_rows - 1) / best_rows;
    return g;
}

hipError_t launch_ssimk(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], const GeometryF& geo, const PairFDesc* descs_dev, bool map, bool wide,
                        float data_range, int xcd_count, double* partials, double* sums, hipStream_t stream)
{
    if (geo.count == 0) return hipSuccess;
    if (radius < 1 || radius > MAXR || !(data_range > 0.0f) || !std::isfinite(data_range) || geo.count > ssimf_max_count(geo.width, geo.height))
        return hipErrorInvalidValue;
    KKArgs ka;
    ka.descs = descs_dev;
    ka.width = geo.width; ka.height = geo.height;
    ka.strip_rows = geo.strip_rows; ka.strips_x = geo.strips_x; ka.strips_y = geo.strips_y;
    ka.cells_x = geo.cells_x; ka.cells_y = geo.cells_y;
    ka.cell_shift = geo.cell_rows == 32 ? 5 : 3;
    ka.count = geo.count;
    ka.xcds = xcd_count >= 1 ? (uint32_t)xcd_count : 8u;
    ka.partials = partials;
    ka.range = data_range;
    ssimf_constants(data_range, ka.c1, ka.c2);
    for (int i = 0; i <= MAXR; ++i) ka.gf[i] = gf[i];
    const dim3 grid((uint32_t)((uint64_t)geo.strips_x * geo.strips_y * geo.count));
    hipError_t e;
    switch (radius) {
    case 1:  e = launch_strip<1>(ka, map, wide, grid, stream); break;
    case 2:  e = launch_strip<2>(ka, map, wide, grid, stream); break;
    case 3:  e = launch_strip<3>(ka, map, wide, grid, stream); break;
    default: e = launch_strip<4>(ka, map, wide, grid, stream); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssimk_reduce_kernel, dim3(geo.count), dim3(kReduceThreads), 0, stream, partials, geo.cells_per_image(), sums);
    return hipGetLastError();
}

hipError_t launch_ssimk_grad(uint32_t radius, const float (&gf)[kSKMaxRadius + 1], uint32_t width, uint32_t height, uint32_t count,
                             const PairFDesc* descs_dev, const GradFDesc* grads_dev, const float* g_out, const GradOutFDesc* gouts_dev,
                             float data_range, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (radius < 1 || radius > MAXR || !(data_range > 0.0f) || !std::isfinite(data_range) || which < 1 || which > 3 ||
        (g_out == NULL) == (gouts_dev == NULL) || count > ssimf_max_count(width, height))
        return hipErrorInvalidValue;
    KKGArgs ka;
    ka.descs = descs_dev; ka.grads = grads_dev; ka.g_out = g_out; ka.gouts = g_out ? NULL : gouts_dev;
    ka.width = width; ka.height = height;
    ka.tiles_x = (width + kSFTile - 1) / kSFTile; ka.tiles_y = (height + kSFTile - 1) / kSFTile;
    ka.range = data_range;
    ssimf_constants(data_range, ka.c1, ka.c2);
    float tail[kSKMaxRadius + 1];
    window_tails(radius, gf, tail, ka.total);
    for (int i = 0; i <= MAXR; ++i) { ka.gf[i] = gf[i]; ka.tail[i] = tail[i]; }
    const dim3 grid((uint32_t)((uint64_t)ka.tiles_x * ka.tiles_y * count));
    switch (radius) {
    case 1:  return launch_grad<1>(ka, which, grid, stream);
    case 2:  return launch_grad<2>(ka, which, grid, stream);
    case 3:  return launch_grad<3>(ka, which, grid, stream);
    default: return launch_grad<4>(ka, which, grid, stream);
    }
}

} // namespace ssim_hip
