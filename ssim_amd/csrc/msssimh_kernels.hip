// msssimh_kernels.hip -- gfx950 kernels of multi-scale SSIM on float16 / bfloat16 samples and of its gradient, behind
// rmgr_ssim_hip_enqueue_msssimh, rmgr_ssim_hip_compute_msssimh_device / _host and rmgr_ssim_hip_enqueue_msssimh_grad.  The definition
// they implement is in include/rmgr/ssim-hip.h: msssimf's, applied to the samples widened to float32, with the gradient rounded once into
// the samples' encoding.
//
// Only scale 0 touches 16-bit memory -- the pyramid is float32 from scale 1 on -- so only scale 0 has kernels here: its strip kernel, its
// pyramid step and its gradient kernel.  They are those of msssimf_kernels.hip, copied, not included (DESIGN.md sections 12 to 14 and 17),
// with the loads and stores of ssimh_kernels.hip:
//  * a sample gets into a register through a 2-byte load and the exact widen<TYPE>; byte offsets scale by 2.  From stage_from on (strip),
//    from the four widened samples on (pyramid step) and from the `in` plane on (gradient) every instruction is msssimf's, built with the
//    same flags (-ffp-contract=off): the cell sums, the scale-1 plane and the float32 gradient have the bits of msssimf on the widened
//    planes;
//  * a gradient pixel leaves through narrow<TYPE>: the float32 value, the coarser scale's gradient included, rounded once to nearest-even,
//    one 2-byte store.
// Scales >= 1, the reduction, the product and the coefficients run on msssimf_kernels.hip's kernels (launch_msssimf_from,
// launch_msssimf_grad_from) over the same partials layout, pyramid and coarse gradient planes.
//
// Centring, per-pixel values and cells: see the top of msssimf_kernels.hip; the rules are the same, on the widened samples.
#include "msssimh_kernels.h"
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
typedef const uint16_t __attribute__((address_space(1)))*   gptr_cu16;
typedef uint16_t __attribute__((address_space(1)))*         gptr_u16;
typedef float __attribute__((address_space(1)))*            gptr_f32;
typedef double __attribute__((address_space(1)))*           gptr_f64;
typedef const PairHDesc __attribute__((address_space(1)))* gptr_desch;

__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float opaque(float v) { asm("" : "+v"(v)); return v; }

// A stored sample -> float32, exactly (ssimh_kernels.hip).
template <int TYPE>
__device__ __forceinline__ float widen(uint16_t s)
{
    if constexpr (TYPE == kSHTypeBF16) return __builtin_bit_cast(float, (uint32_t)s << 16);
    else                               return (float)__builtin_bit_cast(_Float16, s);
}
// float32 -> the samples' encoding, one rounding to nearest-even (ssimh_kernels.hip).
template <int TYPE>
__device__ __forceinline__ uint16_t narrow(float v)
{
    if constexpr (TYPE == kSHTypeBF16) {
        const uint32_t u = __builtin_bit_cast(uint32_t, v);
        const uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;               // no carry out of a finite or infinite value
        return (uint16_t)((u & 0x7FFFFFFFu) > 0x7F800000u ? (u >> 16) | 0x0040u : r);   // NaN: quiet, never rounded into Inf
    } else {
        return __builtin_bit_cast(uint16_t, (_Float16)v);
    }
}

__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Row pass of the lane's two columns, centre tap first, the two dependent chains interleaved.
__device__ __forceinline__ void rows_pair(f2& hA, f2& hB, const f2 (&a)[6], const f2 (&b)[6], const float (&g)[6])
{
    hA = a[0] * f2{g[0], g[0]};
    hB = b[0] * f2{g[0], g[0]};
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        hA = fma_(a[k], f2{g[k], g[k]}, hA);
        hB = fma_(b[k], f2{g[k], g[k]}, hB);
    }
}
// Column pass: the ring scatter.  acc[k] is the running sum of output row (r - 5 + k) while source row r is processed.
// KMIN (warm-up rows only): ring entries below KMIN stand for rows above the strip and are never read.
template <int KMIN = 0>
__device__ __forceinline__ void columns_pair(f2 (&accA)[11], f2 (&accB)[11], f2 hA, f2 hB, const float (&g)[6])
{
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const int t = k < 5 ? 5 - k : k - 5;
        if (k >= KMIN) {
            accA[k] = fma_(hA, f2{g[t], g[t]}, accA[k + 1]);
            accB[k] = fma_(hB, f2{g[t], g[t]}, accB[k + 1]);
        }
    }
    accA[10] = hA * f2{g[5], g[5]};
    accB[10] = hB * f2{g[5], g[5]};
}
template <int KMIN = 0>
__device__ __forceinline__ void blur_pair(f2 (&accA)[11], f2 (&accB)[11], const f2 (&a)[6], const f2 (&b)[6], const float (&g)[6])
{
    f2 hA, hB;
    rows_pair(hA, hB, a, b, g);
    columns_pair<KMIN>(accA, accB, hA, hB, g);
}

// cs and SSIM of the lane's two columns from the centred moments (msssim_px2 of msssimf_kernels.hip): m0, m1 =
// (mu_a', mu_b') of each column, e0, e1 = (E[a'^2 + b'^2], E[a'b']); cen = (cA, cB).
__device__ __forceinline__ f2 msssim_px2(f2 m0, f2 m1, f2 e0, f2 e1, f2 cen, float c1, float c2, f2& cs)
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
    const f2 A2 = fma_(two, sAB, C2), B2 = sS + C2;
    const f2 n = fma_(two, muAB, C1) * A2;
    const f2 den = (tm + C1) * B2;
    const f2 r = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    const f2 r2 = {__builtin_amdgcn_rcpf(B2.x), __builtin_amdgcn_rcpf(B2.y)};
    cs = A2 * r2;
    return n * r;
}

// Scale 0 of one launch: the caller's descriptors, the size and the cell partials (KMArgs of msssimf_kernels.hip).
struct KMHArgs {
    const PairHDesc* descs;
    uint32_t width, height, strip_rows, strips_x, strips_y;
    uint32_t cells_x, cells_y, cell_shift;
    uint32_t count, xcds;
    double*  partials;            // [image][cell_y][cell_x]{cs, ssim}
    float    c1, c2, range;
    float    gf[6];
};

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Workgroup g of `total` -> its place in the strip list when each XCD is to walk one contiguous share of it (neighbouring strips
// share halo cache lines; consecutive workgroup ids go to the XCDs round robin).  A bijection for any total.
__device__ __forceinline__ uint32_t xcd_order(uint32_t g, uint32_t total, uint32_t xcds)
{
    uint32_t xcd, slot, q, rem;
    if (xcds == 8) { xcd = g & 7u; slot = g >> 3; q = total >> 3; rem = total & 7u; }
    else           { slot = g / xcds; xcd = g - slot * xcds; q = total / xcds; rem = total - q * xcds; }
    return xcd * q + (xcd < rem ? xcd : rem) + slot;
}

// Cells are reduced eight at a time (ssim_kernels.hip has the long form): each lane parks its leaf of a cell in LDS, and a
// batch of eight cells is summed as fixed trees -- eight leaves per lane as ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)), then two DPP
// levels over the four lanes of a 32-leaf tree.
enum { CELL_BATCH = 8 };
struct CellBatch { double leaf[CELL_BATCH][64]; };

#define MSH_DPP_ADD(t, CTRL) do {                                                                             \
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

// A leaf is the lane's column pair; leaves 0-31 of a batch row are cell 2 sx, leaves 32-63 cell 2 sx + 1.  which: 0 the cs sum, 1 the
// ssim sum of the cell (adjacent doubles).
__device__ __forceinline__ void cell_batch_flush(const KMHArgs& args, uint32_t img, uint32_t sx, const CellBatch& cb, uint32_t cell_y_first, uint32_t n, uint32_t which)
{
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    double t = cell_batch_local(cb, lane);
    MSH_DPP_ADD(t, DPP_QUAD_XOR1);
    MSH_DPP_ADD(t, DPP_QUAD_XOR2);
    const uint32_t c = (uint32_t)lane >> 3, cx = 2u * sx + (((uint32_t)lane >> 2) & 1u);
    if ((lane & 3) == 0 && c < n && cx < args.cells_x)
        ((gptr_f64)args.partials)[(((size_t)img * args.cells_y + cell_y_first + c) * args.cells_x + cx) * 2 + which] = t;
}

// LDS slot = one source row of 144 pixels starting seven columns left of the strip: a lane's twelve window pixels (columns x-5 ..
// x+6 of its first column x) start on an even slot pixel and are six aligned 16-byte reads per plane.
struct Slot {
    static constexpr int STRIP_W = kSFStripW, PAD = 7, ROW_PX = 144;
    f2 ab[ROW_PX];   // (a', b')
    f2 q[ROW_PX];    // (a'^2 + b'^2, a'b')
};

enum { ROW_WARMUP = 0, ROW_MAIN = 1, ROW_LAST = 2 };

// WIDE: 64-bit lane offsets for the samples (pairs that fail fitsh_narrow()).
// TYPE: kSHTypeF16 or kSHTypeBF16, the encoding of the samples.
template <int TYPE, bool WIDE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void msssimh_strip_kernel(const KMHArgs args)
{
    constexpr int PAD = Slot::PAD, ROW_PX = Slot::ROW_PX;
    constexpr int NLOAD = 3;                         // samples each lane stages per row and image
    typedef typename std::conditional<WIDE, int64_t, uint32_t>::type Off;

    __shared__ __attribute__((aligned(16))) Slot ring[2];
    __shared__ __attribute__((aligned(16))) CellBatch cells[2];      // cs, ssim

    const int lane = threadIdx.x;
    const float gf[6] = {args.gf[0], args.gf[1], args.gf[2], args.gf[3], args.gf[4], args.gf[5]};

    // the strip: image-major, then strip row, then strip column, each XCD walking a contiguous share of that list
    const uint32_t per_img = args.strips_x * args.strips_y;
    const uint32_t id = xcd_order(blockIdx.x, per_img * args.count, args.xcds);
    const uint32_t img = id / per_img, lin = id - img * per_img;
    const uint32_t sy = lin / args.strips_x, sx = lin - sy * args.strips_x;
    PairHDesc pd;
    {
        const gptr_desch gd = (gptr_desch)args.descs + img;
        pd.a = (const uint16_t*)uniform64((int64_t)gd->a); pd.a_step = uniform64(gd->a_step); pd.a_stride = uniform64(gd->a_stride);
        pd.b = (const uint16_t*)uniform64((int64_t)gd->b); pd.b_step = uniform64(gd->b_step); pd.b_stride = uniform64(gd->b_stride);
    }
    const int W = (int)args.width, H = (int)args.height;
    const int x0 = (int)(sx * Slot::STRIP_W), y0 = (int)(sy * args.strip_rows);
    const int y_end = y0 + (int)args.strip_rows < H ? y0 + (int)args.strip_rows : H;

    // the strip column's centre (see the top of the file), per image
    f2 cen;
    {
        const int64_t cx = x0 + 64 < W ? x0 + 64 : W - 1, cy = (H - 1) / 2;
        const float sa = widen<TYPE>((uint16_t)__builtin_amdgcn_readfirstlane((uint32_t)((gptr_cu16)pd.a)[cx * pd.a_step + cy * pd.a_stride]));
        const float sb = widen<TYPE>((uint16_t)__builtin_amdgcn_readfirstlane((uint32_t)((gptr_cu16)pd.b)[cx * pd.b_step + cy * pd.b_stride]));
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
        offA[t] = (Off)((int64_t)(xg - refA) * pd.a_step * 2);
        offB[t] = (Off)((int64_t)(xg - refB) * pd.b_step * 2);
    }

    float va[NLOAD], vb[NLOAD];
    auto fetch_to = [&](int r, float (&oa)[NLOAD], float (&ob)[NLOAD]) {     // row r (clamped) -> registers
        const int ry = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
        const gptr_u8 ra = baseA + (int64_t)ry * pd.a_stride * 2;
        const gptr_u8 rb = baseB + (int64_t)ry * pd.b_stride * 2;
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            if constexpr (!WIDE) asm volatile("" : "+v"(offA[t]), "+v"(offB[t]));   // keeps the zero-extension foldable into the load
            oa[t] = widen<TYPE>(*(gptr_cu16)(ra + offA[t]));
            ob[t] = widen<TYPE>(*(gptr_cu16)(rb + offB[t]));
        }
    };
    auto fetch = [&](int r) { fetch_to(r, va, vb); };
    auto stage_from = [&](Slot& s, const float (&ia)[NLOAD], const float (&ib)[NLOAD]) {   // registers -> the two planes of a slot
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            const f2 ab = f2{ia[t], ib[t]} - cen;         // (a', b')
            const float a = ab.x, b = ab.y;
            const int p = sp[t];
            s.ab[p] = ab;
            s.q[p] = f2{__builtin_fmaf(b, b, a * a), a * b};
        }
    };
    auto stage = [&](Slot& s) { stage_from(s, va, vb); };

    f2 accAB[2][11], accQ[2][11];
#pragma unroll
    for (int k = 0; k < 11; ++k) accAB[0][k] = accAB[1][k] = accQ[0][k] = accQ[1][k] = f2{0.0f, 0.0f};
    double colsum[2] = {0.0, 0.0}, colcs[2] = {0.0, 0.0};

    const int r_begin = y0 - 5;
    {
        float a0[NLOAD], b0[NLOAD], a1[NLOAD], b1[NLOAD];
        fetch_to(r_begin, a0, b0);
        fetch_to(r_begin + 1, a1, b1);
        fetch(r_begin + 2);
        stage_from(ring[0], a0, b0);
        stage_from(ring[1], a1, b1);
    }
    wave_sync();

    const bool col_ok[2] = {x0 + 2 * lane < W, x0 + 2 * lane + 1 < W};

    f2 wab[12], wq[12];
    const int e = 2 * lane + PAD - 5;                     // even: the 16-byte reads are aligned
    auto load_ab = [&](const Slot& s) {
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const f4 v = *reinterpret_cast<const f4*>(&s.ab[e + 2 * t]);
            wab[2 * t] = v.xy; wab[2 * t + 1] = v.zw;
        }
    };
    // The (a', b') row pass of the row about to be blurred: computed at the end of the previous iteration and carried over.
    f2 hab[2];
    auto fold_ab = [&]() {
        f2 s[2][6];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int m = 5 + c;
            s[c][0] = wab[m];
#pragma unroll
            for (int i = 1; i <= 5; ++i) s[c][i] = wab[m + i] + wab[m - i];
        }
        rows_pair(hab[0], hab[1], s[0], s[1], gf);
    };
    load_ab(ring[0]);
    fold_ab();

    auto row = [&](const int r, auto slot, auto phase_tag, auto kmin_tag) {
        constexpr int cur = decltype(slot)::value;
        constexpr int phase = decltype(phase_tag)::value;
        constexpr int KMIN = decltype(kmin_tag)::value;
        const Slot& s = ring[cur];
        __builtin_amdgcn_s_setprio(2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const f4 u = *reinterpret_cast<const f4*>(&s.q[e + 2 * t]);
            wq[2 * t] = u.xy;  wq[2 * t + 1] = u.zw;
        }
        __builtin_amdgcn_sched_barrier(0);
        columns_pair<KMIN>(accAB[0], accAB[1], hab[0], hab[1], gf);
        __builtin_amdgcn_sched_barrier(0);
        {
            const f2 s0[6] = {wq[5], wq[6] + wq[4], wq[7] + wq[3], wq[8] + wq[2], wq[9] + wq[1], wq[10] + wq[0]};
            const f2 s1[6] = {wq[6], wq[7] + wq[5], wq[8] + wq[4], wq[9] + wq[3], wq[10] + wq[2], wq[11] + wq[1]};
            blur_pair<KMIN>(accQ[0], accQ[1], s0, s1, gf);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ring entry 0 is now the finished output row r - 5
        if constexpr (phase != ROW_WARMUP) {
            f2 cs;
            const f2 v = msssim_px2(accAB[0][0], accAB[1][0], accQ[0][0], accQ[1][0], cen, args.c1, args.c2, cs);
            colsum[0] += (double)v.x;
            colsum[1] += (double)v.y;
            colcs[0] += (double)cs.x;
            colcs[1] += (double)cs.y;
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
    // the ten warm-up rows in pairs (the two LDS slots); warm-up row i only feeds ring entries k >= 10 - i
    row(r, S0(), Warm(), std::integral_constant<int, 9>());     row(r + 1, S1(), Warm(), std::integral_constant<int, 9>());
    row(r + 2, S0(), Warm(), std::integral_constant<int, 7>()); row(r + 3, S1(), Warm(), std::integral_constant<int, 7>());
    row(r + 4, S0(), Warm(), std::integral_constant<int, 5>()); row(r + 5, S1(), Warm(), std::integral_constant<int, 5>());
    r += 6;
#pragma unroll 1
    for (int i = 0; i < 2; ++i, r += 2) {
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
        cells[0].leaf[parked][lane] = (col_ok[0] ? colcs[0] : 0.0) + (col_ok[1] ? colcs[1] : 0.0);
        cells[1].leaf[parked][lane] = (col_ok[0] ? colsum[0] : 0.0) + (col_ok[1] ? colsum[1] : 0.0);
        colsum[0] = colsum[1] = colcs[0] = colcs[1] = 0.0;
        if (++parked == CELL_BATCH) {
            wave_sync();
            cell_batch_flush(args, img, sx, cells[0], cell_y, parked, 0);
            cell_batch_flush(args, img, sx, cells[1], cell_y, parked, 1);
            wave_sync();
            cell_y += parked;
            parked = 0;
        }
    }
    if (parked) {
        wave_sync();
        cell_batch_flush(args, img, sx, cells[0], cell_y, parked, 0);
        cell_batch_flush(args, img, sx, cells[1], cell_y, parked, 1);
    }
}
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
uint32_t cell_rows_of(uint32_t height) { return height >= 2048 ? 32u : 8u; }

// ---- the gradient ------------------------------------------------------------------------------------------------------------
// msssimh_grad_kernel: msssimf_grad_kernel at scale 0 (its steps are repeated in the comments below).  The samples come in through
// widen<TYPE> (step 1, the centre, the re-read of step 6); the float32 result, the coarser scale's gradient included, leaves through
// narrow<TYPE> as one 2-byte store.  One 256-lane workgroup = one 32 x 32 tile of gradient pixels at an absolute position; every
// gradient pixel is written by one work-item in a fixed order: no atomics, the same bits in any batch.
enum { GT = kSFTile, GIN = GT + 20, GST = GT + 10 };

struct KGHArgs {
    const PairHDesc* descs;       // scale 0: the caller's planes
    const GradHDesc* grads;       // scale 0: the caller's gradient planes, in the samples' encoding
    const GradFDesc* up;          // scale 1's gradient planes (dense float32); unused by the LAST form
    const float*     coef;        // k_s of pair i at coef[i * coef_stride]
    uint32_t coef_stride;
    uint32_t width, height, tiles_x, tiles_y;
    float    c1, c2, range;
    float    gf[6], tail[6], total;
};

// w(q, j) above for an axis of n pixels.
__device__ __forceinline__ float adjoint_weight(int q, int n, int j, const float (&g)[6], const float (&tail)[6], float total)
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
// TYPE: kSHTypeF16 or kSHTypeBF16, the encoding of the samples and of the gradient.
// LAST: scales == 1, scale 0 is the coarsest (the ssim form, no coarser gradient to add); otherwise the cs form, whose epilogue adds the adjoint of
// the clamped 2 x 2 box filter applied to the next coarser scale's gradient: 0.25 c g_{s+1}(x >> 1, y >> 1).
template <int TYPE, int WHICH, bool LAST>
__global__ __launch_bounds__(256)
void msssimh_grad_kernel(const KGHArgs args)
{
    constexpr int NP = WHICH == 3 ? 4 : 3;                       // partial planes: d_mu (of A, or of the one wanted), d_aa, d_ab, d_mu of B
    constexpr int XN = 2 * GIN * GIN > NP * GST * GST ? 2 * GIN * GIN : NP * GST * GST;
    constexpr int YN = 4 * GIN * GST;                            // >= NP * GST * GT
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
    const PairHDesc pd = args.descs[img];
    const GradHDesc gd = args.grads[img];
    const gptr_cu16 pa = (gptr_cu16)pd.a, pb = (gptr_cu16)pd.b;
    const float gf[6] = {args.gf[0], args.gf[1], args.gf[2], args.gf[3], args.gf[4], args.gf[5]};
    const float tail[6] = {args.tail[0], args.tail[1], args.tail[2], args.tail[3], args.tail[4], args.tail[5]};
    const float k = ((gptr_cf32)args.coef)[(size_t)img * args.coef_stride];

    // The coarser scale's gradient at this pixel, through the adjoint of the clamped box filter: the last column (row) of an odd
    // width (height) was read twice by the clamp.  0.25 c is a power of two: the product is exact.
    auto upstream = [&](const float* gup, int64_t ustep, int64_t ustride, int qx, int qy) -> float {
        if constexpr (LAST) return 0.0f;
        const float cx = ((W & 1) && qx == W - 1) ? 2.0f : 1.0f, cy = ((H & 1) && qy == H - 1) ? 2.0f : 1.0f;
        return (0.25f * (cx * cy)) * ((gptr_cf32)gup)[(int64_t)(qx >> 1) * ustep + (int64_t)(qy >> 1) * ustride];
    };
    GradFDesc ud = {nullptr, 0, 0, nullptr, 0, 0};
    if constexpr (!LAST) ud = args.up[img];

    // k == 0 (a zero weight, gOut == 0, or MS == 0): this scale contributes +0 everywhere, whatever the samples are.
    if (k == 0.0f) {
        for (int idx = tid; idx < GT * GT; idx += 256) {
            const int y = idx / GT, x = idx - y * GT;
            const int qx = x0 + x, qy = y0 + y;
            if (qx >= W || qy >= H) continue;
            if constexpr (WHICH != 2)
                ((gptr_u16)gd.ga)[(int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride] = narrow<TYPE>(0.0f + upstream(ud.ga, ud.ga_step, ud.ga_stride, qx, qy));
            if constexpr (WHICH != 1)
                ((gptr_u16)gd.gb)[(int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride] = narrow<TYPE>(0.0f + upstream(ud.gb, ud.gb_step, ud.gb_stride, qx, qy));
        }
        return;
    }

    f2 cen;                                                      // the strip column's centre (top of the file)
    {
        const int xs = x0 & ~(kSFStripW - 1);
        const int64_t cx = xs + 64 < W ? xs + 64 : W - 1, cy = (H - 1) / 2;
        const float sa = widen<TYPE>(pa[cx * pd.a_step + cy * pd.a_stride]), sb = widen<TYPE>(pb[cx * pd.b_step + cy * pd.b_stride]);
        cen = f2{__builtin_fabsf(sa) <= args.range ? sa : 0.0f, __builtin_fabsf(sb) <= args.range ? sb : 0.0f};
    }

    // 1. samples
    for (int idx = tid; idx < GIN * GIN; idx += 256) {
        const int j = idx / GIN, i = idx - j * GIN;
        int x = x0 - 10 + i, y = y0 - 10 + j;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        const f2 v = {widen<TYPE>(pa[(int64_t)x * pd.a_step + (int64_t)y * pd.a_stride]), widen<TYPE>(pb[(int64_t)x * pd.b_step + (int64_t)y * pd.b_stride])};
        in[idx] = v - cen;
    }
    __syncthreads();

    // 2. row pass: H*[j][u] is the blur along x at image column x0 - 5 + u of source row y0 - 10 + j
    for (int idx = tid; idx < GIN * GST; idx += 256) {
        const int j = idx / GST, u = idx - j * GST;
        const f2* row = in + j * GIN + u;
        f2 ab[11], q[11];
#pragma unroll
        for (int t = 0; t < 11; ++t) {
            ab[t] = row[t];
            q[t] = f2{__builtin_fmaf(ab[t].y, ab[t].y, ab[t].x * ab[t].x), ab[t].x * ab[t].y};
        }
        const f2 sab[6] = {ab[5], ab[6] + ab[4], ab[7] + ab[3], ab[8] + ab[2], ab[9] + ab[1], ab[10] + ab[0]};
        const f2 sq[6] = {q[5], q[6] + q[4], q[7] + q[3], q[8] + q[2], q[9] + q[1], q[10] + q[0]};
        f2 hab, hq;
        rows_pair(hab, hq, sab, sq, gf);
        Hab[idx] = hab;
        Hq[idx] = hq;
    }
    __syncthreads();

    // 3. column pass, SSIM terms, weighted partials
    for (int idx = tid; idx < GST * GST; idx += 256) {
        const int v = idx / GST, u = idx - v * GST;
        const int px = x0 - 5 + u, py = y0 - 5 + v;
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (px >= 0 && px < W && py >= 0 && py < H) {
            const f2* cab = Hab + v * GST + u;
            const f2* cq = Hq + v * GST + u;
            f2 m = cab[0] * f2{gf[5], gf[5]}, e = cq[0] * f2{gf[5], gf[5]};
#pragma unroll
            for (int t = 1; t < 11; ++t) {
                const float w = gf[t < 5 ? 5 - t : t - 5];
                m = fma_(cab[t * GST], f2{w, w}, m);
                e = fma_(cq[t * GST], f2{w, w}, e);
            }
            // the forward kernel's terms (ssim_px2), then the derivative
            const float pc = opaque(m.x * m.y), tc = opaque(opaque(m.x * m.x) + opaque(m.y * m.y));
            const float sS = opaque(e.x - tc), sAB = opaque(e.y - pc);
            const float uA = m.x + cen.x, uB = m.y + cen.y;
            const float muAB = opaque(uA * uB), tm = opaque(opaque(uA * uA) + opaque(uB * uB));
            const float A2 = __builtin_fmaf(2.0f, sAB, args.c2), B2 = sS + args.c2;
            const float r2 = __builtin_amdgcn_rcpf(B2);
            float dab, daa, dmA, dmB;
            if constexpr (LAST) {
                const float A1 = __builtin_fmaf(2.0f, muAB, args.c1), B1 = tm + args.c1;
                const float r1 = __builtin_amdgcn_rcpf(B1);
                const float r12 = opaque(r1 * r2);
                const float ssim = opaque(opaque(A1 * A2) * r12);
                dab = opaque(opaque(2.0f * A1) * r12);
                daa = -opaque(ssim * r2);
                const float f1 = opaque(A2 * r12), f2_ = opaque(ssim * r1);
                dmA = opaque(opaque(opaque(opaque(2.0f * uB) * f1) - opaque(opaque(2.0f * uA) * f2_)) - opaque(opaque(2.0f * m.x) * daa)) - opaque(m.y * dab);
                dmB = opaque(opaque(opaque(opaque(2.0f * uA) * f1) - opaque(opaque(2.0f * uB) * f2_)) - opaque(opaque(2.0f * m.y) * daa)) - opaque(m.x * dab);
            } else {
                // cs = A2 / B2 alone: d_ab = 2 / B2, d_aa = -cs / B2, and d_mu in the centred variables has no luminance part
                const float cs = opaque(A2 * r2);
                dab = opaque(2.0f * r2);
                daa = -opaque(cs * r2);
                dmA = -opaque(opaque(2.0f * m.x) * daa) - opaque(m.y * dab);
                dmB = -opaque(opaque(2.0f * m.y) * daa) - opaque(m.x * dab);
            }
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
        float wx[11];
#pragma unroll
        for (int j = -5; j <= 5; ++j) wx[j + 5] = adjoint_weight(qx, W, j, gf, tail, args.total);
        for (int idx = tid; idx < GST * GT; idx += 256) {
            const int v = idx / GT;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
                const float* src = P + pl * GST * GST + v * GST + x;
                float acc = src[0] * wx[0];
#pragma unroll
                for (int t = 1; t < 11; ++t) acc = __builtin_fmaf(src[t], wx[t], acc);
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
        float wy[11];
#pragma unroll
        for (int j = -5; j <= 5; ++j) wy[j + 5] = adjoint_weight(qy, H, j, gf, tail, args.total);
        float r[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            const float* src = Q + pl * GST * GT + y * GT + x;
            float acc = src[0] * wy[0];
#pragma unroll
            for (int t = 1; t < 11; ++t) acc = __builtin_fmaf(src[t * GT], wy[t], acc);
            r[pl] = acc;
        }
        const float a = widen<TYPE>(pa[(int64_t)qx * pd.a_step + (int64_t)qy * pd.a_stride]) - cen.x;
        const float b = widen<TYPE>(pb[(int64_t)qx * pd.b_step + (int64_t)qy * pd.b_stride]) - cen.y;
        if constexpr (WHICH != 2) {
            const float g = opaque(r[0] + opaque(opaque(2.0f * a) * r[1])) + opaque(b * r[2]);
            ((gptr_u16)gd.ga)[(int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride] = narrow<TYPE>(LAST ? g : opaque(g) + upstream(ud.ga, ud.ga_step, ud.ga_stride, qx, qy));
        }
        if constexpr (WHICH != 1) {
            const float g = opaque(r[WHICH == 3 ? 3 : 0] + opaque(opaque(2.0f * b) * r[1])) + opaque(a * r[2]);
            ((gptr_u16)gd.gb)[(int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride] = narrow<TYPE>(LAST ? g : opaque(g) + upstream(ud.gb, ud.gb_step, ud.gb_stride, qx, qy));
        }
    }
}
// the true 1-D Gaussian, sigma 1.5, normalised over the 11 taps, rounded to float: the engine's taps, centre first
void gaussian_taps(float (&gf)[6])
{
    double g[6], norm = 0.0;
    for (int i = 0; i <= 5; ++i) {
        g[i] = exp(-(double)(i * i) / (2.0 * 1.5 * 1.5));
        norm += (i == 0) ? g[i] : 2.0 * g[i];
    }
    for (int i = 0; i <= 5; ++i) gf[i] = (float)(g[i] / norm);
}

bool valid_type(int type) { return type == kSHTypeF16 || type == kSHTypeBF16; }

// The pyramid step from the caller's planes into row 1 of descs_dev.
template <int TYPE>
void launch_down(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height, hipStream_t stream)
{
    const uint32_t dw = msf_dim(width, 1), dh = msf_dim(height, 1);
    const uint32_t per = (uint32_t)(((uint64_t)dw * dh + 255) / 256);
    hipLaunchKernelGGL((msssimh_down_kernel<TYPE>), dim3(per * count), dim3(256), 0, stream, descs0_dev, descs_dev + (size_t)count, width, height, dw, dh, per);
}

template <int TYPE>
void launch_strip(const KMHArgs& ka, dim3 grid, dim3 block, bool wide, hipStream_t stream)
{
    if (wide) hipLaunchKernelGGL((msssimh_strip_kernel<TYPE, true>), grid, block, 0, stream, ka);
    else      hipLaunchKernelGGL((msssimh_strip_kernel<TYPE, false>), grid, block, 0, stream, ka);
}

template <int TYPE>
void launch_grad(const KGHArgs& ka, dim3 grid, dim3 block, int which, bool last, hipStream_t stream)
{
    if (last) {
        if (which == 1)      hipLaunchKernelGGL((msssimh_grad_kernel<TYPE, 1, true>), grid, block, 0, stream, ka);
        else if (which == 2) hipLaunchKernelGGL((msssimh_grad_kernel<TYPE, 2, true>), grid, block, 0, stream, ka);
        else                 hipLaunchKernelGGL((msssimh_grad_kernel<TYPE, 3, true>), grid, block, 0, stream, ka);
    } else {
        if (which == 1)      hipLaunchKernelGGL((msssimh_grad_kernel<TYPE, 1, false>), grid, block, 0, stream, ka);
        else if (which == 2) hipLaunchKernelGGL((msssimh_grad_kernel<TYPE, 2, false>), grid, block, 0, stream, ka);
        else                 hipLaunchKernelGGL((msssimh_grad_kernel<TYPE, 3, false>), grid, block, 0, stream, ka);
    }
}

} // namespace

hipError_t launch_msssimh(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, uint32_t count, uint32_t width, uint32_t height,
                          uint32_t scales, int type, bool wide, float data_range, const double* weights, int cu_count, int xcd_count,
                          double* partials, double* means, double* values, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_type(type) || !(data_range > 0.0f) || !std::isfinite(data_range) || scales < 1 || scales > kMSFMaxScales ||
        count > msssimf_max_count(width, height))
        return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1) {
        if (type == kSHTypeBF16) launch_down<kSHTypeBF16>(descs0_dev, descs_dev, count, width, height, stream);
        else                     launch_down<kSHTypeF16>(descs0_dev, descs_dev, count, width, height, stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // scale 0's strips and cells, as launch_msssimf_from lays them out: its partials come first
    KMHArgs ka;
    ka.descs = descs0_dev;
    ka.width = width; ka.height = height;
    ka.strip_rows = strip_rows_of(width, height, count, cu_count);
    ka.strips_x = (width + kSFStripW - 1) / kSFStripW;
    ka.strips_y = (height + ka.strip_rows - 1) / ka.strip_rows;
    const uint32_t cr = cell_rows_of(height);
    ka.cells_x = (width + 63) / 64; ka.cells_y = (height + cr - 1) / cr;
    ka.cell_shift = cr == 32 ? 5 : 3;
    ka.count = count;
    ka.xcds = xcd_count >= 1 ? (uint32_t)xcd_count : 8u;
    ka.partials = partials;
    ka.range = data_range;
    ssimf_constants(data_range, ka.c1, ka.c2);
    gaussian_taps(ka.gf);
    const dim3 grid((uint32_t)((uint64_t)ka.strips_x * ka.strips_y * count)), block(64);
    if (type == kSHTypeBF16) launch_strip<kSHTypeBF16>(ka, grid, block, wide, stream);
    else                     launch_strip<kSHTypeF16>(ka, grid, block, wide, stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_msssimf_from(1, descs_dev, count, width, height, scales, false, data_range, weights, cu_count, xcd_count, partials, means,
                               values, stream);
}

hipError_t launch_msssimh_grad(const PairHDesc* descs0_dev, const PairFDesc* descs_dev, const GradHDesc* grads0_dev, const GradFDesc* grads_dev,
                               uint32_t count, uint32_t width, uint32_t height, uint32_t scales, int type, float data_range,
                               const double* weights, const double* means, const float* g_out, float* coef, int which, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!valid_type(type) || !(data_range > 0.0f) || !std::isfinite(data_range) || scales < 1 || scales > kMSFMaxScales || which < 1 ||
        which > 3 || count > msssimf_max_count(width, height))
        return hipErrorInvalidValue;
    hipError_t e;
    if (scales > 1) {
        if (type == kSHTypeBF16) launch_down<kSHTypeBF16>(descs0_dev, descs_dev, count, width, height, stream);
        else                     launch_down<kSHTypeF16>(descs0_dev, descs_dev, count, width, height, stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // the coefficients of every scale, the rest of the pyramid, the float32 gradients from the coarsest scale down to scale 1
    if ((e = launch_msssimf_grad_from(1, descs_dev, grads_dev, count, width, height, scales, data_range, weights, means, g_out, coef, which,
                                      stream)) != hipSuccess)
        return e;
    KGHArgs ka;
    ka.range = data_range;
    ssimf_constants(data_range, ka.c1, ka.c2);
    gaussian_taps(ka.gf);
    // tail[d] = g_d + ... + g_5 and the sum of all eleven taps: sums of the float taps in double, rounded once
    double t = 0.0;
    for (int i = 5; i >= 0; --i) { t += (double)ka.gf[i]; ka.tail[i] = (float)t; }
    ka.total = (float)(2.0 * t - (double)ka.gf[0]);
    ka.coef_stride = scales;
    const bool last = scales == 1;
    ka.descs = descs0_dev;
    ka.grads = grads0_dev;
    ka.up = last ? nullptr : grads_dev + (size_t)count;
    ka.coef = coef;
    ka.width = width; ka.height = height;
    ka.tiles_x = (width + kSFTile - 1) / kSFTile; ka.tiles_y = (height + kSFTile - 1) / kSFTile;
    const dim3 grid((uint32_t)((uint64_t)ka.tiles_x * ka.tiles_y * count)), block(256);
    if (type == kSHTypeBF16) launch_grad<kSHTypeBF16>(ka, grid, block, which, last, stream);
    else                     launch_grad<kSHTypeF16>(ka, grid, block, which, last, stream);
    return hipGetLastError();
}

} // namespace ssim_hip
