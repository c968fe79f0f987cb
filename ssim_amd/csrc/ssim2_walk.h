// ssim2_walk.h -- the strip walk of SSIM on 2-D float-family samples and the gradient tile, written once for the kernel files of the
// family (ssimf / ssimh / ssimk / ssimhk / ssimw / msssimf / msssimh / msssimk / msssimhk _kernels.hip).  Not installed, and included by those nine files only: each of
// them keeps its __global__ kernels -- their names, template parameters and launch bounds, which its tests count and budget -- as
// one-line calls of strip_body, grad_body and reduce_body, and its launch_* functions.  Everything here has internal linkage, so an
// instantiation and its LDS belong to the one kernel of the including file that calls it.  The definition the kernels implement is in
// include/rmgr/ssim-hip.h; tests/ssimf_model.py and tests/ssimk_model.py restate it in float64 and restate the arithmetic below in fp32.
// The nine files are built with the same flags (-ffp-contract=off).
//
// The bodies are templates on these things, and on nothing else:
//  * Sample: how a sample gets into a register and how a gradient pixel leaves one.  SampleF32 is a float load / store.  SampleH<TYPE>
//    is a 2-byte load and an exact widening (widen<TYPE>: bfloat16 is the upper half of a float32, a shift; float16 goes through the
//    hardware convert, which keeps subnormals and maps NaN and Inf to NaN and Inf); byte offsets scale by 2; narrow<TYPE> rounds the
//    float32 value once, to nearest-even, and a 2-byte store writes it (float16: the hardware convert, subnormals kept, overflow to Inf;
//    bfloat16: integer rounding of the bit pattern, NaN kept NaN).  From stage_from on (forward) and from the `in` plane on (gradient)
//    there is one instruction stream, which is what gives value, map, sums and the float32 gradient of the 16-bit entries the bits of
//    the float32 ones on the widened planes.  Loads and stores are the plain per-sample form: a base pointer is only aligned to its
//    sample, and the forward kernel is VALU-bound.
//  * R, the window's radius, 1 .. 5 (3 .. 11 taps): register rings of 2R + 1 entries, 2R warm-up rows from source row y0 - R on, the
//    finished row is r - R; a lane reads its 2R + 2 window pixels (columns x - R .. x + R + 1 of its first column x) as R + 1 aligned
//    16-byte LDS reads.  A window never reads beyond its radius: a NaN sample reaches the (2R + 1)^2 map pixels around it and no others.
//    Shape<R> holds the slot layout and the warm-up schedule, which are NOT one rule: radius 5 keeps the layout and schedule it was
//    tuned with, radius 1 .. 4 theirs.  They give the same bits, but not the same code, LDS addresses or speed.
//  * FORM (strip_body).  kFormSsim: SSIM, one fp64 sum per cell, an optional map.  kFormMulti: a scale of MS-SSIM -- no map, and TWO
//    fp64 sums per cell, cs = A2 / B2 and ssim = A1 A2 / (B1 B2), flushed as [cell]{cs, ssim}; the ssim one has the bits of kFormSsim.
//  * MAP, WIDE (strip_body).  MAP: 0 no map; 1 any ssimStep (one 4-byte store per column); 2 ssimStep == 1 and an even width (one
//    8-byte store per lane; radius 5 only).  WIDE: 64-bit lane offsets for the samples and the map (pairs that fail fitsf_narrow() /
//    fitsh_narrow()); the map then goes out as plain guarded stores.
//  * KFORM (grad_body, defaulted: ssimf / ssimh do not name it): where the weight k of a pixel's partial derivatives comes from.
//    kKUniform: k = float(double(gOut) / (double(W) double(H))) for the whole pair.  kKPerPixel: k(p) = gMap(p), read per pixel through
//    the pair's GradOutFDesc.  kKEither: a branch on a kernel argument between the two (g_out != NULL: uniform).  kKCoef (the multi-scale
//    form): k = g_out[pair * g_out_stride] as it stands, the k_s of that pair at the launch's scale, computed on the device.  The
//    product k d is the same instruction in every form, a plain fp32 product (k = 0 does not hide a NaN statistic), so a constant
//    plane gMap gives the uniform form's bits.
//  * MS (grad_body, defaulted likewise).  kMsNone.  kMsLast: the coarsest scale of MS-SSIM (the ssim form, no coarser gradient to
//    add).  kMsUp: a finer scale -- the cs form, whose epilogue adds the adjoint of the clamped 2 x 2 box filter applied to the next
//    coarser scale's gradient, 0.25 c g_{s+1}(x >> 1, y >> 1), before the single store.  In both multi-scale forms a pair whose k is 0
//    (a zero weight, gOut == 0, or MS == 0) gets +0 (plus the coarser gradient) in every pixel, whatever its samples are.
//
// strip_body<Sample, R, FORM, MAP, WIDE>: one 64-lane wavefront = one workgroup = one vertical strip of 128 output columns (two per lane) x
//    strip_rows rows.  Per source row the wave loads the row's float samples of A and B (edge-clamped, any step / stride) one
//    row ahead into registers, centres them (below), writes the (a', b') and (a'^2 + b'^2, a'b') planes of the row into a 2-slot
//    LDS ring, reads each lane's 12-pixel window back with 16-byte reads, runs the horizontal pass on the folded sums and
//    scatters the result into 11-deep register rings (the vertical pass); the ring's oldest entry is a finished output row:
//    SSIM formula, fp64 column sums, optional map store.  Intermediates never touch HBM: 8 B of samples per pixel (+4 B with a
//    map).  Plain fp32 VALU, no MFMA.  (The counts are radius 5's.)
// reduce_body: each image's cell partials summed in a fixed order.
// grad_body<Sample, R, WHICH, KFORM, MS>: the gradient, one fused launch that recomputes the statistics (DESIGN.md section 12 has the
//    reasons).  Its own comment is above it.
//
// Centring.  Both kernels blur a' = a - cA, b' = b - cB.  The centre of the 128 columns from x0 = 128 k on is A's and B's sample
// at (min(x0 + 64, W - 1), (H - 1) / 2), as in ssim16_kernels.hip, when its magnitude is at most dataRange, else 0 (so a NaN, an
// Inf or a far outlier at that one position cannot spoil a whole strip column: it then behaves like any other sample).  The
// position is fixed by the image, so every strip height, tile, batch, split and entry point sees the same centre.  Unlike
// integer samples the subtraction rounds: a' is a - c to half an ulp of a', an input perturbation below the samples' own
// resolution wherever |a - c| <= |a|, and it leaves numbers near 0 in smooth areas, where the cancellation in E[a'^2] - mu_a'^2
// would otherwise cost the most.  The emulation in tests/ssimf_model.py makes the same subtraction.  In MS-SSIM the rule holds at
// every scale ON THAT SCALE'S PLANES; the pyramid is a fixed function of the image.
//
// Per-pixel values and cells.  Every output pixel receives the 11 row-pass values of its source rows in source-row order, first
// one multiplied into zero, whatever row the strip starts at; a cell (64 columns x cell_rows rows at an absolute position) is
// the per-column sum in row order, the column pairs, then a fixed tree.  The sums are therefore bit-identical for any strip
// height, batch or split.  Centres, cells, tiles and summation orders are position-based: none depends on the radius or on the size
// of a sample.
#ifndef SSIM_AMD_SSIM2_WALK_H
#define SSIM_AMD_SSIM2_WALK_H

#include "msssimh_kernels.h"    // PairFDesc, GradFDesc, GeometryF, PairHDesc, GradHDesc, kSHTypeF16 / BF16, ssimf_max_count, ssimf_constants
#include "ssimk_kernels.h"      // GradOutFDesc, window_taps, window_tails, kSKMaxRadius
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace ssim_hip {
namespace {

typedef float  f2 __attribute__((ext_vector_type(2)));
typedef float  f4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

typedef const uint8_t __attribute__((address_space(1)))*  gptr_u8;
typedef const float __attribute__((address_space(1)))*    gptr_cf32;
typedef float __attribute__((address_space(1)))*          gptr_f32;
typedef double __attribute__((address_space(1)))*         gptr_f64;
typedef const uint16_t __attribute__((address_space(1)))* gptr_cu16;
typedef uint16_t __attribute__((address_space(1)))*       gptr_u16;

__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float opaque(float v) { asm("" : "+v"(v)); return v; }

__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

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

// A stored sample -> float32, exactly.
template <int TYPE>
__device__ __forceinline__ float widen(uint16_t s)
{
    if constexpr (TYPE == kSHTypeBF16) return __builtin_bit_cast(float, (uint32_t)s << 16);
    else                               return (float)__builtin_bit_cast(_Float16, s);
}
// float32 -> the samples' encoding, one rounding to nearest-even.
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

// The sample policies: the descriptors of a pair, a sample's size, and a sample in and out of a register -- element `at` of a plane
// (the gradient tile), a byte base plus a lane offset (the strip's staging), and the wave-uniform form of the centre sample.
struct SampleF32 {
    typedef float     T;
    typedef PairFDesc Pair;
    typedef GradFDesc Grad;
    enum { BYTES = 4 };
    static __device__ __forceinline__ float load(const float* p, int64_t at) { return ((gptr_cf32)p)[at]; }
    static __device__ __forceinline__ void store(float* p, int64_t at, float v) { ((gptr_f32)p)[at] = v; }
    template <class Off> static __device__ __forceinline__ float load_bytes(gptr_u8 base, Off off) { return *(gptr_cf32)(base + off); }
    static __device__ __forceinline__ float load_uniform(const float* p, int64_t at)
    {
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, ((gptr_cf32)p)[at])));
    }
};
template <int TYPE> struct SampleH {
    typedef uint16_t  T;
    typedef PairHDesc Pair;
    typedef GradHDesc Grad;
    enum { BYTES = 2 };
    static __device__ __forceinline__ float load(const uint16_t* p, int64_t at) { return widen<TYPE>(((gptr_cu16)p)[at]); }
    static __device__ __forceinline__ void store(uint16_t* p, int64_t at, float v) { ((gptr_u16)p)[at] = narrow<TYPE>(v); }
    template <class Off> static __device__ __forceinline__ float load_bytes(gptr_u8 base, Off off) { return widen<TYPE>(*(gptr_cu16)(base + off)); }
    static __device__ __forceinline__ float load_uniform(const uint16_t* p, int64_t at)
    {
        return widen<TYPE>((uint16_t)__builtin_amdgcn_readfirstlane((uint32_t)((gptr_cu16)p)[at]));
    }
};

enum { MAXR = kSKMaxRadius };
enum { kFormSsim = 0, kFormMulti = 1 };
enum { kKUniform = 0, kKPerPixel = 1, kKEither = 2, kKCoef = 3 };
enum { kMsNone = 0, kMsLast = 1, kMsUp = 2 };

// What the radius decides.  N ring entries, NWIN window pixels of a lane's two columns.  The LDS slot is one source row of ROW_PX
// pixels starting PAD columns left of the strip; a lane's window starts on the even slot pixel 2 lane + PAD - R.
//   R = 5: 144 pixels starting seven columns left of the strip; the ten warm-up rows run as three pairs that skip the ring entries
//   standing for rows above the strip (warm-up row i only feeds ring entries k >= 2R - i), then a loop of two pairs.
//   R = 1 .. 4: 128 + 2R pixels starting R columns left (the last lane's window ends on the slot's last pixel); the first pair skips,
//   the later pairs run as one loop over the full ring (what they write below 2R - i leaves the ring before the first finished row
//   is read).
template <int R> struct Shape {
    static_assert(R >= 1 && R <= MAXR, "radius");
    static constexpr int N = 2 * R + 1, NWIN = 2 * R + 2;
    static constexpr int STRIP_W = kSFStripW, PAD = R == 5 ? 7 : R, ROW_PX = R == 5 ? 144 : STRIP_W + 2 * R;
    static constexpr int WARM_PAIRS = R == 5 ? 3 : 1;            // warm-up pairs with a KMIN of their own, KMIN = 2R - 1, 2R - 3, ...
    static constexpr int NLOAD = 3;                              // samples each lane stages per row and image (192 >= ROW_PX)
    static_assert((PAD - R) % 2 == 0 && 126 + PAD - R + NWIN <= ROW_PX && ROW_PX <= 64 * NLOAD, "slot");
};
template <int R> struct Slot {
    f2 ab[Shape<R>::ROW_PX];   // (a', b')
    f2 q[Shape<R>::ROW_PX];    // (a'^2 + b'^2, a'b')
};

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

// SSIM of the lane's two columns from the centred moments: m0, m1 = (mu_a', mu_b') of each column, e0, e1 = (E[a'^2 + b'^2],
// E[a'b']); cen = (cA, cB).  sigma_a^2 + sigma_b^2 = E[a'^2 + b'^2] - (mu_a'^2 + mu_b'^2), sigma_ab = E[a'b'] - mu_a' mu_b',
// mu = mu' + centre.  The quotient is n * rcp(d) (1 ulp, as MODE_SEPARABLE).  kFormMulti: plus cs = A2 * rcp(B2).
template <int FORM>
__device__ __forceinline__ f2 ssim_px2(f2 m0, f2 m1, f2 e0, f2 e1, f2 cen, float c1, float c2, f2& cs)
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
    if constexpr (FORM == kFormMulti) {
        const f2 r2 = {__builtin_amdgcn_rcpf(B2.x), __builtin_amdgcn_rcpf(B2.y)};
        cs = A2 * r2;
    }
    return n * r;
}

// What a strip kernel takes by value: one launch (MS-SSIM: one scale of one launch) -- its descriptors, size, strips and cell partials.
template <class PairDesc>
struct Strip2Args {
    const PairDesc* descs;
    uint32_t width, height, strip_rows, strips_x, strips_y;
    uint32_t cells_x, cells_y, cell_shift;
    uint32_t count, xcds;
    double*  partials;            // [image][cell_y][cell_x]; kFormMulti: [image][cell_y][cell_x]{cs, ssim}
    float    c1, c2, range;
    float    gf[MAXR + 1];
};

// Cells are reduced eight at a time (ssim_kernels.hip has the long form): each lane parks its leaf of a cell in LDS, and a
// batch of eight cells is summed as fixed trees -- eight leaves per lane as ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)), then two DPP
// levels over the four lanes of a 32-leaf tree.
enum { CELL_BATCH = 8 };
struct CellBatch { double leaf[CELL_BATCH][64]; };

#define S2_DPP_ADD(t, CTRL) do {                                                                             \
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

// A leaf is the lane's column pair; leaves 0-31 of a batch row are cell 2 sx, leaves 32-63 cell 2 sx + 1.  A cell holds NSUM adjacent
// doubles; which: the one this batch is (kFormMulti: 0 the cs sum, 1 the ssim sum).
template <int NSUM, class Args>
__device__ __forceinline__ void cell_batch_flush(const Args& args, uint32_t img, uint32_t sx, const CellBatch& cb, uint32_t cell_y_first, uint32_t n, uint32_t which)
{
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    double t = cell_batch_local(cb, lane);
    S2_DPP_ADD(t, DPP_QUAD_XOR1);
    S2_DPP_ADD(t, DPP_QUAD_XOR2);
    const uint32_t c = (uint32_t)lane >> 3, cx = 2u * sx + (((uint32_t)lane >> 2) & 1u);
    if ((lane & 3) == 0 && c < n && cx < args.cells_x)
        ((gptr_f64)args.partials)[(((size_t)img * args.cells_y + cell_y_first + c) * args.cells_x + cx) * NSUM + which] = t;
}

enum { ROW_WARMUP = 0, ROW_MAIN = 1, ROW_LAST = 2 };

template <class Sample, int R, int FORM, int MAP, bool WIDE>
__device__ __forceinline__ void strip_body(const Strip2Args<typename Sample::Pair>& args)
{
    static_assert(FORM == kFormSsim || MAP == 0, "a scale of MS-SSIM has no map");
    static_assert(MAP != 2 || R == 5, "the 8-byte map store is radius 5's");
    typedef Shape<R> S;
    typedef typename Sample::Pair PairDesc;
    typedef const PairDesc __attribute__((address_space(1)))* gptr_desc;
    constexpr int PAD = S::PAD, ROW_PX = S::ROW_PX;
    constexpr int N = S::N;                          // ring entries
    constexpr int NWIN = S::NWIN;                    // window pixels of a lane's two columns
    constexpr int NLOAD = S::NLOAD;
    constexpr int NSUM = FORM == kFormMulti ? 2 : 1;
    typedef typename std::conditional<WIDE, int64_t, uint32_t>::type Off;

    __shared__ __attribute__((aligned(16))) Slot<R> ring[2];
    __shared__ __attribute__((aligned(16))) CellBatch cells[NSUM];   // kFormMulti: cs, ssim

    const int lane = threadIdx.x;
    float gf[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) gf[i] = args.gf[i];

    // the strip: image-major, then strip row, then strip column, each XCD walking a contiguous share of that list
    const uint32_t per_img = args.strips_x * args.strips_y;
    const uint32_t id = xcd_order(blockIdx.x, per_img * args.count, args.xcds);
    const uint32_t img = id / per_img, lin = id - img * per_img;
    const uint32_t sy = lin / args.strips_x, sx = lin - sy * args.strips_x;
    PairDesc pd;
    {
        const gptr_desc gd = (gptr_desc)args.descs + img;
        pd.a = (const typename Sample::T*)uniform64((int64_t)gd->a); pd.a_step = uniform64(gd->a_step); pd.a_stride = uniform64(gd->a_stride);
        pd.b = (const typename Sample::T*)uniform64((int64_t)gd->b); pd.b_step = uniform64(gd->b_step); pd.b_stride = uniform64(gd->b_stride);
        pd.map = (float*)uniform64((int64_t)gd->map); pd.map_step = uniform64(gd->map_step); pd.map_stride = uniform64(gd->map_stride);
    }
    const int W = (int)args.width, H = (int)args.height;
    const int x0 = (int)(sx * S::STRIP_W), y0 = (int)(sy * args.strip_rows);
    const int y_end = y0 + (int)args.strip_rows < H ? y0 + (int)args.strip_rows : H;

    // the strip column's centre (see the top of the file), per image
    f2 cen;
    {
        const int64_t cx = x0 + 64 < W ? x0 + 64 : W - 1, cy = (H - 1) / 2;
        const float sa = Sample::load_uniform(pd.a, cx * pd.a_step + cy * pd.a_stride);
        const float sb = Sample::load_uniform(pd.b, cx * pd.b_step + cy * pd.b_stride);
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
        offA[t] = (Off)((int64_t)(xg - refA) * pd.a_step * Sample::BYTES);
        offB[t] = (Off)((int64_t)(xg - refB) * pd.b_step * Sample::BYTES);
    }

    float va[NLOAD], vb[NLOAD];
    auto fetch_to = [&](int r, float (&oa)[NLOAD], float (&ob)[NLOAD]) {     // row r (clamped) -> registers
        const int ry = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
        const gptr_u8 ra = baseA + (int64_t)ry * pd.a_stride * Sample::BYTES;
        const gptr_u8 rb = baseB + (int64_t)ry * pd.b_stride * Sample::BYTES;
#pragma unroll
        for (int t = 0; t < NLOAD; ++t) {
            if constexpr (!WIDE) asm volatile("" : "+v"(offA[t]), "+v"(offB[t]));   // keeps the zero-extension foldable into the load
            oa[t] = Sample::load_bytes(ra, offA[t]);
            ob[t] = Sample::load_bytes(rb, offB[t]);
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
    double colsum[2] = {0.0, 0.0}, colcs[2] = {0.0, 0.0};

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
    const int refM = pd.map_step >= 0 ? x0 : (x0 + S::STRIP_W - 1 < W ? x0 + S::STRIP_W - 1 : W - 1);
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
            f2 cs;
            const f2 v = ssim_px2<FORM>(accAB[0][0], accAB[1][0], accQ[0][0], accQ[1][0], cen, args.c1, args.c2, cs);
            colsum[0] += (double)v.x;
            colsum[1] += (double)v.y;
            if constexpr (FORM == kFormMulti) {
                colcs[0] += (double)cs.x;
                colcs[1] += (double)cs.y;
            }
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
                    if constexpr (MAP == 2) {
                        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
                        const u2 both = {__builtin_bit_cast(uint32_t, v0), __builtin_bit_cast(uint32_t, v1)};
                        __builtin_amdgcn_raw_buffer_store_b64(both, rs, offM[0], 0, 2);
                    } else {
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v0), rs, offM[0], 0, 2);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v1), rs, offM[1], 0, 2);
                    }
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
    // the 2R warm-up rows in pairs (the two LDS slots): Shape<R> has the schedule
    row(r, S0(), Warm(), std::integral_constant<int, 2 * R - 1>()); row(r + 1, S1(), Warm(), std::integral_constant<int, 2 * R - 1>());
    if constexpr (S::WARM_PAIRS == 3) {
        row(r + 2, S0(), Warm(), std::integral_constant<int, 2 * R - 3>()); row(r + 3, S1(), Warm(), std::integral_constant<int, 2 * R - 3>());
        row(r + 4, S0(), Warm(), std::integral_constant<int, 2 * R - 5>()); row(r + 5, S1(), Warm(), std::integral_constant<int, 2 * R - 5>());
    }
    r += 2 * S::WARM_PAIRS;
#pragma unroll 1
    for (int i = S::WARM_PAIRS; i < R; ++i, r += 2) {
        row(r, S0(), Warm(), K0());
        row(r + 1, S1(), Warm(), K0());
    }
    // main rows, one reduction cell at a time; only the image's last cell can be shorter (or odd)
    const int cell_rows = 1 << args.cell_shift;
    uint32_t cell_y = (uint32_t)y0 >> args.cell_shift, parked = 0;
    auto flush = [&]() {
        if constexpr (FORM == kFormMulti) cell_batch_flush<NSUM>(args, img, sx, cells[0], cell_y, parked, 0);
        cell_batch_flush<NSUM>(args, img, sx, cells[NSUM - 1], cell_y, parked, NSUM - 1);
    };
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
        if constexpr (FORM == kFormMulti) cells[0].leaf[parked][lane] = (col_ok[0] ? colcs[0] : 0.0) + (col_ok[1] ? colcs[1] : 0.0);
        cells[NSUM - 1].leaf[parked][lane] = (col_ok[0] ? colsum[0] : 0.0) + (col_ok[1] ? colsum[1] : 0.0);
        colsum[0] = colsum[1] = colcs[0] = colcs[1] = 0.0;
        if (++parked == CELL_BATCH) {
            wave_sync();
            flush();
            wave_sync();
            cell_y += parked;
            parked = 0;
        }
    }
    if (parked) {
        wave_sync();
        flush();
    }
}

// Per-image sum of the cell partials in a fixed order: thread t of 1024 adds cells t, t + 1024, ... in that order, each wave
// runs a fixed xor butterfly, and the 16 wave totals are added in wave order.  One workgroup per image.
constexpr int kStripReduceThreads = 1024;

__device__ __forceinline__ void reduce_body(const double* __restrict__ partials, uint64_t per_image, double* __restrict__ sums)
{
    __shared__ double sh[kStripReduceThreads / 64];
    const double* p = partials + (size_t)blockIdx.x * per_image;
    double acc = 0.0;
    for (uint64_t i = threadIdx.x; i < per_image; i += kStripReduceThreads)
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
        for (int w = 1; w < kStripReduceThreads / 64; ++w)
            t += sh[w];
        sums[blockIdx.x] = t;
    }
}

// ---- the gradient ------------------------------------------------------------------------------------------------------------
// grad_body: one 256-lane workgroup = one 32 x 32 tile of gradient pixels at an absolute position; everything between the
// samples and the gradient stays in LDS.  (The counts below are radius 5's: 10 stands for 2R, 5 for R, 11 for 2R + 1.)
//   1. the (widened,) centred samples (a', b') of the tile + 10 (52 x 52, edge-clamped coordinates) -> LDS;
//   2. row pass of (a', b') and (a'^2 + b'^2, a'b') on 52 rows x 42 columns, folded sums and tap order as the forward kernel;
//   3. column pass on the tile + 5 (42 x 42), in source-row order as the forward kernel; per pixel the SSIM terms and the
//      weighted partials k d_mu, k d_aa, k d_ab (k d_mu of both images when both gradients are wanted: d_bb equals d_aa) -> LDS;
//      a position outside the image holds 0 and reads nothing from gMap: it is not a clamped copy, the clamp is in the adjoint's
//      weights.  A per-pixel k needs no LDS: the work-item that computes a pixel's partials is the one that reads its k, and the load
//      is issued ahead of the column pass, whose 22 LDS reads and 20 fused multiply-adds cover it;
//   4. adjoint row pass (42 rows x 32 columns), 5. adjoint column pass (32 x 32), both as gathers: gradient pixel q collects
//      w(q, j) v(q + j), j = -5 .. 5 in that order, the first product plain, the others fused;  w(q, j) is the tap g|j| in the
//      interior, and on the first (last) row or column the sum of the taps the forward pass clamped onto it from p = q + j:
//      tail[|j|] = g|j| + ... + g5 for j >= 0 (j <= 0), and the sum of all taps on an axis of size 1;
//   6. dLoss/da = Gt(k d_mu_a) + 2 a' Gt(k d_aa) + b' Gt(k d_ab) in fp32 (16-bit samples: rounded once into the samples' encoding),
//      one store per pixel.
// The derivative is taken in the centred variables: d_mu = 2 mu_b A2 / (B1 B2) - 2 mu_a ssim / B1 - 2 mu_a' d_aa - mu_b' d_ab with
// mu = mu' + c.  With taps that sum to 1 this is the header's formula with the terms that cancel across its three summands
// (2 c_a Gt(k d_aa) + c_b Gt(k d_ab) against Gt of the same inside k d_mu) taken out before they are rounded.
// Every gradient pixel is written by one work-item in a fixed order, and the tile grid is fixed by the image: no atomics, the
// same bits in any batch.
enum { GT = kSFTile };

// What a gradient kernel takes by value.
template <class PairDesc, class GradDesc>
struct Grad2Args {
    const PairDesc*     descs;
    const GradDesc*     grads;
    const float*        g_out;       // kKUniform: gOut of pair i at g_out[i] (kKEither: or NULL); kKCoef: k of pair i at g_out[i * g_out_stride]
    const GradOutFDesc* gouts;       // the per-pixel upstream form (kKPerPixel; kKEither: g_out == NULL)
    const GradFDesc*    up;          // kMsUp: the next coarser scale's gradient planes (dense float32)
    uint32_t g_out_stride;
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
template <class Sample, int R, int WHICH, int KFORM = kKUniform, int MS = kMsNone>
__device__ __forceinline__ void grad_body(const Grad2Args<typename Sample::Pair, typename Sample::Grad>& args)
{
    static_assert(R >= 1 && R <= MAXR, "radius");
    static_assert((MS == kMsNone) == (KFORM != kKCoef), "the multi-scale forms read k_s");
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
    const typename Sample::Pair pd = args.descs[img];
    const typename Sample::Grad gd = args.grads[img];
    float gf[R + 1], tail[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) { gf[i] = args.gf[i]; tail[i] = args.tail[i]; }
    // the upstream gradient: one k for the launch's pair, or a plane read per pixel
    const bool per_pixel = KFORM == kKPerPixel || (KFORM == kKEither && args.g_out == nullptr);
    GradOutFDesc go = {nullptr, 0, 0};
    float k_uniform = 0.0f;
    if constexpr (KFORM == kKCoef) k_uniform = ((gptr_cf32)args.g_out)[(size_t)img * args.g_out_stride];
    else if (per_pixel)            go = args.gouts[img];
    else                           k_uniform = (float)((double)((gptr_cf32)args.g_out)[img] / ((double)W * (double)H));
    const gptr_cf32 pk = (gptr_cf32)go.g;

    // kMsUp: the coarser scale's gradient at this pixel, through the adjoint of the clamped box filter: the last column (row) of an
    // odd width (height) was read twice by the clamp.  0.25 c is a power of two: the product is exact.
    auto upstream = [&](const float* gup, int64_t ustep, int64_t ustride, int qx, int qy) -> float {
        if constexpr (MS != kMsUp) return 0.0f;
        const float cx = ((W & 1) && qx == W - 1) ? 2.0f : 1.0f, cy = ((H & 1) && qy == H - 1) ? 2.0f : 1.0f;
        return (0.25f * (cx * cy)) * ((gptr_cf32)gup)[(int64_t)(qx >> 1) * ustep + (int64_t)(qy >> 1) * ustride];
    };
    GradFDesc ud = {nullptr, 0, 0, nullptr, 0, 0};
    if constexpr (MS == kMsUp) ud = args.up[img];

    // k == 0 (a zero weight, gOut == 0, or MS == 0): this scale contributes +0 everywhere, whatever the samples are.
    if constexpr (MS != kMsNone) {
        if (k_uniform == 0.0f) {
            for (int idx = tid; idx < GT * GT; idx += 256) {
                const int y = idx / GT, x = idx - y * GT;
                const int qx = x0 + x, qy = y0 + y;
                if (qx >= W || qy >= H) continue;
                if constexpr (WHICH != 2)
                    Sample::store(gd.ga, (int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride, 0.0f + upstream(ud.ga, ud.ga_step, ud.ga_stride, qx, qy));
                if constexpr (WHICH != 1)
                    Sample::store(gd.gb, (int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride, 0.0f + upstream(ud.gb, ud.gb_step, ud.gb_stride, qx, qy));
            }
            return;
        }
    }

    f2 cen;                                                      // the strip column's centre (top of the file)
    {
        const int xs = x0 & ~(kSFStripW - 1);
        const int64_t cx = xs + 64 < W ? xs + 64 : W - 1, cy = (H - 1) / 2;
        const float sa = Sample::load(pd.a, cx * pd.a_step + cy * pd.a_stride), sb = Sample::load(pd.b, cx * pd.b_step + cy * pd.b_stride);
        cen = f2{__builtin_fabsf(sa) <= args.range ? sa : 0.0f, __builtin_fabsf(sb) <= args.range ? sb : 0.0f};
    }

    // 1. samples
    for (int idx = tid; idx < GIN * GIN; idx += 256) {
        const int j = idx / GIN, i = idx - j * GIN;
        int x = x0 - 2 * R + i, y = y0 - 2 * R + j;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        const f2 v = {Sample::load(pd.a, (int64_t)x * pd.a_step + (int64_t)y * pd.a_stride), Sample::load(pd.b, (int64_t)x * pd.b_step + (int64_t)y * pd.b_stride)};
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
            const float r2 = __builtin_amdgcn_rcpf(B2);
            float dab, daa, dmA, dmB;
            if constexpr (MS != kMsUp) {
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
        const float a = Sample::load(pd.a, (int64_t)qx * pd.a_step + (int64_t)qy * pd.a_stride) - cen.x;
        const float b = Sample::load(pd.b, (int64_t)qx * pd.b_step + (int64_t)qy * pd.b_stride) - cen.y;
        if constexpr (WHICH != 2) {
            const float g = opaque(r[0] + opaque(opaque(2.0f * a) * r[1])) + opaque(b * r[2]);
            Sample::store(gd.ga, (int64_t)qx * gd.ga_step + (int64_t)qy * gd.ga_stride, MS != kMsUp ? g : opaque(g) + upstream(ud.ga, ud.ga_step, ud.ga_stride, qx, qy));
        }
        if constexpr (WHICH != 1) {
            const float g = opaque(r[WHICH == 3 ? 3 : 0] + opaque(opaque(2.0f * b) * r[1])) + opaque(a * r[2]);
            Sample::store(gd.gb, (int64_t)qx * gd.gb_step + (int64_t)qy * gd.gb_stride, MS != kMsUp ? g : opaque(g) + upstream(ud.gb, ud.gb_step, ud.gb_stride, qx, qy));
        }
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------

const uint64_t kMaxBlocks = (uint64_t(1) << 26) - 1;      // x 64 work-items stays below 2^32
const uint64_t kMaxGradBlocks = (uint64_t(1) << 24) - 1;  // x 256 work-items stays below 2^32

inline uint32_t cell_rows_of(uint32_t height) { return height >= 2048 ? 32u : 8u; }

// The engine's taps, centre first: the true 1-D Gaussian, sigma 1.5, normalised over the 11 taps, rounded to float.
inline void default_taps(float (&gf)[MAXR + 1]) { window_taps(MAXR, kSKGaussian, 1.5f, gf); }

inline bool valid_range(float data_range) { return data_range > 0.0f && std::isfinite(data_range); }

// The strips of `count` pairs.  Three waves per SIMD, four SIMDs per CU: a round of strips; pick the strip height (whole cells, at
// most 2048 rows) that finishes the launch's strips in the fewest row-times, `warm_rows` warm-up rows included.
inline GeometryF plan_strips(uint32_t width, uint32_t height, uint32_t count, int cu_count, uint32_t warm_rows)
{
    GeometryF g;
    g.width = width; g.height = height; g.count = count;
    g.cell_rows = cell_rows_of(height);
    g.cells_x = (width + 63) / 64;
    g.cells_y = (height + g.cell_rows - 1) / g.cell_rows;
    g.strips_x = (width + kSFStripW - 1) / kSFStripW;
    const uint64_t slots = (uint64_t)(cu_count > 0 ? cu_count : 256) * 4 * 3;
    const uint64_t cols = (uint64_t)g.strips_x * count;
    uint64_t best = ~uint64_t(0);
    uint32_t best_rows = g.cell_rows;
    for (uint32_t rows = g.cell_rows; rows <= std::max<uint32_t>(g.cell_rows, 2048); rows += g.cell_rows) {
        const uint64_t per_col = (height + rows - 1) / rows;
        const uint64_t rounds = (cols * per_col + slots - 1) / slots;
        const uint64_t cost = rounds * (std::min<uint64_t>(rows, height) + warm_rows);
        if (cost <= best) { best = cost; best_rows = rows; }
        if (rows >= height) break;
    }
    g.strip_rows = best_rows;
    g.strips_y = (height + best_rows - 1) / best_rows;
    return g;
}

// The arguments of a strip launch over `geo`, and its grid.
template <class PairDesc>
inline Strip2Args<PairDesc> fill_strip(const GeometryF& geo, const PairDesc* descs_dev, float data_range, const float (&taps)[MAXR + 1],
                                       int xcd_count, double* partials)
{
    Strip2Args<PairDesc> ka;
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
    for (int i = 0; i <= MAXR; ++i) ka.gf[i] = taps[i];
    return ka;
}
inline dim3 strip_grid(const GeometryF& geo) { return dim3((uint32_t)((uint64_t)geo.strips_x * geo.strips_y * geo.count)); }

// The arguments of a gradient launch over pairs of width x height under the window gf[0 .. radius], and its grid; the caller sets
// the upstream members its form reads (g_out, gouts, up, g_out_stride).
template <class PairDesc, class GradDesc>
inline Grad2Args<PairDesc, GradDesc> fill_grad(uint32_t width, uint32_t height, const PairDesc* descs_dev, const GradDesc* grads_dev,
                                               float data_range, uint32_t radius, const float (&taps)[MAXR + 1])
{
    Grad2Args<PairDesc, GradDesc> ka;
    ka.descs = descs_dev; ka.grads = grads_dev;
    ka.g_out = nullptr; ka.gouts = nullptr; ka.up = nullptr; ka.g_out_stride = 1;
    ka.width = width; ka.height = height;
    ka.tiles_x = (width + kSFTile - 1) / kSFTile; ka.tiles_y = (height + kSFTile - 1) / kSFTile;
    ka.range = data_range;
    ssimf_constants(data_range, ka.c1, ka.c2);
    for (int i = 0; i <= MAXR; ++i) ka.gf[i] = taps[i];
    window_tails(radius, ka.gf, ka.tail, ka.total);
    return ka;
}
template <class Args> inline dim3 grad_grid(const Args& ka, uint32_t count) { return dim3((uint32_t)((uint64_t)ka.tiles_x * ka.tiles_y * count)); }

// Run-time choices -> template arguments: f is called once, with std::integral_constant tags.
template <int V> using Tag = std::integral_constant<int, V>;
template <class F> inline void pick_which(int which, F f) { if (which == 1) f(Tag<1>()); else if (which == 2) f(Tag<2>()); else f(Tag<3>()); }
template <class F> inline void pick_type(int type, F f) { if (type == kSHTypeBF16) f(Tag<kSHTypeBF16>()); else f(Tag<kSHTypeF16>()); }
template <class F> inline void pick_bool(bool b, F f) { if (b) f(std::true_type()); else f(std::false_type()); }
template <class F> inline void pick_radius4(uint32_t radius, F f)       // 1 .. 4
{
    switch (radius) {
    case 1:  f(Tag<1>()); break;
    case 2:  f(Tag<2>()); break;
    case 3:  f(Tag<3>()); break;
    default: f(Tag<4>()); break;
    }
}
// (MAP, WIDE) of a strip launch: the wide form has no 8-byte map store; f(Tag<MAP>, bool tag).
template <class F> inline void pick_map(bool map, bool map_unit, bool wide, F f)
{
    if (wide) {
        if (map) f(Tag<1>(), std::true_type());
        else     f(Tag<0>(), std::true_type());
    } else if (!map)   f(Tag<0>(), std::false_type());
    else if (map_unit) f(Tag<2>(), std::false_type());
    else               f(Tag<1>(), std::false_type());
}

} // namespace
} // namespace ssim_hip

#endif
